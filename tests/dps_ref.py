"""CPU restatement of DPS (Chung et al., ICLR 2023, Algorithm 1) as dmme_amd.DPS states it, in torch, float64 or float32: the operator
A = M o (Kh . Kw^T) per channel plane and its adjoint, the per-step rows, the adjoint stage, the update, one step and the whole chain over
any differentiable `eps_model` with given normals (torch.autograd.grad gives J_eps^T d_out).  The reference project has no such sampler:
this file is the yardstick, as tests/ilvr_ref.py is for ILVR.

Grid 0 = tau_0 < ... < tau_n = T, the walk n -> 0; row i is the transition a = i -> b = i - 1 (alpha = abar_a / abar_b):
    x0 = A_t x - B_t e;  r = m (y - Kh x0 Kw^T);  g = Kh^T r Kw;  d_out = B_t g;  dx = J_e(x)^T d_out
    u  = c0 (x - c1 e) [+ c2 z]      c0 = 1/sqrt(alpha), c1 = (1 - alpha)/sqrt(1 - abar_a), c2 = sqrt(1 - alpha) (0 where b = 0)
    x' = u + (zeta / n_b)(A_t g - dx)   n_b = ||r_b||, per image; skipped where zeta = 0 or n_b = 0
In float64 the chain uses the float64 rows and matrices; in float32 both rounded to float32 and every operation rounded (the products as
torch.matmul forms them): what the device does up to its summation order.  `normals[k]` is the block of x's shape of the k-th step.

The bounds at the end are derived from the unit roundoff of fp32 and the lengths of the dot products, not measured."""

from __future__ import annotations

from typing import Callable, Dict, Iterable, Sequence

import numpy as np
import torch
from torch import Tensor

from .ddim_ref import alpha_bar  # noqa: F401  (the linear schedule the package holds)
from .ilvr_ref import resize
from .repaint_ref import grid  # noqa: F401  (the same grid)

C0, C1, C2, AT, BT, ZETA = range(6)


# ------------------------------------------------------------------------------------------ the operator
def blur_matrix(n: int, size: int, sigma: float) -> Tensor:
    """float64 [n, n]: a Gaussian of `size` taps along one axis as a band matrix, windows clipped to the axis and renormalised"""
    i = torch.arange(n, dtype=torch.float64)
    d = i[None, :] - i[:, None]
    w = torch.where(d.abs() <= size // 2, torch.exp(-0.5 * (d / sigma) ** 2), torch.zeros_like(d))
    return w / w.sum(dim=1, keepdim=True)


def average_matrix(n: int, s: int) -> Tensor:
    assert n % s == 0
    K = torch.zeros(n // s, n, dtype=torch.float64)
    for p in range(n // s):
        K[p, p * s:(p + 1) * s] = 1.0 / s
    return K


def operator(name: str, H: int, W: int, **kw):
    """float64 (Kh [h, H], Kw [w, W]) of a preset: "identity", "blur" (size, sigma), "bicubic" (scale), "average" (scale)"""
    if name == "identity":
        return torch.eye(H, dtype=torch.float64), torch.eye(W, dtype=torch.float64)
    if name == "blur":
        return blur_matrix(H, kw["size"], kw["sigma"]), blur_matrix(W, kw["size"], kw["sigma"])
    if name == "bicubic":
        return resize(H, H // kw["scale"]), resize(W, W // kw["scale"])
    if name == "average":
        return average_matrix(H, kw["scale"]), average_matrix(W, kw["scale"])
    raise ValueError(name)


def rounded(K: Tensor) -> Tensor:
    """the fp32 matrix the device reads, as float64"""
    return K.to(torch.float32).to(torch.float64)


def A(x: Tensor, Kh: Tensor, Kw: Tensor, mask=None) -> Tensor:
    """M o (Kh x Kw^T) over the last two axes, in x's dtype"""
    y = Kh.to(x.dtype) @ x @ Kw.to(x.dtype).T
    return y if mask is None else torch.where(mask != 0, y, torch.zeros_like(y))


def At(r: Tensor, Kh: Tensor, Kw: Tensor) -> Tensor:
    """Kh^T r Kw over the last two axes (the mask is the caller's: r is zero where nothing is measured)"""
    return Kh.to(r.dtype).T @ r @ Kw.to(r.dtype)


# ------------------------------------------------------------------------------------------ rows, stages, step, chain
def rows(abar: np.ndarray, grid_: Sequence[int], zeta: float):
    """(float64 [n+1][8], t_table): row 0 is never stepped from"""
    ab = np.asarray(abar, dtype=np.float64)
    n = len(grid_) - 1
    out = np.zeros((n + 1, 8), dtype=np.float64)
    out[0, :6] = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    for i in range(1, n + 1):
        a, b = ab[grid_[i]], ab[grid_[i - 1]]
        alpha = a / b
        out[i, :6] = (alpha**-0.5, (1.0 - alpha) / np.sqrt(1.0 - a), 0.0 if i == 1 else np.sqrt(1.0 - alpha), a**-0.5, np.sqrt(1.0 - a) / np.sqrt(a), zeta)
    return out, [int(t) for t in grid_]


def _row(row, dtype):
    return [float(np.float32(v)) if dtype == torch.float32 else float(v) for v in row]


def adjoint(x: Tensor, e: Tensor, y: Tensor, mask, Kh: Tensor, Kw: Tensor, row, dtype=torch.float64):
    """(g, d_out, sumsq [B, C], r) of the adjoint stage in `dtype`; e: the eps plane; y is not looked at where the mask is 0"""
    r_ = _row(row, dtype)
    x, e, y = (v.to(dtype) for v in (x, e, y))
    x0 = r_[AT] * x - r_[BT] * e
    Y = A(x0, Kh, Kw)
    r = y - Y
    if mask is not None:
        r = torch.where(mask != 0, r, torch.zeros_like(r))
    g = At(r, Kh, Kw)
    return g, r_[BT] * g, (r * r).sum(dim=(-2, -1)), r


def update(x: Tensor, e: Tensor, g, dx, sumsq, z, row, dtype=torch.float64) -> Tensor:
    """the update in `dtype` from given g, dx, sumsq [B, C] and normals z (read only where c2 != 0)"""
    r_ = _row(row, dtype)
    x, e = x.to(dtype), e.to(dtype)
    u = r_[C0] * (x - r_[C1] * e)
    if r_[C2] != 0.0:
        u = u + r_[C2] * z.to(dtype)
    if r_[ZETA] == 0.0:
        return u
    nb = sumsq.to(dtype).sum(dim=1).sqrt()
    sc = torch.where(nb != 0, r_[ZETA] / nb.clamp_min(torch.finfo(dtype).tiny), torch.zeros_like(nb)).reshape(-1, 1, 1, 1)
    corr = sc * (r_[AT] * g.to(dtype) - dx.to(dtype))
    return u + torch.where(sc != 0, corr, torch.zeros_like(corr))


def step(eps_model: Callable[[Tensor, Tensor], Tensor], x: Tensor, y: Tensor, mask, Kh: Tensor, Kw: Tensor, row, t: int, z, dtype=torch.float64) -> Tensor:
    """one whole step: the network with autograd, the adjoint stage, J_eps^T d_out, the update"""
    xin = x.detach().to(dtype).requires_grad_(True)
    with torch.enable_grad():
        out = eps_model(xin, torch.tensor([t]))
        e = out[:, : x.shape[1]]
        g, d_out, sumsq, _ = adjoint(xin.detach(), e.detach(), y, mask, Kh, Kw, row, dtype)
        (dx,) = torch.autograd.grad(e, xin, d_out)
    return update(xin.detach(), e.detach(), g, dx, sumsq, z, row, dtype)


def chain(eps_model, x: Tensor, y: Tensor, mask, Kh: Tensor, Kw: Tensor, tab, ttab, normals, dtype=torch.float64, keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    """the whole walk from loop index n = len(ttab) - 1: {i: the state after the step from index i} for i in `keep`, the final state under 0"""
    x, out, keep = x.to(dtype), {}, set(keep)
    n = len(ttab) - 1
    for k, i in enumerate(range(n, 0, -1)):
        x = step(eps_model, x, y, mask, Kh, Kw, tab[i], ttab[i], normals[k], dtype)
        if i in keep:
            out[i] = x
    out[0] = x
    return out


def residual_norm(x: Tensor, y: Tensor, mask, Kh: Tensor, Kw: Tensor) -> float:
    """||m (y - A x)|| over the whole batch, float64"""
    r = y.double() - A(x.double(), Kh.double(), Kw.double())
    if mask is not None:
        r = torch.where(mask != 0, r, torch.zeros_like(r))
    return float(r.norm())


# ------------------------------------------------------------------------------------------ the error bounds the GPU tests ask for
EPS = 2.0 ** -24  # the unit roundoff of float32


def _abs64(*ts):
    return [t.double().abs().cpu() for t in ts]


def measure_bound(x: Tensor, Kh: Tensor, Kw: Tensor) -> Tensor:
    """|fp32(Kh x Kw^T) - exact| <= (H + W + 8) 2^-24 (|Kh| |x| |Kw|^T) elementwise, over the fp32-rounded tables handed in: the standard
    forward error of two chained fp32 dot products of lengths W and H, with or without fma, in any summation order (tests/ilvr_ref.py:
    filter_bound); float64"""
    H, W = x.shape[-2:]
    aKh, ax, aKw = _abs64(Kh, x, Kw)
    return (H + W + 8) * EPS * (aKh @ ax @ aKw.T)


def adjoint_bound(x: Tensor, e: Tensor, y: Tensor, mask, Kh: Tensor, Kw: Tensor, row):
    """(bound on |g - exact| elementwise, bound on |sumsq - exact| [B, C]) for fp32 inputs and the fp32 row, stage by stage, each product
    contributing (chain length + a small constant) 2^-24 of the absolute-value product and each further stage the previous stage's bound
    pushed through the absolute-value matrices:
        e0 = 3 u (|A_t x| + |B_t e|)                                          two products and a difference
        eY = (H + W + 8) u |Kh| |x0| |Kw|^T + |Kh| e0 |Kw|^T                  the measurement's bound, plus x0's rounding carried through
        er = m (eY + u (|r| + eY))                                            one more rounded difference
        eU = (w + 2) u (|r| + er) |Kw| + er |Kw|                              a product of length w
        eg = (h + 2) u |Kh|^T (|r| |Kw| + eU) + |Kh|^T eU                     a product of length h
        ess = sum (2 |r| er + er^2) + (h w + 2) u sum (|r| + er)^2           the squares' own rounding and a sum of h w terms in any order"""
    at, bt = float(row[AT]), float(row[BT])
    x, e, y = (v.double().cpu() for v in (x, e, y))
    Kh, Kw = Kh.double().cpu(), Kw.double().cpu()
    aKh, aKw = Kh.abs(), Kw.abs()
    h, H = Kh.shape
    w, W = Kw.shape
    x0 = at * x - bt * e
    e0 = 3 * EPS * ((at * x).abs() + (bt * e).abs())
    eY = (H + W + 8) * EPS * (aKh @ x0.abs() @ aKw.T) + aKh @ e0 @ aKw.T
    r = y - Kh @ x0 @ Kw.T
    m = torch.ones_like(r) if mask is None else (mask.double().cpu() != 0).double()
    r = torch.where(m != 0, r, torch.zeros_like(r))  # (y may be NaN where nothing is measured)
    er = m * (eY + EPS * (r.abs() + eY))
    eU = (w + 2) * EPS * ((r.abs() + er) @ aKw) + er @ aKw
    eg = (h + 2) * EPS * (aKh.T @ (r.abs() @ aKw + eU)) + aKh.T @ eU
    ess = (2 * r.abs() * er + er * er).sum(dim=(-2, -1)) + (h * w + 2) * EPS * ((r.abs() + er) ** 2).sum(dim=(-2, -1))
    return eg, ess


def update_bound(x: Tensor, e: Tensor, g: Tensor, dx: Tensor, sumsq: Tensor, z, row) -> Tensor:
    """bound on |x' - exact| elementwise for fp32 operands and the fp32 row, first order in u = 2^-24 with 0.1 % for the higher orders:
        u's part     5 u (|c0 x| + |c0 c1 e| + |c2 z|)      c1 e, the difference, c0 ., c2 z and the sum: each term meets at most 4 roundings
        sc = zeta / sqrt(sum_c sumsq): relative error (C + 3) u   (C - 1 sums under a root halve, the root, the quotient)
        v = A_t g - dx: 2 u (|A_t g| + |dx|);   p = sc v: |sc| (C + 6) u (|A_t g| + |dx|)
        the final sum: u (|u| + |p|)"""
    c0, c1, c2, at, zeta = (float(row[k]) for k in (C0, C1, C2, AT, ZETA))
    x, e = x.double().cpu(), e.double().cpu()
    U = (c0 * x).abs() + (c0 * c1 * e).abs()
    if c2 != 0.0:
        U = U + (c2 * z.double().cpu()).abs()
    bound = 5 * EPS * U
    absu, absp = U, torch.zeros_like(U)
    if zeta != 0.0:
        Cc = x.shape[1]
        nb = sumsq.double().cpu().sum(dim=1).sqrt()
        sc = torch.where(nb != 0, zeta / nb.clamp_min(1e-300), torch.zeros_like(nb)).reshape(-1, 1, 1, 1)
        V = (at * g.double().cpu()).abs() + dx.double().cpu().abs()
        bound = bound + sc * (Cc + 6) * EPS * V
        absp = sc * V
    return 1.001 * (bound + EPS * (absu + absp))
