"""CPU restatement of ILVR (Choi et al. 2021) as dmme_amd.ILVR states it, in torch, float64 or float32: the low-pass matrix, the per-step
rows, one step, and the whole chain over any `eps_model` with given normals.  The reference project has no such sampler: this file is the
yardstick, as tests/repaint_ref.py is for RePaint.

Grid 0 = tau_0 < ... < tau_n = T, the walk n -> 0; row i is the transition a = i -> b = i - 1 (alpha = abar_a / abar_b):
    u  = c0 (x - c1 e) [+ c2 z0]     c0 = 1/sqrt(alpha), c1 = (1 - alpha)/sqrt(1 - abar_a), c2 = sqrt(1 - alpha) (0 where b = 0)
    k  = ka y [+ ks z1]              ka = sqrt(abar_b), ks = sqrt(1 - abar_b)
    x' = u + Ph (k - u) Pw^T         where g = 1 (b >= range_level), else x' = u
each bracket only where its coefficient is not zero.  In float64 the chain uses the float64 rows and matrices; in float32 both rounded to
float32 and every operation rounded (the products as torch.matmul forms them): what the device does up to its summation order.
`normals[k]` is the [2, *shape] block of the k-th step (k = 0 for the first), whatever the step uses of it."""

from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Sequence

import numpy as np
import torch
from torch import Tensor

from .ddim_ref import alpha_bar  # noqa: F401  (the linear schedule the package holds)
from .repaint_ref import grid  # noqa: F401  (the same grid)

C0, C1, C2, KA, KS, G = range(6)


def _kernel(x: Tensor, a: float = -0.5) -> Tensor:
    """Keys' cubic convolution kernel"""
    x = x.abs()
    inner = (a + 2.0) * x**3 - (a + 3.0) * x**2 + 1.0
    outer = a * (x**3 - 5.0 * x**2 + 8.0 * x - 4.0)
    return torch.where(x < 1.0, inner, torch.where(x < 2.0, outer, torch.zeros_like(x)))


def resize(n_in: int, n_out: int) -> Tensor:
    """float64 [n_out, n_in]: antialiased bicubic resampling of one axis, pixel centres at half-integers (align_corners=False).  All taps
    at once: tap j of output i weighs kernel((j + 1/2 - centre_i) / stretch), stretch = max(n_in / n_out, 1), inside the window
    [round(centre - 2 stretch), round(centre + 2 stretch)) clipped to the axis; rows renormalised"""
    scale = n_in / n_out
    stretch = max(scale, 1.0)
    centre = scale * (torch.arange(n_out, dtype=torch.float64) + 0.5)
    j = torch.arange(n_in, dtype=torch.float64)
    lo = torch.clamp(torch.trunc(centre - 2.0 * stretch + 0.5), min=0)
    hi = torch.clamp(torch.trunc(centre + 2.0 * stretch + 0.5), max=n_in)
    w = _kernel((j[None, :] + 0.5 - centre[:, None]) / stretch)
    w = torch.where((j[None, :] >= lo[:, None]) & (j[None, :] < hi[:, None]), w, torch.zeros_like(w))
    return w / w.sum(dim=1, keepdim=True)


def lowpass_matrix(n: int, N: int) -> Tensor:
    """float64 [n, n]: up o down along one axis"""
    assert n % N == 0 and N >= 2
    return resize(n // N, n) @ resize(n, n // N)


def rows(abar: np.ndarray, grid_: Sequence[int], range_level: int = 0):
    """(float64 [n+1][8], t_table): row 0 is never stepped from"""
    ab = np.asarray(abar, dtype=np.float64)
    n = len(grid_) - 1
    out = np.zeros((n + 1, 8), dtype=np.float64)
    out[0, :6] = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    for i in range(1, n + 1):
        A, Bb = ab[grid_[i]], ab[grid_[i - 1]]
        alpha = A / Bb
        last = i == 1
        out[i, :6] = (alpha**-0.5, (1.0 - alpha) / np.sqrt(1.0 - A), 0.0 if last else np.sqrt(1.0 - alpha), np.sqrt(Bb), np.sqrt(1.0 - Bb),
                      1.0 if i - 1 >= range_level else 0.0)
    return out, [int(t) for t in grid_]


def _row(row, dtype):
    return [float(np.float32(v)) if dtype == torch.float32 else float(v) for v in row]


def low_pass(d: Tensor, Ph: Tensor, Pw: Tensor) -> Tensor:
    """Ph d Pw^T over the last two axes, in d's dtype"""
    return Ph.to(d.dtype) @ d @ Pw.to(d.dtype).T


def step(x: Tensor, e: Tensor, y: Tensor, z2, row, Ph: Tensor, Pw: Tensor, dtype=torch.float64) -> Tensor:
    """one update in `dtype`; z2: [2, *x.shape], read only where the row's coefficient is not zero; Ph, Pw: float64 matrices (float32:
    rounded here)"""
    r = _row(row, dtype)
    x, e, y = (v.to(dtype) for v in (x, e, y))
    u = r[C0] * (x - r[C1] * e)
    if r[C2] != 0.0:
        u = u + r[C2] * z2[0].to(dtype)
    if r[G] == 0.0:
        return u
    k = r[KA] * y
    if r[KS] != 0.0:
        k = k + r[KS] * z2[1].to(dtype)
    return u + low_pass(k - u, Ph.to(dtype), Pw.to(dtype))


def chain(eps_model: Callable[[Tensor, Tensor], Tensor], x: Tensor, y: Tensor, tab, ttab, normals, Ph: Tensor, Pw: Tensor, dtype=torch.float64,
          keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    """the whole walk from loop index n = len(ttab) - 1: {i: the state after the step from index i} for i in `keep`, the final state under 0"""
    x, out, keep = x.to(dtype), {}, set(keep)
    n = len(ttab) - 1
    for k, i in enumerate(range(n, 0, -1)):
        eps = eps_model(x, torch.tensor([ttab[i]]))
        x = step(x, eps, y, normals[k], tab[i], Ph, Pw, dtype)
        if i in keep:
            out[i] = x
    out[0] = x
    return out


def sample_like(eps_model, x_T: Tensor, y: Tensor, abar: np.ndarray, grid_: List[int], N: int, range_level: int, normals, dtype=torch.float64,
                keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    tab, ttab = rows(abar, grid_, range_level)
    H, W = x_T.shape[-2:]
    return chain(eps_model, x_T, y, tab, ttab, normals, lowpass_matrix(H, N), lowpass_matrix(W, N), dtype, keep)


# ------------------------------------------------------------------------------------------ the error bounds the GPU tests ask for
EPS = 2.0 ** -24  # the unit roundoff of float32


def filter_bound(d: Tensor, Ph: Tensor, Pw: Tensor) -> Tensor:
    """|fp32(Ph d Pw^T) - exact| <= (H + W + 8) 2^-24 (|Ph| |d| |Pw|^T) elementwise, over the fp32-rounded tables handed in: the standard
    forward error of two chained fp32 dot products of lengths W and H, with or without fma, in any summation order; float64"""
    H, W = d.shape[-2:]
    return (H + W + 8) * EPS * (Ph.double().abs().cpu() @ d.double().abs().cpu() @ Pw.double().abs().cpu().T)


def update_bound(x, e, y, z2, row, Ph, Pw) -> Tensor:
    """2^-24 [8 A + (H + W + 16) (|Ph| A |Pw|^T)] elementwise, A = |c0 x| + |c0 c1 e| + |c2 z0| + |ka y| + |ks z1|: a few roundings of u, k,
    d and the final sum (each at most 2^-24 of a value that A bounds), the filter's bound with |d| <= A, and d's own rounding carried
    through |Ph| . |Pw|^T (the 8 added to the filter's H + W + 8).  An unconditioned row: 2^-24 8 A with A of the reverse step alone."""
    c0, c1, c2, ka, ks, g = (float(v) for v in row[:6])
    x, e, y, z2 = (v.double().cpu() for v in (x, e, y, z2))
    A = (c0 * x).abs() + (c0 * c1 * e).abs() + (c2 * z2[0]).abs()
    if g == 0.0:
        return EPS * 8 * A
    H, W = x.shape[-2:]
    A = A + (ka * y).abs() + (ks * z2[1]).abs()
    return EPS * (8 * A + (H + W + 16) * (Ph.double().abs().cpu() @ A @ Pw.double().abs().cpu().T))


def update_rows(N: int = 4):
    """the three fp32 rows the update is checked on, from the package's tables (T = 100, 10 levels): an interior conditioned step, the
    last step (conditioned, c2 = ks = 0) and an unconditioned step (range_level = 4, the transition 3 -> 2)"""
    import dmme_amd

    cond = dmme_amd.ILVR(torch.nn.Identity(), 100, 10, N, 0)._chain_tables()[1]
    free = dmme_amd.ILVR(torch.nn.Identity(), 100, 10, N, 4)._chain_tables()[1]
    out = {"interior": cond[8], "last": cond[1], "unconditioned": free[3]}
    assert out["interior"][2] != 0.0 and out["interior"][4] != 0.0 and out["interior"][5] == 1.0
    assert out["last"][2] == 0.0 and out["last"][4] == 0.0 and out["last"][5] == 1.0 and out["unconditioned"][5] == 0.0 and out["unconditioned"][2] != 0.0
    return out
