"""CPU restatement of DDNM+ (Wang, Yu, Zhang 2023) as dmme_amd.DDNM states it, in torch, float64 or float32: the per-step rows, the
operator A = M o Pool_s o Gray_g and its pseudo-inverse, one step, and the whole walk over any `eps_model` with given normals.  The
reference project has no such sampler: this file is the yardstick, as tests/repaint_ref.py is for RePaint.

Grid 0 = tau_0 < ... < tau_n = T; a level walk (repaint_levels) is cut into downward transitions a -> b = a - 1, each with the upward run
b -> c behind it; the k-th sits at loop index n_rows - k (alpha = abar_a / abar_b, beta = 1 - alpha, var = beta (1 - abar_b)/(1 - abar_a)):
    x0 = A_t x - B_t e               A_t = 1/sqrt(abar_a), B_t = sqrt(1 - abar_a)/sqrt(abar_a)
    r  = m (mean_cell(x0) - y)       a cell: the (C if gray else 1) s s elements one measurement value averages
    xh = x0 - lambda r               lambda = 1 where sigma_y = 0 or sqrt(var) >= ca sigma_y, else sqrt(var)/(ca sigma_y)
    u  = ca xh + cb x [+ cz z0]      ca = sqrt(abar_b) beta/(1 - abar_a), cb = sqrt(alpha) (1 - abar_b)/(1 - abar_a),
                                     cz = sqrt(max(var - (ca lambda sigma_y)^2, 0))
    x' = u, or r0 u + r1 z1          r0 = sqrt(abar_c/abar_b), r1 = sqrt(1 - abar_c/abar_b) where c > b
each bracket only where its coefficient is not zero; for b = 0 the row is exactly (1, 0, 0, A_t, B_t, lambda, 1, 0).  In float32 the rows
are rounded to float32 and every operation is rounded: what the device does up to the order of a cell's sum.  `normals[k]` is the
[2, *shape] block of the k-th step (k = 0 for the first), whatever the step uses of it."""

from __future__ import annotations

from typing import Callable, Dict, Iterable, Sequence

import numpy as np
import torch
from torch import Tensor

from .ddim_ref import alpha_bar  # noqa: F401  (the linear schedule the package holds)
from .repaint_ref import grid  # noqa: F401  (the same grid)

CA, CB, CZ, AT, BT, LAM, R0, R1 = range(8)


def transitions(walk: Sequence[int]):
    """[(a, b, c)]: every step down a -> b = a - 1 of the walk with the level c its following upward run ends at (c = b: none)"""
    out, p, last = [], 0, len(walk) - 1
    while p < last:
        a, b = walk[p], walk[p + 1]
        assert b == a - 1 and b >= 0
        p += 1
        c = b
        while p < last and walk[p + 1] == walk[p] + 1:
            p, c = p + 1, c + 1
        out.append((a, b, c))
    return out


def rows(abar: np.ndarray, grid_: Sequence[int], walk: Sequence[int], sigma_y: float = 0.0):
    """(float64 [n_rows+1][8], t_table): row 0 is never stepped from"""
    ab = np.asarray(abar, dtype=np.float64)
    steps = transitions(list(walk))
    n = len(steps)
    out = np.zeros((n + 1, 8), dtype=np.float64)
    out[0] = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0)
    ttab = [0] * (n + 1)
    for k, (a, b, c) in enumerate(steps):
        i = n - k
        Aa, Bb, Cc = ab[grid_[a]], ab[grid_[b]], ab[grid_[c]]
        ttab[i] = int(grid_[a])
        at, bt = Aa**-0.5, ((1.0 - Aa) / Aa) ** 0.5
        if b == 0:
            out[i] = (1.0, 0.0, 0.0, at, bt, 1.0 if sigma_y == 0.0 else 0.0, 1.0, 0.0)
            continue
        alpha = Aa / Bb
        beta = 1.0 - alpha
        ca = Bb**0.5 * beta / (1.0 - Aa)
        cb = alpha**0.5 * (1.0 - Bb) / (1.0 - Aa)
        var = beta * (1.0 - Bb) / (1.0 - Aa)
        lam = 1.0 if sigma_y == 0.0 or var**0.5 >= ca * sigma_y else var**0.5 / (ca * sigma_y)
        cz = max(var - (ca * lam * sigma_y) ** 2, 0.0) ** 0.5
        r0, r1 = (1.0, 0.0) if c == b else ((Cc / Bb) ** 0.5, (1.0 - Cc / Bb) ** 0.5)
        out[i] = (ca, cb, cz, at, bt, lam, r0, r1)
    return out, ttab


def _row(row, dtype):
    return [float(np.float32(v)) if dtype == torch.float32 else float(v) for v in row]


def cell_mean(x: Tensor, s: int, gray: bool) -> Tensor:
    """Pool_s o Gray_g: (B, C, H, W) -> (B, Cm, H/s, W/s), in x's dtype"""
    B, C, H, W = x.shape
    v = x.reshape(B, C, H // s, s, W // s, s)
    return v.mean(dim=(1, 3, 5)).unsqueeze(1) if gray else v.mean(dim=(3, 5))


def replicate(y: Tensor, s: int, gray: bool, C: int) -> Tensor:
    """(B, Cm, h, w) -> (B, C, s h, s w): every element of a cell gets the cell's value"""
    out = y.repeat_interleave(s, dim=2).repeat_interleave(s, dim=3)
    return out.expand(-1, C, -1, -1) if gray else out


def A(x: Tensor, s: int, gray: bool, mask=None) -> Tensor:
    y = cell_mean(x, s, gray)
    return y if mask is None else mask.to(y.dtype) * y


def A_pinv(y: Tensor, s: int, gray: bool, C: int, mask=None) -> Tensor:
    return replicate(y if mask is None else mask.to(y.dtype) * y, s, gray, C)


def x0_of(x: Tensor, e: Tensor, row, dtype=torch.float64) -> Tensor:
    r = _row(row, dtype)
    return r[AT] * x.to(dtype) - r[BT] * e.to(dtype)


def rectified(x: Tensor, e: Tensor, y: Tensor, m: Tensor, row, s: int, gray: bool, dtype=torch.float64) -> Tensor:
    """xh = x0 - lambda m (mean_cell(x0) - y); y is not looked at where m == 0"""
    r = _row(row, dtype)
    x0 = x0_of(x, e, row, dtype)
    res = torch.where(m != 0, cell_mean(x0, s, gray) - torch.where(m != 0, y.to(dtype), torch.zeros((), dtype=dtype)), torch.zeros((), dtype=dtype))
    return x0 - r[LAM] * replicate(res, s, gray, x.shape[1])


def step(x: Tensor, e: Tensor, y: Tensor, m: Tensor, z2, row, s: int, gray: bool, dtype=torch.float64) -> Tensor:
    """one update in `dtype`; z2: [2, *x.shape], read only where the row's coefficient is not zero"""
    r = _row(row, dtype)
    u = r[CA] * rectified(x, e, y, m, row, s, gray, dtype)
    if r[CB] != 0.0:
        u = u + r[CB] * x.to(dtype)
    if r[CZ] != 0.0:
        u = u + r[CZ] * z2[0].to(dtype)
    if r[R1] != 0.0:
        u = r[R0] * u + r[R1] * z2[1].to(dtype)
    return u


def chain(eps_model: Callable[[Tensor, Tensor], Tensor], x: Tensor, y: Tensor, m: Tensor, tab, ttab, normals, s: int, gray: bool, dtype=torch.float64,
          keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    """the whole walk from loop index n = len(ttab) - 1: {i: the state after the step from index i} for i in `keep`, the final state under 0"""
    x, out, keep = x.to(dtype), {}, set(keep)
    n = len(ttab) - 1
    for k, i in enumerate(range(n, 0, -1)):
        eps = eps_model(x, torch.tensor([ttab[i]]))
        x = step(x, eps, y, m, normals[k], tab[i], s, gray, dtype)
        if i in keep:
            out[i] = x
    out[0] = x
    return out


# ------------------------------------------------------------------------------------------ the error bounds the GPU tests ask for
EPS = 2.0 ** -24  # the unit roundoff of float32


def mean_bound(x: Tensor, s: int, gray: bool) -> Tensor:
    """|fp32 mean of a cell - exact| <= (n + 1) 2^-24 max_cell |x|: the n - 1 rounded sums of a sequential sum miss it by at most
    (n - 1) u sum|x| <= (n - 1) u n max|x|, the division by n brings that to (n - 1) u max|x| and adds its own rounding u max|x|; one u
    more for second order; per cell, float64"""
    B, C, H, W = x.shape
    n = (C if gray else 1) * s * s
    v = x.double().abs().cpu().reshape(B, C, H // s, s, W // s, s)
    mx = v.amax(dim=(1, 3, 5)).unsqueeze(1) if gray else v.amax(dim=(3, 5))
    return (n + 1) * EPS * mx


def update_bound(x, e, y, m, z2, row, s: int, gray: bool) -> Tensor:
    """elementwise, first order in u = 2^-24, with X0 = |A_t x| + |B_t e| >= |x0|, P the cell mean replicated over the cell, n the cell size:
      x0   two products and a difference:                                         3 u X0
      mean its inputs' 3 u P(X0), n - 1 sums and a division:                      (n + 4) u P(X0)
      r    one more difference, |r| <= Rb = m (P(X0) + |y|):                      (n + 5) u P(X0) + u |y|          (0 where m = 0)
      xh   a product and a difference, |xh| <= Hb = X0 + lambda Rb:               4 u X0 + lambda m (n + 8) u (P(X0) + |y|)
      u    up to three products and two sums, |u| <= Ub = |ca| Hb + |cb x| + |cz z0|:   |ca| err(xh) + 3 u Ub
      x'   with a jump two products and a sum more:                               r0 err(u) + 2 u (r0 Ub + |r1 z1|)
    and one Ub more for everything of second order."""
    ca, cb, cz, at, bt, lam, r0, r1 = (abs(float(v)) for v in row)
    x, e, y, m, z2 = (v.double().cpu() for v in (x, e, y, m, z2))
    C = x.shape[1]
    n = (C if gray else 1) * s * s
    X0 = (at * x).abs() + (bt * e).abs()
    yabs = torch.where(m != 0, y.abs(), torch.zeros((), dtype=torch.float64))
    PY = replicate(torch.where(m != 0, cell_mean(X0, s, gray) + yabs, torch.zeros((), dtype=torch.float64)), s, gray, C)
    Hb = X0 + lam * PY
    Ub = ca * Hb + (cb * x).abs() + (cz * z2[0]).abs()
    err_u = ca * (4.0 * X0 + lam * (n + 8) * PY) + 4.0 * Ub
    if r1 == 0.0:
        return EPS * err_u
    return EPS * (r0 * err_u + 2.0 * (r0 * Ub + (r1 * z2[1]).abs()))


def consistency_bound(x0: Tensor, xh: Tensor, y: Tensor, s: int, gray: bool) -> Tensor:
    """(2 n + 4) 2^-24 M per cell, M the largest of |x0|, |xh| and |y| over the cell: what A xh may miss y by on a measured cell with
    lambda = 1, where xh = x0 - (mean(x0) - y) in fp32 - the two means' n + 1 roundings each and the two differences'"""
    B, C, H, W = x0.shape
    n = (C if gray else 1) * s * s
    v = torch.maximum(x0.double().abs().cpu(), xh.double().abs().cpu()).reshape(B, C, H // s, s, W // s, s)
    mx = v.amax(dim=(1, 3, 5)).unsqueeze(1) if gray else v.amax(dim=(3, 5))
    return (2 * n + 4) * EPS * torch.maximum(mx, y.double().abs().cpu())


def update_rows():
    """the four fp32 rows the update is checked on, from the package's tables (T = 100): an interior step and the last step of the
    straight walk at sigma_y = 0, a step with a folded jump (travel 2 / 2), and a step with lambda < 1 (sigma_y = 0.5)"""
    import dmme_amd

    plain = dmme_amd.DDNM(torch.nn.Identity(), 100, 10)._chain_tables()[1]
    travel = dmme_amd.DDNM(torch.nn.Identity(), 100, 10, travel_length=2, travel_repeat=2)._chain_tables()[1]
    noisy = dmme_amd.DDNM(torch.nn.Identity(), 100, 10, sigma_y=0.5)._chain_tables()[1]
    out = {"interior": plain[8], "last": plain[1], "travel": next(r for r in travel[1:] if r[7] != 0.0), "noisy": next(r for r in noisy[2:] if r[5] < 1.0)}
    assert out["interior"][2] != 0.0 and out["interior"][5] == 1.0 and out["interior"][7] == 0.0
    assert out["last"][:3] == (1.0, 0.0, 0.0) and out["last"][5:] == (1.0, 1.0, 0.0)
    assert 0.0 < out["noisy"][5] < 1.0
    return out
