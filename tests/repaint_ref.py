"""CPU restatement of RePaint inpainting (Lugmayr et al. 2022) and SDEdit editing (Meng et al. 2022) as dmme_amd.RePaint states them,
in float64 or float32: the level walk, the fold of an upward run into one Gaussian, the per-step rows, one step, and whole chains over
any `eps_model`.  The reference project has neither sampler: this file is the yardstick, as tests/dpmpp_ref.py is for DPM-Solver++.

Grid 0 = tau_0 < ... < tau_n = T, level k = noise level tau_k.  One row per downward transition a -> b = a - 1, with the upward run
b -> c that follows it folded in (alpha = abar_a / abar_b, beta = 1 - alpha, abar at tau_a, tau_b, tau_c):
    u  = c0 (x - c1 e) [+ c2 z0]     c0 = 1/sqrt(alpha), c1 = beta/sqrt(1 - abar_a), c2 = sqrt(beta) (0 where b = 0)
    k  = ka x0 [+ ks z1]             ka = sqrt(abar_b), ks = sqrt(1 - abar_b)
    y  = m k + (1 - m) u
    x' = y, or r0 y + r1 z2          r0 = prod sqrt(alpha_l), r1 = sqrt(1 - prod alpha_l) over the levels l = b+1 .. c of the run
each bracket only where its coefficient is not zero.  In float64 the chains use the float64 rows; in float32 the rows rounded to
float32, every product, sum and difference rounded: what the device does.  The whole-chain functions take the normals as an argument:
`normals[k]` is the [3, *shape] block of the k-th step (k = 0 for the first), whatever the step uses of it."""

from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from oracle import diffusion as D

from .ddim_ref import alpha_bar  # noqa: F401  (the linear schedule the package holds)

C0, C1, C2, KA, KS, R0, R1 = range(7)


def grid(abar: np.ndarray, n: int) -> List[int]:
    """0 followed by the strictly increasing timesteps of DDIM's linear tau table"""
    T = len(abar) - 1
    return [0] + sorted({int(v) for v in D.tau_table(T, n, "linear") if int(v) > 0})


def levels(n: int, j: int, r: int) -> List[int]:
    """the walk, built stretch by stretch instead of step by step: down to the highest level that has room to jump (l = 1 + m j with
    l + j <= n), there r - 1 times (up j levels, down j levels), on to the next such level below, ..., from level 1 down to 0"""
    out, k = [n], n
    for l in sorted((l for l in range(1, n + 1, j) if l + j <= n), reverse=True):
        out += list(range(k - 1, l - 1, -1))
        for _ in range(r - 1):
            out += list(range(l + 1, l + j + 1)) + list(range(l + j - 1, l - 1, -1))
        k = l
    return out + list(range(k - 1, -1, -1))


def down_count(n: int, j: int, r: int) -> int:
    return n + (r - 1) * j * ((n - 1) // j)


def fold(abar: np.ndarray, grid_: Sequence[int], b: int, c: int) -> Tuple[float, float]:
    """(r0, r1) of the run b -> c as the composition of its single forward steps x <- sqrt(alpha_l) x + sqrt(1 - alpha_l) z: the mean
    factors multiply, the variances add up to 1 - prod alpha_l"""
    prod = 1.0
    r0 = 1.0
    for l in range(b + 1, c + 1):
        a = abar[grid_[l]] / abar[grid_[l - 1]]
        r0 *= np.sqrt(a)
        prod *= a
    return float(r0), float(np.sqrt(1.0 - prod))


def transitions(walk: Sequence[int]) -> List[Tuple[int, int, int]]:
    """(a, b, c) per downward transition, in walk order"""
    out, p = [], 0
    while p + 1 < len(walk):
        a, b = walk[p], walk[p + 1]
        assert b == a - 1, (a, b)
        p += 1
        while p + 1 < len(walk) and walk[p + 1] > walk[p]:
            p += 1
        out.append((a, b, walk[p]))
    return out


def rows(abar: np.ndarray, grid_: Sequence[int], walk: Sequence[int]):
    """(float64 [n_rows+1][8], t_table): the k-th transition at loop index n_rows - k; row 0 is never stepped from"""
    ab = np.asarray(abar, dtype=np.float64)
    tr = transitions(walk)
    n_rows = len(tr)
    out = np.zeros((n_rows + 1, 8), dtype=np.float64)
    out[0, :7] = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0)
    ttab = [0] * (n_rows + 1)
    for k, (a, b, c) in enumerate(tr):
        A, Bb = ab[grid_[a]], ab[grid_[b]]
        alpha = A / Bb
        r0, r1 = (1.0, 0.0) if c == b else fold(ab, grid_, b, c)
        out[n_rows - k, :7] = (1.0 / np.sqrt(alpha), (1.0 - alpha) / np.sqrt(1.0 - A), np.sqrt(1.0 - alpha) if b > 0 else 0.0, np.sqrt(Bb), np.sqrt(1.0 - Bb),
                               r0, r1)
        ttab[n_rows - k] = grid_[a]
    return out, ttab


def _row(row, dtype):
    return [float(np.float32(v)) if dtype == torch.float32 else float(v) for v in row]


def step(x: Tensor, e: Tensor, x0: Tensor, m: Tensor, z3: Optional[Tensor], row, dtype=torch.float64) -> Tensor:
    """one update in `dtype`, each product, sum and difference rounded; z3: [3, *x.shape], read only where the row's coefficient is not zero"""
    r = _row(row, dtype)
    x, e, x0, m = (v.to(dtype) for v in (x, e, x0, m))
    u = r[C0] * (x - r[C1] * e)
    if r[C2] != 0.0:
        u = u + r[C2] * z3[0].to(dtype)
    k = r[KA] * x0
    if r[KS] != 0.0:
        k = k + r[KS] * z3[1].to(dtype)
    y = m * k + (1.0 - m) * u
    return r[R0] * y + r[R1] * z3[2].to(dtype) if r[R1] != 0.0 else y


def chain(eps_model: Callable[[Tensor, Tensor], Tensor], x: Tensor, x0: Tensor, m: Tensor, tab, ttab, first: int, normals, dtype=torch.float64,
          keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    """`first` steps from loop index `first`: {i: the state after the step from index i} for i in `keep`, the final state under 0"""
    x, out, keep = x.to(dtype), {}, set(keep)
    for k, i in enumerate(range(first, 0, -1)):
        eps = eps_model(x, torch.tensor([ttab[i]]))
        x = step(x, eps, x0, m, normals[k], tab[i], dtype)
        if i in keep:
            out[i] = x
    out[0] = x
    return out


def inpaint(eps_model, x_T: Tensor, x0: Tensor, m: Tensor, abar: np.ndarray, grid_: Sequence[int], j: int, r: int, normals, dtype=torch.float64,
            keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    """the whole RePaint walk from x_T"""
    tab, ttab = rows(abar, grid_, levels(len(grid_) - 1, j, r))
    return chain(eps_model, x_T, x0, m, tab, ttab, len(ttab) - 1, normals, dtype, keep)


def edit_level(n: int, strength: float) -> int:
    return min(n, max(1, int(round(strength * n))))


def edit(eps_model, guide: Tensor, m: Tensor, abar: np.ndarray, grid_: Sequence[int], strength: float, z_guide: Tensor, normals, dtype=torch.float64):
    """SDEdit: the guide noised to level k with z_guide, then the plain walk k -> 0 (loop index = level)"""
    n = len(grid_) - 1
    k = edit_level(n, strength)
    ab = float(abar[grid_[k]])
    sa, sd = (float(np.float32(np.sqrt(ab))), float(np.float32(np.sqrt(1 - ab)))) if dtype == torch.float32 else (np.sqrt(ab), np.sqrt(1 - ab))
    x_k = sa * guide.to(dtype) + sd * z_guide.to(dtype)
    tab, ttab = rows(abar, grid_, list(range(n, -1, -1)))
    return chain(eps_model, x_k, guide, m, tab, ttab, k, normals, dtype)[0]
