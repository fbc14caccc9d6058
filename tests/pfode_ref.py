"""CPU restatement of the probability-flow ODE walks as dmme_amd.ProbabilityFlow states them (Song et al., ICLR 2021, section 4.3 and
appendix D.2), in numpy / torch, float64 or float32: the stage tables from the closed forms, the four-term stage update with its save rule,
the Rademacher probe and the dequantisation on tests/philox_ref.py's words, the probe dot, the latent's log-density, and the assembled walks
over any differentiable `eps_model` (torch.autograd.grad gives J^T z).  The reference project has no such sampler: this file is the yardstick.

    sig(t) = sqrt((1 - abar_t) / abar_t);  step a -> b:  k0 = sqrt(abar_b / abar_a),  k1 = sqrt(1 - abar_b) - k0 sqrt(1 - abar_a),  h = sig(b) - sig(a)
    stage A (t = a):  x' = k0 x_a + k1 e_a                         w_A = (h / 2) sqrt(abar_a)
    stage B (t = b):  x_b = k0 x_a + (k1 / 2)(e_a + e_b)           w_B = (h / 2) sqrt(abar_b)
    log p(x_0) = log N(x_T; 0, I) + (D / 2)(ln abar_{g_n} - ln abar_{g_0}) + sum_k w_k z_k^T J_k z_k

The bounds are derived from the unit roundoff of fp32 and the number of rounded operations, not measured."""

from __future__ import annotations

import math
from typing import Callable, List, Sequence

import numpy as np
import torch
from torch import Tensor

from . import philox_ref as P
from .ddim_ref import alpha_bar  # noqa: F401  (the linear schedule the package holds)

U = 2.0 ** -24  # unit roundoff of fp32
C0, C1, C2, C3, W, SAVE = range(6)
LN_2PI = math.log(2.0 * math.pi)


def sig(ab: np.ndarray, t: int) -> float:
    return float(np.sqrt((1.0 - ab[t]) / ab[t]))


def heun(ab: np.ndarray, a: int, b: int):
    """(k0, k1, h) of the step a -> b in float64"""
    k0 = np.sqrt(ab[b] / ab[a])
    return float(k0), float(np.sqrt(1.0 - ab[b]) - k0 * np.sqrt(1.0 - ab[a])), sig(ab, b) - sig(ab, a)


def stages(ab, grid: Sequence[int], direction: str, likelihood: bool = False, final_denoise: bool = True, euler: bool = False):
    """the walk as a list of (row [8] float64, t) in the order the stages run; `euler`: stage A alone with the whole step's weight"""
    ab = np.asarray(ab, dtype=np.float64)
    g = list(grid)
    m = len(g) - 1
    pairs = [(g[j], g[j + 1]) for j in range(m)] if direction == "encode" else [(g[m - j], g[m - j - 1]) for j in range(m)]
    out = []
    for a, b in pairs:
        k0, k1, h = heun(ab, a, b)
        if euler:
            out.append((np.array([k0, 0, k1, 0, h * np.sqrt(ab[a]) if likelihood else 0.0, 0, 0, 0]), a))
            continue
        wa, wb = (0.5 * h * np.sqrt(ab[a]), 0.5 * h * np.sqrt(ab[b])) if likelihood else (0.0, 0.0)
        out.append((np.array([k0, 0, k1, 0, wa, 1, 0, 0]), a))
        out.append((np.array([0, k0, 0.5 * k1, 0.5 * k1, wb, 0, 0, 0]), b))
    if direction == "decode" and final_denoise:
        a = pairs[-1][1]
        out.append((np.array([1.0 / np.sqrt(ab[a]), 0, -np.sqrt(1.0 - ab[a]) / np.sqrt(ab[a]), 0, 0, 0, 0, 0]), a))
    return out


def tables(ab, grid, direction, likelihood=False, final_denoise=True):
    """(rows [n + 1][8], t_table [n + 1]) in the package's loop-index order: stage k at index n - k, row 0 never stepped from"""
    st = stages(ab, grid, direction, likelihood, final_denoise)
    n = len(st)
    rows = np.zeros((n + 1, 8))
    rows[0, 0] = 1.0
    ttab = [st[-1][1]] * (n + 1)
    for k, (row, t) in enumerate(st):
        rows[n - k], ttab[n - k] = row, t
    return rows, ttab


# ------------------------------------------------------------------------------------------ the stage update
def stage(x: Tensor, xs: Tensor, e: Tensor, es: Tensor, row, dtype=torch.float64):
    """(x_new, xs, es) in `dtype`: x_new = c0 x + c1 xs + c2 e + c3 es with zero-coefficient terms left out; xs <- x, es <- e where save.
    float32: the device's order of operations, a rounded product and three fused multiply-adds (numpy has no fma: each is formed in
    float64 from float32 operands and rounded once, which is exact enough to be the fma except in double-rounding corner cases)"""
    c = [float(v) for v in row[:4]]
    ops = [x, xs, e, es]
    if dtype == torch.float64:
        r = torch.zeros_like(x, dtype=torch.float64)
        for cj, oj in zip(c, ops):
            if cj != 0.0:
                r = r + cj * oj.double()
    else:
        r = torch.zeros_like(x, dtype=torch.float32)
        for cj, oj in zip(c, ops):
            if cj != 0.0:
                r = (float(np.float32(cj)) * oj.float().double() + r.double()).float()
    if float(row[SAVE]) != 0.0:
        xs, es = x.clone(), e.clone()
    return r, xs, es


def stage_bound(x, xs, e, es, row) -> Tensor:
    """|device - float64| elementwise: one rounded product and at most three fused multiply-adds, each off by at most u of its own
    result, which the sum of the terms' magnitudes bounds (to first order; the factor 4 covers the (1 + u)^3 growth with room)"""
    c = [abs(float(v)) for v in row[:4]]
    tot = torch.zeros_like(x, dtype=torch.float64)
    for cj, oj in zip(c, (x, xs, e, es)):
        if cj != 0.0:
            tot = tot + cj * oj.double().abs()
    return 4.0 * U * tot


# ------------------------------------------------------------------------------------------ probe, dequantisation, dot, prior
def rademacher(seed: int, offset: int, numel: int) -> np.ndarray:
    """float32[numel]: -1 where bit 31 of the element's word of the span is set, else +1"""
    w = P._span_words(seed, offset, numel).reshape(-1)[: int(numel)]
    return np.where((w >> np.uint32(31)) != 0, np.float32(-1.0), np.float32(1.0)).astype(np.float32)


def probe(seed: int, offset: int, B: int, chw: int, planes: int = 1) -> np.ndarray:
    """float32 (B, planes * chw): the span's values in the eps plane, zeros behind it"""
    z = rademacher(seed, offset, B * chw).reshape(B, chw)
    return np.concatenate([z] + [np.zeros_like(z)] * (planes - 1), axis=1)


def dequantize(x: np.ndarray, seed: int, offset: int) -> np.ndarray:
    """float32, bit for bit: x + fp32((u - 0.5) * fp32(2 / 255)), the difference exact"""
    x = np.asarray(x, dtype=np.float32)
    u = P.uniforms(seed, offset, x.size).astype(np.float32).reshape(x.shape)
    return (x + (u - np.float32(0.5)) * np.float32(2.0 / 255.0)).astype(np.float32)


def dot(z: Tensor, dx: Tensor) -> Tensor:
    """float64 [B]: sum z dx per image"""
    B = z.shape[0]
    return (z.double().reshape(B, -1) * dx.double().reshape(B, -1)).sum(dim=1)


def dot_bound(z: Tensor, dx: Tensor) -> Tensor:
    """|device - float64| per image: a sum of D terms in any order, the last rounding to fp32 of the double finish included"""
    B = z.shape[0]
    D = z[0].numel()
    return (D + 8) * U * (z.double().reshape(B, -1) * dx.double().reshape(B, -1)).abs().sum(dim=1)


def prior(x: Tensor) -> Tensor:
    """float64 [B]: log N(x; 0, I)"""
    B = x.shape[0]
    D = x[0].numel()
    return -0.5 * x.double().reshape(B, -1).pow(2).sum(dim=1) - 0.5 * D * LN_2PI


def prior_bound(x: Tensor) -> Tensor:
    B = x.shape[0]
    D = x[0].numel()
    return 0.5 * (D + 8) * U * x.double().reshape(B, -1).pow(2).sum(dim=1)


# ------------------------------------------------------------------------------------------ the assembled walks
def walk(eps_model: Callable, x: Tensor, ab, grid, direction: str, dtype=torch.float64, final_denoise: bool = True) -> Tensor:
    """the no-grad walk; in float32 the rows are rounded once, as the package rounds them"""
    x = x.to(dtype)
    xs, es = torch.zeros_like(x), torch.zeros_like(x)
    with torch.no_grad():
        for row, t in stages(ab, grid, direction, False, final_denoise):
            if dtype == torch.float32:
                row = row.astype(np.float32).astype(np.float64)
            e = eps_model(x, torch.tensor([t]))[:, : x.shape[1]].to(dtype)
            x, xs, es = stage(x, xs, e, es, row, dtype)
    return x


def likelihood(eps_model: Callable, x0: Tensor, ab, grid, probes: Callable[[int], Tensor], dtype=torch.float64, rows32: bool = True):
    """the likelihood walk g_0 -> g_n on given probes (`probes(k)`: the +-1 tensor of x's shape of stage k).  The rows are the package's
    (rounded to fp32 once) unless rows32 is False.  Returns a dict: log_p, prior, acc (float64 [B]), latent, and per stage s [B], w, max |dx|."""
    ab = np.asarray(ab, dtype=np.float64)
    x = x0.to(dtype)
    B, D = x.shape[0], x[0].numel()
    xs, es = torch.zeros_like(x), torch.zeros_like(x)
    acc = torch.zeros(B, dtype=torch.float64)
    trace, ws, dxmax = [], [], []
    for k, (row, t) in enumerate(stages(ab, grid, "encode", True)):
        if rows32:
            row = row.astype(np.float32).astype(np.float64)
        z = probes(k).to(dtype)
        xin = x.detach().clone().requires_grad_(True)
        e = eps_model(xin, torch.tensor([t]))[:, : x.shape[1]]
        (dx,) = torch.autograd.grad(e, xin, z)
        s = dot(z, dx) if dtype == torch.float64 else (z * dx).reshape(B, -1).sum(dim=1).double()
        acc = acc + float(row[W]) * s
        trace.append(s)
        ws.append(float(row[W]))
        dxmax.append(float(dx.detach().abs().max()))
        x, xs, es = stage(x, xs, e.detach().to(dtype), es, row, dtype)
    pr = prior(x) if dtype == torch.float64 else (-0.5 * x.reshape(B, -1).pow(2).sum(dim=1).double() - 0.5 * D * LN_2PI)
    log_p = pr + 0.5 * D * (math.log(ab[grid[-1]]) - math.log(ab[grid[0]])) + acc
    return dict(log_p=log_p, prior=pr, acc=acc, latent=x.detach(), s=trace, w=ws, dxmax=dxmax)


def bits_per_dim(log_p: Tensor, D: int) -> Tensor:
    return -log_p / (D * math.log(2.0)) + math.log2(255.0 / 2.0)


# ------------------------------------------------------------------------------------------ the analytic Gaussian problem
def gaussian_loglik(ab, grid, x0: np.ndarray, var: float = 0.25, euler: bool = False) -> float:
    """log p(x0) by the walk for data N(0, var I) in float64: eps(x, t) = sqrt(1 - abar) x / (var abar + 1 - abar), whose Jacobian is
    diagonal, so z^T J z = tr J for every +-1 probe"""
    ab = np.asarray(ab, dtype=np.float64)
    x = np.asarray(x0, dtype=np.float64).copy()
    D = x.size
    coef = lambda t: np.sqrt(1.0 - ab[t]) / (var * ab[t] + 1.0 - ab[t])
    xs, es, acc = np.zeros_like(x), np.zeros_like(x), 0.0
    for row, t in stages(ab, grid, "encode", True, euler=euler):
        e = coef(t) * x
        acc += row[W] * D * coef(t)
        new = row[C0] * x + row[C1] * xs + row[C2] * e + row[C3] * es
        if row[SAVE] != 0:
            xs, es = x, e
        x = new
    return float(-0.5 * (x * x).sum() - 0.5 * D * LN_2PI + 0.5 * D * (np.log(ab[grid[-1]]) - np.log(ab[grid[0]])) + acc)


def gaussian_exact(ab, t: int, x0: np.ndarray, var: float = 0.25) -> float:
    """log p_t(x0) of the noised Gaussian: N(0, (var abar_t + 1 - abar_t) I)"""
    ab = np.asarray(ab, dtype=np.float64)
    v = var * ab[t] + 1.0 - ab[t]
    x = np.asarray(x0, dtype=np.float64)
    return float(-0.5 * (x * x).sum() / v - 0.5 * x.size * np.log(2.0 * np.pi * v))
