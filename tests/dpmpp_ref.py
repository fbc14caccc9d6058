"""CPU restatement of DPM-Solver++(2M) (dmme_amd.DPMSolverPP; Lu et al. 2022, the multistep second-order solver in data-prediction
form) in float64 or float32: the timestep grid, the per-index rows, one step, whole chains over any `eps_model`, and the
classifier-free mix.  The reference project has no such sampler: this file is the yardstick, as tests/ddim_ref.py is for the
paper-form DDIM sampler.

alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = log(alpha_t / sigma_t); grid tau_0 = 0 < ... < tau_n = T.  Step from
index i (a = tau_i) to i - 1 (p = tau_{i-1}), h = lambda_p - lambda_a:
    x0 = q0 x + q1 e   (q0 = 1/alpha_a, q1 = -sigma_a/alpha_a; clamped to [-1, 1] iff clip)
    D  = x0 + w (x0 - x0_prev) where the history is valid, else x0      (w = h / (2 h_prev); 0 at i = n, at order 1 and at i = 1)
    x' = k0 x + k1 D   (k0 = sigma_p/sigma_a, k1 = -alpha_p expm1(-h); at i = 1: k0 = 0, k1 = 1)
In float64 the chains use the float64 rows; in float32 the rows rounded to float32, every product and sum rounded: what the device does."""

from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from oracle import diffusion as D

from .ddim_ref import alpha_bar, gaussian_predictor  # noqa: F401  (the schedule the package holds; the exact predictor of N(0, std^2 I) data)

Q0, Q1, K0, K1, W, CLIP, SCALE = range(7)


def log_snr(abar: np.ndarray) -> np.ndarray:
    ab = np.asarray(abar, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 0.5 * (np.log(ab) - np.log1p(-ab))


def schedule(abar: np.ndarray, S: int, kind: str) -> List[int]:
    """the S (+1) timesteps of the chosen schedule before duplicates go: DDIM's two tables, or the timesteps nearest to S points
    uniform in lambda between t = T and t = 1"""
    T = len(abar) - 1
    if kind in ("linear", "quadratic"):
        return [int(v) for v in D.tau_table(T, S, kind)]
    assert kind == "logsnr", kind
    lam = log_snr(abar)
    pts = [lam[T]] if S == 1 else [lam[1] + (lam[T] - lam[1]) * j / (S - 1) for j in range(S)]
    return [1 + int(np.argmin(np.abs(lam[1:] - v))) for v in pts]


def grid(abar: np.ndarray, S: int, kind: str) -> List[int]:
    """0 followed by the strictly increasing subsequence of the schedule"""
    return [0] + sorted({t for t in schedule(abar, S, kind) if t > 0})


def rows(abar: np.ndarray, grid_: Sequence[int], order: int = 2, clip: bool = False, scale: float = 1.0) -> np.ndarray:
    """float64 [n+1][8]: (q0, q1, k0, k1, w, clip, s, 0) of the step from index i; row 0 is never stepped from"""
    ab, lam, n = np.asarray(abar, dtype=np.float64), log_snr(abar), len(grid_) - 1
    out = np.zeros((n + 1, 8), dtype=np.float64)
    out[:, CLIP], out[:, SCALE] = float(clip), scale
    out[0, :4] = (1.0, 0.0, 0.0, 1.0)
    for i in range(1, n + 1):
        a, p = ab[grid_[i]], ab[grid_[i - 1]]
        out[i, Q0], out[i, Q1] = 1.0 / np.sqrt(a), -np.sqrt(1 - a) / np.sqrt(a)
        if i == 1:
            out[i, K0], out[i, K1] = 0.0, 1.0
            continue
        h = lam[grid_[i - 1]] - lam[grid_[i]]
        out[i, K0], out[i, K1] = np.sqrt(1 - p) / np.sqrt(1 - a), -np.sqrt(p) * np.expm1(-h)
        if order == 2 and i < n:
            out[i, W] = h / (2.0 * (lam[grid_[i]] - lam[grid_[i + 1]]))
    return out


def _row(row, dtype):
    return [float(np.float32(v)) if dtype == torch.float32 else float(v) for v in row]


def step(x: Tensor, eps: Tensor, prev: Optional[Tensor], row, valid: bool, dtype=torch.float64):
    """(x', x0) in `dtype`, each product and sum rounded; `prev` is not touched unless `valid`"""
    r = _row(row, dtype)
    x, eps = x.to(dtype), eps.to(dtype)
    x0 = r[Q0] * x + r[Q1] * eps
    if r[CLIP] != 0.0:
        x0 = x0.clamp(-1.0, 1.0)
    d = x0 + r[W] * (x0 - prev.to(dtype)) if valid else x0
    return r[K0] * x + r[K1] * d, x0


def mix(e_c: Tensor, e_u: Tensor, s: float, dtype=torch.float64) -> Tensor:
    """e_u + s (e_c - e_u): three separately rounded operations; s as the fp32 tables carry it in a float32 chain"""
    s = float(np.float32(s)) if dtype == torch.float32 else float(s)
    return e_u.to(dtype) + s * (e_c.to(dtype) - e_u.to(dtype))


def decode(eps_model: Callable[[Tensor, Tensor], Tensor], x: Tensor, abar: np.ndarray, grid_: Sequence[int], order: int = 2, clip: bool = False,
           start: Optional[int] = None, dtype=torch.float64, keep: Iterable[int] = (), x0s: Optional[list] = None) -> Dict[int, Tensor]:
    """`start` steps from x = x_{tau_start}, the first of them first order.  Returns {i: the state after the step from index i} for i
    in `keep` and the final state under key 0; every x0 prediction is appended to `x0s` when given.  eps_model(x, t) -> the predicted
    noise (a guided chain passes a model that mixes)."""
    n = len(grid_) - 1
    start = n if start is None else start
    tab = rows(abar, grid_, order, clip)
    x = x.to(dtype)
    out, keep, prev = {}, set(keep), None
    for i in range(start, 0, -1):
        eps = eps_model(x, torch.tensor([grid_[i]]))
        x, prev = step(x, eps, prev, tab[i], prev is not None, dtype)
        if x0s is not None:
            x0s.append(prev)
        if i in keep:
            out[i] = x
    out[0] = x
    return out


def end_gain_error(abar: np.ndarray, grid_: Sequence[int], order: int, std: float = 0.5) -> float:
    """|gain of the chain x_T -> x_0 under the exact predictor of N(0, std^2 I) data  -  the probability-flow ODE's own gain|, float64.
    The ODE maps N(0, abar_T std^2 + 1 - abar_T) onto N(0, std^2) linearly."""
    T = grid_[-1]
    got = float(decode(gaussian_predictor(abar, std), torch.ones(1, dtype=torch.float64), abar, grid_, order)[0])
    return abs(got - std / np.sqrt(abar[T] * std * std + 1 - abar[T]))


def ddim_gain_error(abar: np.ndarray, grid_: Sequence[int], std: float = 0.5) -> float:
    """the same figure for the paper-form DDIM step (eta = 0) of tests/ddim_ref.py on the same grid"""
    from . import ddim_ref as R

    got = float(R.decode(gaussian_predictor(abar, std), torch.ones(1, dtype=torch.float64), abar, list(grid_), 0.0)[0])
    T = grid_[-1]
    return abs(got - std / np.sqrt(abar[T] * std * std + 1 - abar[T]))
