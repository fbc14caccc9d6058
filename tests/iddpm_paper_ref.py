"""CPU restatement, in float64 numpy, of what the package adds to Improved DDPM beyond the reference project (Nichol & Dhariwal 2021):
the strided sampling chain with the learned variance (section 4), the loss-second-moment timestep resampler (section 3.3) and the
prior term of the variational bound.  The reference project has none of the three, so this file is the yardstick, as
tests/ddim_ref.py is for the paper-form DDIM sampler.  The per-image loss rows themselves are held against oracle/iddpm.py.

Strided chain over s_1 < ... < s_K (s_0 = 0, abar_{s_0} = 1):
  s_k = 1 + round((k-1)(T-1)/(K-1)), Python's round (half to even)
  beta'_k = min(1 - abar_{s_k}/abar_{s_{k-1}}, 0.999),   beta~'_k = beta'_k (1 - abar_{s_{k-1}})/(1 - abar_{s_k})
  row k = (1/sqrt(1 - beta'_k), beta'_k/sqrt(1 - abar_{s_k}), log beta'_k, log max(beta~'_k, 1e-12))
  x' = row0 (x - row1 eps) + sqrt(exp(v row2 + (1 - v) row3)) z, the noise left out on the step from s_1 = 1
Resampler with a history of H losses per timestep, warm iff every timestep 1..T has H of them:
  p_t = 1/T while not warm, else (1 - u0) s_t / sum(s) + u0 / T with s_t = sqrt(mean_k hist[t][k]^2)
  t_b = 1 + #{t : cdf_t <= u_b cdf_T} (cdf: inclusive prefix sum of p), weight_b = 1/(T p[t_b])
  push (t, L): append while the row has room, otherwise drop the oldest; entries with t outside 1..T or a non-finite L are skipped"""

from __future__ import annotations

from typing import List, Sequence

import numpy as np


def space_timesteps(T: int, K: int) -> List[int]:
    if not 2 <= K <= T:
        raise ValueError((T, K))
    return [1 + round((k - 1) * (T - 1) / (K - 1)) for k in range(1, K + 1)]


def respaced_rows(abar: np.ndarray, steps: Sequence[int]) -> np.ndarray:
    """float64 [K+1][4]; row 0 is zero (never stepped from).  abar: float64[T+1], index = timestep"""
    abar = np.asarray(abar, dtype=np.float64).reshape(-1)
    rows = np.zeros((len(steps) + 1, 4), dtype=np.float64)
    prev = 1.0
    for k, s in enumerate(steps, start=1):
        cur = abar[s]
        beta = min(1.0 - cur / prev, 0.999)
        beta_tilde = beta * (1.0 - prev) / (1.0 - cur)
        rows[k] = (1.0 / np.sqrt(1.0 - beta), beta / np.sqrt(1.0 - cur), np.log(beta), np.log(max(beta_tilde, 1e-12)))
        prev = cur
    return rows


def respaced_betas(abar: np.ndarray, steps: Sequence[int]) -> np.ndarray:
    """float64 [K]: beta'_k without the clip"""
    a = np.asarray(abar, dtype=np.float64).reshape(-1)[list(steps)]
    return 1.0 - a / np.concatenate([[1.0], a[:-1]])


def chain_step(x: np.ndarray, model_out: np.ndarray, z: np.ndarray, row: Sequence[float], add_noise: bool) -> np.ndarray:
    """one update in float64; x, z: (B, C, H, W), model_out: (B, 2C, H, W) = (eps, v)"""
    x, z, out = (np.asarray(v, dtype=np.float64) for v in (x, z, model_out))
    C = x.shape[1]
    eps, v = out[:, :C], out[:, C:]
    mean = row[0] * (x - row[1] * eps)
    if not add_noise:
        return mean
    return mean + np.sqrt(np.exp(v * row[2] + (1.0 - v) * row[3])) * z


def prior_rows(x0: np.ndarray, abar_T: float) -> np.ndarray:
    """KL(q(x_T | x_0) || N(0, I)) per image, nats/dim: mean of 0.5 (-log(1 - a) - 1 + (1 - a) + a x_0^2); the constant part is
    written -log1p(-a) - a, the same number without the cancellation against 1"""
    a = float(abar_T)
    x = np.asarray(x0, dtype=np.float64).reshape(len(x0), -1)
    return (0.5 * ((-np.log1p(-a) - a) + a * x * x)).mean(axis=1)


def probabilities(hist: np.ndarray, count: np.ndarray, T: int, H: int, u0: float):
    """(warm, float64 p[T+1]) with p[0] = 0"""
    warm = bool(np.all(np.asarray(count)[1 : T + 1] == H))
    p = np.zeros(T + 1, dtype=np.float64)
    if not warm:
        p[1:] = 1.0 / T
        return warm, p
    s = np.sqrt(np.mean(np.asarray(hist, dtype=np.float64)[1 : T + 1, :H] ** 2, axis=1))
    p[1:] = (1.0 - u0) * s / s.sum() + u0 / T
    return warm, p


def bin_violations(p32: np.ndarray, u: np.ndarray, t: np.ndarray, T: int) -> np.ndarray:
    """indices of the draws that are not in the bin of their uniform.  cdf64: float64 prefix sums of the kernel's own fp32 p; draw b
    must satisfy cdf64[t_b - 1] - m <= u_b cdf64[T] <= cdf64[t_b] + m with m = (T + 2) 2^-24 cdf64[T], the worst-case error of an fp32
    prefix sum of T terms in any order plus the rounding of the product."""
    cdf = np.concatenate([[0.0], np.cumsum(np.asarray(p32, dtype=np.float64)[1 : T + 1])])
    m = (T + 2) * 2.0**-24 * cdf[T]
    x = np.asarray(u, dtype=np.float64) * cdf[T]
    t = np.asarray(t, dtype=np.int64)
    ok = (cdf[t - 1] - m <= x) & (x <= cdf[t] + m)
    return np.nonzero(~ok)[0]


def push(hist: np.ndarray, count: np.ndarray, t: Sequence[int], L: Sequence[float], T: int, H: int) -> int:
    """the batch pushed in index order, in place (hist: float32[T+1][H], count: int32[T+1]); returns the status flag"""
    status = 0
    for tb, v in zip(np.asarray(t).tolist(), np.asarray(L, dtype=np.float32)):
        if tb < 1 or tb > T or not np.isfinite(v):
            status = 1
            continue
        if count[tb] < H:
            hist[tb, count[tb]] = v
            count[tb] += 1
        else:
            hist[tb, :-1] = hist[tb, 1:].copy()
            hist[tb, H - 1] = v
    return status
