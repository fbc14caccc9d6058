"""CPU restatement of the paper-form DDIM sampler (dmme_amd.GeneralizedDDIM; Song, Meng & Ermon 2021, eq. 12) in float64 or float32:
the coefficient tables, the reverse and the encoding step, whole chains over any `eps_model`, and the spherical interpolation of
latents.  The reference project ships only the collapsed update (oracle.diffusion.ddim_step), so there is nothing of its own to
compare against: this file is the yardstick, as tests/classifier_ref.py is for classifier guidance.

Every step, in either direction, is  x' = (k0 x + k1 eps) + k2 z.
  reverse, a = abar[tau_i] -> p = abar[tau_{i-1}]:  sigma = eta sqrt((1-p)/(1-a)) sqrt(1 - a/p)  (0 where p == 1 or a == 1)
                                                    k0 = sqrt(p/a), k1 = sqrt(max(1 - p - sigma^2, 0)) - k0 sqrt(1-a), k2 = sigma
  encode,  a = abar[tau_i] -> n = abar[tau_{i+1}]:  k0 = sqrt(n/a), k1 = sqrt(1-n) - k0 sqrt(1-a), k2 = 0; network at max(tau_i, 1)
In float64 the chains use the float64 coefficients; in float32 they use those coefficients rounded to float32 and round every
product and sum, which is what the device does."""

from __future__ import annotations

from typing import Callable, Dict, Iterable, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from oracle import diffusion as D


def alpha_bar(timesteps: int) -> np.ndarray:
    """the schedule the package holds (fp32 cumprod of the reference's linear beta), widened to float64; index = timestep"""
    return D.alpha_tables(D.linear_beta(timesteps))[1].to(torch.float64).numpy()


def tau(timesteps: int, sub_timesteps: int, schedule: str = "quadratic"):
    return [int(v) for v in D.tau_table(timesteps, sub_timesteps, schedule)]


def reverse_rows(abar: np.ndarray, tau_: Sequence[int], eta: float) -> np.ndarray:
    """float64 [S+1][3]: (k0, k1, k2 = sigma) of the step tau_i -> tau_{i-1}; row 0 is the identity (never stepped from)"""
    S = len(tau_) - 1
    rows = np.zeros((S + 1, 3), dtype=np.float64)
    rows[0] = (1.0, 0.0, 0.0)
    for i in range(1, S + 1):
        a, p = abar[tau_[i]], abar[tau_[i - 1]]
        sigma = 0.0 if (p == 1.0 or a == 1.0) else eta * np.sqrt((1 - p) / (1 - a)) * np.sqrt(1 - a / p)
        k0 = np.sqrt(p / a)
        rows[i] = (k0, np.sqrt(max(1 - p - sigma * sigma, 0.0)) - k0 * np.sqrt(1 - a), sigma)
    return rows


def encode_rows(abar: np.ndarray, tau_: Sequence[int]):
    """float64 [S][3] and the timesteps the network sees: entry i is the step tau_i -> tau_{i+1}, i = 0 .. S-1"""
    S = len(tau_) - 1
    rows = np.zeros((S, 3), dtype=np.float64)
    for i in range(S):
        a, n = abar[tau_[i]], abar[tau_[i + 1]]
        k0 = np.sqrt(n / a)
        rows[i] = (k0, np.sqrt(1 - n) - k0 * np.sqrt(1 - a), 0.0)
    return rows, [max(tau_[i], 1) for i in range(S)]


def _row(row, dtype):
    """the three scalars as python floats: rounded to float32 for a float32 chain (the device's tables), untouched in float64"""
    return [float(np.float32(v)) if dtype == torch.float32 else float(v) for v in row]


def step(x: Tensor, eps: Tensor, z: Optional[Tensor], row, dtype=torch.float64) -> Tensor:
    """(k0 x + k1 eps) + k2 z in `dtype`, each product and sum rounded; z is used only where k2 != 0"""
    k0, k1, k2 = _row(row, dtype)
    m = k0 * x.to(dtype) + k1 * eps.to(dtype)
    return m + k2 * z.to(dtype) if k2 != 0.0 else m


reverse_step = step
encode_step = step


def decode(eps_model: Callable[[Tensor, Tensor], Tensor], x: Tensor, abar: np.ndarray, tau_: Sequence[int], eta: float = 0.0,
           noises: Optional[Dict[int, Tensor]] = None, start: Optional[int] = None, dtype=torch.float64, keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    """`start` reverse steps from x = x_{tau_start}; noises[i] is the z of the step from index i.  Returns {i: the state after the
    step from index i} for i in `keep`, and the final state under key 0."""
    S = len(tau_) - 1
    start = S if start is None else start
    rows = reverse_rows(abar, tau_, eta)
    x = x.to(dtype)
    out, keep = {}, set(keep)
    for i in range(start, 0, -1):
        eps = eps_model(x, torch.tensor([tau_[i]]))
        x = step(x, eps, None if noises is None else noises.get(i), rows[i], dtype)
        if i in keep:
            out[i] = x
    out[0] = x
    return out


generate = decode


def encode(eps_model: Callable[[Tensor, Tensor], Tensor], x0: Tensor, abar: np.ndarray, tau_: Sequence[int], upto: Optional[int] = None,
           dtype=torch.float64, keep: Iterable[int] = ()) -> Dict[int, Tensor]:
    """`upto` encoding steps from x_0.  Returns {i: x_{tau_i}} for i in `keep`, and the final state x_{tau_upto} under key -1."""
    S = len(tau_) - 1
    upto = S if upto is None else upto
    rows, ts = encode_rows(abar, tau_)
    x = x0.to(dtype)
    out, keep = {}, set(keep)
    for i in range(upto):
        eps = eps_model(x, torch.tensor([ts[i]]))
        x = step(x, eps, None, rows[i], dtype)
        if i + 1 in keep:
            out[i + 1] = x
    out[-1] = x
    return out


def slerp(xa: np.ndarray, xb: np.ndarray, w: Sequence[float], dtype=np.float64) -> np.ndarray:
    """xa, xb: (B, ...) -> (n, B, ...), every operation in `dtype`; the linear form where sin(theta) < 1e-6"""
    a = np.asarray(xa, dtype=dtype).reshape(len(xa), -1)
    b = np.asarray(xb, dtype=dtype).reshape(len(xb), -1)
    w = np.asarray(w, dtype=dtype)
    one = dtype(1.0)
    out = np.empty((len(w),) + a.shape, dtype=dtype)
    for k in range(a.shape[0]):
        c = np.dot(a[k], b[k]) / (np.sqrt(np.dot(a[k], a[k])) * np.sqrt(np.dot(b[k], b[k])))
        theta = np.arccos(np.clip(c, -one, one))
        sn = np.sin(theta)
        for j, wj in enumerate(w):
            if sn < 1e-6:
                fa, fb = one - wj, wj
            else:
                fa, fb = np.sin((one - wj) * theta) / sn, np.sin(wj * theta) / sn
            out[j, k] = dtype(fa) * a[k] + dtype(fb) * b[k]
    return out.reshape((len(w),) + np.asarray(xa).shape)


def gaussian_predictor(abar: np.ndarray, std: float = 0.5) -> Callable[[Tensor, Tensor], Tensor]:
    """the exact noise predictor for data ~ N(0, std^2 I): eps*(x, t) = sqrt(1 - abar_t) x / (abar_t std^2 + 1 - abar_t)"""
    def eps_model(x: Tensor, t: Tensor) -> Tensor:
        a = float(abar[int(t.reshape(-1)[0])])
        return (np.sqrt(1 - a) / (a * std * std + 1 - a)) * x
    return eps_model
