"""Host-side tables of Improved DDPM (tiny, computed once on the CPU in fp32 with the same torch ops
as the reference; the per-pixel math runs in the HIP kernels dmme_iddpm_step / dmme_iddpm_loss)."""

from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np
import torch
from torch import Tensor


def cosine_schedule(timesteps: int = 4000, offset: float = 0.008) -> Tensor:
    r"""alpha_bar_t = f(t)/f(0), f(t) = cos^2((t/T + s)/(1 + s) * pi/2), t = 0..T
    (reference: equations/iddpm/iddpm.py:6-20)."""

    def f(t):
        return torch.cos((t / timesteps + offset) / (1 + offset) * math.pi / 2) ** 2

    t = torch.arange(0, timesteps + 1)
    zero = torch.tensor([0], dtype=torch.float32)
    return f(t) / f(zero)


def interpolate_variance(v: Tensor, beta_t: Tensor, beta_tilde_t: Tensor) -> Tensor:
    r"""Sigma = exp(v log beta_t + (1 - v) log beta~_t) (reference: equations/iddpm/losses.py:34-37).
    Host/torch form kept for API parity; the sampler and loss kernels evaluate it per pixel."""
    return torch.exp(v * torch.log(beta_t) + (1 - v) * torch.log(beta_tilde_t.clamp(1e-12)))


def process_coefficients(beta: Tensor, alpha: Tensor, alpha_bar: Tensor) -> Tensor:
    """(T+1, 8) fp32 table consumed by dmme_iddpm_step / dmme_iddpm_loss (layout in include/dmme_hip.h), evaluated
    with the reference's fp32 torch expressions: reverse_process (equations/ddpm/ddpm.py:65-71), beta~
    (diffusion_models/iddpm.py:161), interpolate_variance's logs (equations/iddpm/losses.py:34-37) and
    true_reverse_process (equations/iddpm/losses.py:23-31).  Row 0 (t = 0 is never used) is zero."""
    b, a, ab = (v.reshape(-1).to(torch.float32).cpu() for v in (beta, alpha, alpha_bar))
    T1 = b.numel()
    tab = torch.zeros(T1, 8, dtype=torch.float32)
    bt, at, abt, abp = b[1:], a[1:], ab[1:], ab[:-1]
    beta_tilde = (1 - abp) / (1 - abt) * bt
    tab[1:, 0] = 1 / torch.sqrt(at)
    tab[1:, 1] = bt / torch.sqrt(1 - abt)
    tab[1:, 2] = torch.log(bt)
    tab[1:, 3] = torch.log(beta_tilde.clamp(1e-12))
    tab[1:, 4] = torch.sqrt(abp) * bt / (1 - abt)
    tab[1:, 5] = torch.sqrt(at) * (1 - abp) / (1 - abt)
    tab[1:, 6] = torch.sqrt(beta_tilde)
    return tab


def space_timesteps(timesteps: int, sample_steps: int) -> List[int]:
    r"""the K timesteps of a strided sampling chain (Nichol & Dhariwal 2021, section 4), evenly spaced over 1..T with both ends kept:
    s_k = 1 + round((k - 1)(T - 1)/(K - 1)), k = 1..K, with Python's round (half to even, as in the paper's code).  s_1 = 1, s_K = T."""
    T, K = int(timesteps), int(sample_steps)
    if not 2 <= K <= T:
        raise ValueError(f"sample_steps = {sample_steps} must lie in [2, timesteps = {timesteps}]")
    return [1 + round((k - 1) * (T - 1) / (K - 1)) for k in range(1, K + 1)]


def respaced_coefficients(alpha_bar: Tensor, steps: Sequence[int]) -> Tensor:
    r"""(K+1, 4) fp32 rows of the DMME_CHAIN_IDDPM update for the chain that visits only `steps` = s_1 < ... < s_K; row k is the step
    s_k -> s_{k-1} (s_0 = 0, abar_{s_0} = 1) and row 0 is zero (never stepped from).  In float64 from the registered alpha_bar:
      beta'_k = min(1 - abar_{s_k}/abar_{s_{k-1}}, 0.999)   (the constructor's clip)
      beta~'_k = beta'_k (1 - abar_{s_{k-1}})/(1 - abar_{s_k})
      row k = {1/sqrt(1 - beta'_k), beta'_k/sqrt(1 - abar_{s_k}), log beta'_k, log max(beta~'_k, 1e-12)}, each rounded once to fp32."""
    ab = alpha_bar.detach().reshape(-1).to(torch.float64).cpu().numpy()
    s = [int(v) for v in steps]
    if not s or s[0] < 1 or s[-1] >= ab.size or any(b <= a for a, b in zip(s, s[1:])):
        raise ValueError("steps must be strictly increasing timesteps inside 1..T")
    cur, prev = ab[s], np.concatenate([[1.0], ab[s[:-1]]])
    beta = np.minimum(1.0 - cur / prev, 0.999)
    beta_tilde = beta * (1.0 - prev) / (1.0 - cur)
    rows = np.zeros((len(s) + 1, 4), dtype=np.float64)
    rows[1:, 0] = 1.0 / np.sqrt(1.0 - beta)
    rows[1:, 1] = beta / np.sqrt(1.0 - cur)
    rows[1:, 2] = np.log(beta)
    rows[1:, 3] = np.log(np.maximum(beta_tilde, 1e-12))
    return torch.from_numpy(rows.astype(np.float32))
