"""What the samplers that run only as whole device-resident chains share on the host (RePaint / SDEdit, ILVR, DDNM, DPS, the
probability-flow ODE): the argument checks, the rounding of float64 rows to the fp32 tables the device reads, the cached runner of a
table, the refusal of single steps, and for the four that walk the grid 0 = tau_0 < ... < tau_n = T, that grid.  A sampler adds its
table builder, its row's noise rule (chain.ROW_DRAWS), its runner's C call and its public methods."""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .chain import ChainRunner
from .ddpm import DDPM
from .dpm_solver import _from_process, solver_grid


def fp32_tables(rows, ttab):
    """(n, rows, t_table) as a chain takes them, from a table builder's float64 rows [n + 1][8] and timesteps [n + 1]: every scalar
    rounded to fp32 once, here"""
    return len(ttab) - 1, [tuple(float(np.float32(v)) for v in r) for r in rows], ttab


def check_mask(mask, shape, device, none_value: float, binary: bool = True, channels: str = "C", why: str = "") -> Tensor:
    """(B|1, C|1, h, w) -> contiguous fp32 of `shape`; None: `none_value` everywhere.  `binary`: a measurement's mask, values 0 or 1
    (`channels`: what the message calls its channel count, `why`: what it adds on a fractional value); else values in [0, 1] at image
    resolution (RePaint's: 1 = known pixel)"""
    if mask is None:
        return torch.full(tuple(shape), none_value, dtype=torch.float32, device=device)
    m = torch.as_tensor(mask).detach().to(device=device, dtype=torch.float32)
    B, Cc, h, w = shape
    if m.dim() != 4 or m.shape[0] not in (1, B) or m.shape[1] not in (1, Cc) or tuple(m.shape[2:]) != (h, w):
        dims = f"(B|1, {channels}|1, h, w) to the measurement's" if binary else "(B|1, C|1, H, W) to"
        raise ValueError(f"mask: shape {tuple(m.shape)} does not broadcast from {dims} {tuple(shape)}")
    if not bool(((m == 0) | (m == 1)).all() if binary else ((m >= 0) & (m <= 1)).all()):
        raise ValueError(f"mask: values must be 0 or 1 (1: measured){why}" if binary else "mask: values must lie in [0, 1] (1: known pixel, 0: generate)")
    return m.expand(B, Cc, h, w).contiguous()


class WholeChainProcess(DDPM):
    """a process over DDPM's network and schedule that runs whole chains only"""

    _whole_chains = ""  # the refusal of a single step: what the class runs instead
    _image_noun = "batch"

    from_process = classmethod(_from_process)

    def _chain_tables(self):
        n, rows, ttab = self._tables
        return n, list(rows), list(ttab)

    def _image(self, x: Tensor, what: str, copy: bool = False) -> Tensor:
        """a floating-point (B, C, H, W) argument as contiguous fp32 on the process's device (`copy`: never the caller's tensor)"""
        if not (isinstance(x, Tensor) and x.dim() == 4 and x.is_floating_point()):
            raise ValueError(f"{what}: a floating-point {self._image_noun} (B, C, H, W)")
        x = x.detach().to(device=self.beta.device, dtype=torch.float32).contiguous()
        return x.clone() if copy else x

    def _table_runner(self, slot: str, shape, dev, tables=None) -> Optional[ChainRunner]:
        """the cached runner in `slot`: over the process's own tables on the shared buffer, or over `tables` on a buffer of its own"""
        if tables is None:
            return self._buffered_runner(slot, shape, dev)
        return self._buffered_runner(slot, shape, dev, spec=lambda: (self._chain_kind, tables), buf=slot + "_buf")

    def sampling_step(self, *a, **kw):
        raise NotImplementedError(self._whole_chains)

    denoise_once = sampling_step


class GridProcess(WholeChainProcess):
    """... whose levels are the grid 0 = tau_0 < tau_1 < ... < tau_n = T of `solver_grid(alpha_bar, sub_timesteps, "linear")`; level k is
    a sample at noise level tau_k, level 0 a clean image"""

    def _set_grid(self, sub_timesteps: int, alpha_bar=None) -> None:
        """the tail of a constructor: `sub_timesteps` checked, `alpha_bar` (a (T+1) table in place of the linear schedule's) taken, then
        `n_levels`, the `tau` buffer, its host copy `_tau_host` and the float64 `_ab64` the table builders read"""
        if isinstance(sub_timesteps, bool) or int(sub_timesteps) != sub_timesteps or not 1 <= sub_timesteps <= self.timesteps:
            raise ValueError(f"sub_timesteps = {sub_timesteps!r} outside 1..{self.timesteps}")
        if alpha_bar is not None:
            self._use_alpha_bar(alpha_bar)
        self.sub_timesteps = int(sub_timesteps)
        self._ab64 = self.alpha_bar.reshape(-1).to(torch.float64).cpu().numpy()
        self._tau_host = solver_grid(self._ab64, self.sub_timesteps, "linear")
        self.n_levels = len(self._tau_host) - 1
        self.register_buffer("tau", torch.tensor(self._tau_host, dtype=torch.int64), persistent=False)
