"""DPM-Solver++(2M) (Lu, Zhou, Bao, Chen, Li & Zhu 2022): the second-order multistep solver of the diffusion ODE in data-prediction form.

One network call per step, like DDIM, but the update extrapolates with the previous step's x0 prediction:

    alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = log(alpha_t / sigma_t); step a = tau_i -> p = tau_{i-1}, h = lambda_p - lambda_a
    x0 = (x - sigma_a eps) / alpha_a                        (clamped to [-1, 1] with clip_x0)
    D  = x0 + h / (2 h_prev) (x0 - x0_prev)                 (D = x0 on a chain's first step, at order 1, and on the last step)
    x' = sigma_p / sigma_a x - alpha_p expm1(-h) D

The host folds the scalars per index in float64 and rounds them to fp32 (include/dmme_hip.h: dmme_dpmpp_step); the device keeps x0_prev
in a buffer of the runner and a "history valid" flag in the loop state, so one captured step serves every step of every chain."""

from __future__ import annotations

from typing import List, Optional, Tuple

import ctypes as C

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian
from ..equations.ddim import linear_tau, quadratic_tau
from .ddim import DDIM
from .chain import ChainRunner, walk
from .ddpm import DDPM, _scalar_index

TAU_SCHEDULES = ("linear", "quadratic", "logsnr")
ROW = 8  # floats per table row: q0, q1, k0, k1, w, clip, s, -


def log_snr(alpha_bar: np.ndarray) -> np.ndarray:
    """lambda_t = log(alpha_t / sigma_t) in float64 (+inf at abar = 1)"""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 0.5 * (np.log(ab) - np.log1p(-ab))


def logsnr_tau(alpha_bar: np.ndarray, sub_timesteps: int) -> List[int]:
    """the integer timesteps nearest to `sub_timesteps` points uniform in lambda between t = T and t = 1 (ascending; may repeat)"""
    lam = log_snr(alpha_bar)
    T = len(lam) - 1
    pts = [lam[T]] if sub_timesteps == 1 else [lam[1] + (lam[T] - lam[1]) * j / (sub_timesteps - 1) for j in range(sub_timesteps)]
    return [1 + int(np.argmin(np.abs(lam[1:] - v))) for v in pts]


def solver_grid(alpha_bar: np.ndarray, sub_timesteps: int, tau_schedule: str) -> List[int]:
    """0 = tau_0 < tau_1 < ... < tau_n = T: the strictly increasing subsequence of the chosen schedule (a repeated timestep would make h = 0)"""
    T = len(alpha_bar) - 1
    if tau_schedule == "linear":
        ts = [int(v) for v in linear_tau(T, sub_timesteps)]
    elif tau_schedule == "quadratic":
        ts = [int(v) for v in quadratic_tau(T, sub_timesteps)]
    elif tau_schedule == "logsnr":
        ts = logsnr_tau(alpha_bar, sub_timesteps)
    else:
        raise ValueError(f"tau_schedule = {tau_schedule!r}; use one of {TAU_SCHEDULES}")
    return [0] + sorted({t for t in ts if t > 0})


def solver_rows(alpha_bar: np.ndarray, grid, order: int = 2, clip_x0: bool = False, scale: float = 1.0) -> np.ndarray:
    """float64 [n+1][8]: {q0, q1, k0, k1, w, clip, s, 0} of the step from loop index i; row 0 (never stepped from) returns x0 = x"""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    lam = log_snr(ab)
    n = len(grid) - 1
    rows = np.zeros((n + 1, ROW), dtype=np.float64)
    rows[:, 5], rows[:, 6] = float(bool(clip_x0)), scale
    rows[0, :4] = (1.0, 0.0, 0.0, 1.0)
    for i in range(1, n + 1):
        a, p = ab[grid[i]], ab[grid[i - 1]]
        rows[i, 0], rows[i, 1] = 1.0 / np.sqrt(a), -np.sqrt(1 - a) / np.sqrt(a)
        if i == 1:  # p = 0: sigma_p = 0, h = inf - the chain ends on x0
            rows[i, 2:5] = (0.0, 1.0, 0.0)
            continue
        h = lam[grid[i - 1]] - lam[grid[i]]
        rows[i, 2], rows[i, 3] = np.sqrt((1 - p) / (1 - a)), -np.sqrt(p) * np.expm1(-h)
        if order == 2 and i < n:
            rows[i, 4] = h / (2.0 * (lam[grid[i]] - lam[grid[i + 1]]))
    return rows


class DPMChainRunner(ChainRunner):
    """ChainRunner whose captured step is dmme_dpmpp_chain_step: tables of 8 floats per index and `hist`, the previous step's x0 prediction,
    a fixed buffer that travels with x and the loop state (whose flag says whether it is valid)"""

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        super().__init__(process, x, use_graph, spec)
        self.hist = torch.empty_like(x)

    def _carried(self):
        return super()._carried() + [self.hist]

    def _call(self, packed):
        _lib.check(
            _lib.lib().dmme_dpmpp_chain_step(self.plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.plan.workspace), _lib.ptr(self.hist),
                                             _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state), _lib.stream_ptr()),
            "dmme_dpmpp_chain_step",
        )


def _row_arg(row):
    """a table row of ROW floats as the C array the eager entry points take (every kind whose rows are 8 floats)"""
    return (C.c_float * ROW)(*row)


def _from_process(cls, p: DDPM, **kw):
    """the sampler over `p`'s network, noise schedule (an IDDPM's cosine schedule, for one), prediction and x0 thresholding"""
    kw.setdefault("prediction", getattr(p, "prediction", "eps"))
    kw.setdefault("threshold", getattr(p, "threshold", "none"))
    kw.setdefault("threshold_percentile", getattr(p, "threshold_percentile", 0.995))
    return cls(p.model, p.timesteps, alpha_bar=p.alpha_bar.detach().reshape(-1).cpu(), **kw)


class DPMSolverPP(DDIM):
    r"""DPM-Solver++(2M) over any noise-prediction network of the package (an IDDPM network's learned variance is not used), or an x0 / v
    network (`prediction=`: its output becomes an eps prediction behind the forward, from which the rows form the solver's x0).

    `tau_schedule`: "linear" / "quadratic" (DDIM's) or "logsnr" (the integer timesteps nearest to `sub_timesteps` points uniform in
    lambda between t = T and t = 1).  The solver's grid is the strictly increasing subsequence of that schedule: `n_steps` may be below
    `sub_timesteps`.  `order` 1 is DDIM at eta = 0 in data-prediction form.  `alpha_bar`: a (T+1) table in place of the linear
    schedule's (`from_process` takes it from a DDPM / IDDPM instance)."""

    _chain_kind = _lib.CHAIN_DPMPP
    _runner_class = DPMChainRunner

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 20, tau_schedule: str = "logsnr", order: int = 2, clip_x0: bool = False,
                 alpha_bar: Optional[Tensor] = None, *, prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        DDPM.__init__(self, model, timesteps, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)  # (DDIM's constructor knows two schedules and the linear beta only)
        kind = str(tau_schedule).lower()
        if kind not in TAU_SCHEDULES:
            raise ValueError(f"tau_schedule = {tau_schedule!r}; use one of {TAU_SCHEDULES}")
        if order not in (1, 2):
            raise ValueError(f"order = {order!r}; DPM-Solver++(2M) runs at order 1 or 2")
        if int(sub_timesteps) != sub_timesteps or not 1 <= sub_timesteps <= timesteps:
            raise ValueError(f"sub_timesteps = {sub_timesteps!r} outside 1..{timesteps}")
        if alpha_bar is not None:
            self._use_alpha_bar(alpha_bar)
        self.sub_timesteps, self.tau_schedule, self.order, self.clip_x0 = int(sub_timesteps), kind, int(order), bool(clip_x0)
        ab64 = self.alpha_bar.reshape(-1).to(torch.float64).cpu().numpy()
        grid = solver_grid(ab64, self.sub_timesteps, kind)
        self.n_steps = len(grid) - 1
        self.register_buffer("tau", torch.tensor(grid, dtype=torch.int64), persistent=False)
        self._tau_host = grid
        self._tau_dev: Optional[Tensor] = None
        self._ab64 = ab64
        self._s1, self._s2 = np.sqrt(1 - ab64).tolist(), np.sqrt(ab64).tolist()  # what DDIM's constructor leaves for its collapsed update
        self._rows = self._make_rows(1.0)

    from_process = classmethod(_from_process)

    def _make_rows(self, scale: float):
        rows = solver_rows(self._ab64, self._tau_host, self.order, self.clip_x0, scale)
        return [tuple(float(np.float32(v)) for v in r) for r in rows]

    def _chain_tables(self):
        return self.n_steps, list(self._rows), list(self._tau_host)

    def _last_index(self) -> int:
        return self.n_steps

    def _eps_planes(self, x: Tensor, eps: Tensor) -> int:
        planes = eps[0].numel() // x[0].numel()
        if eps.shape[0] != x.shape[0] or planes * x[0].numel() != eps[0].numel() or planes not in (1, 2):
            raise ValueError(f"a network output of shape {tuple(eps.shape)} for images of shape {tuple(x.shape)}")
        return planes

    def _dpm_update(self, x: Tensor, eps: Tensor, i: int, hist: Tensor, valid: bool) -> Tensor:
        """the eager twin of the chain kind, in place on x and hist"""
        eps = eps.detach().to(torch.float32).contiguous()
        _lib.check(_lib.lib().dmme_dpmpp_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(hist), _row_arg(self._rows[i]), int(valid), x.shape[0], x[0].numel(),
                                              self._eps_planes(x, eps), _lib.stream_ptr()), "dmme_dpmpp_step")
        return x

    @staticmethod
    def _history(x: Tensor, history: Optional[Tensor]) -> Tensor:
        if history is None:
            return torch.empty_like(x)
        if not (history.shape == x.shape and history.dtype == torch.float32 and history.device == x.device and history.is_contiguous()):
            raise ValueError("history: a contiguous fp32 tensor of x's shape on x's device")
        return history

    @staticmethod
    def _history_valid(history: Optional[Tensor], history_valid: bool) -> bool:
        if history_valid and history is None:
            raise ValueError("history_valid=True needs the history tensor")
        return bool(history_valid)

    def sampling_step(self, x_tau_i: Tensor, i: Tensor, history: Optional[Tensor] = None, history_valid: bool = False) -> Tensor:
        r"""x_{tau_{i-1}} from x_{tau_i}; i has shape (1,).  `history` (optional) receives this step's x0 prediction in place.  The step
        reads it - a second-order step - only where the caller says `history_valid=True`: it then holds the x0 prediction of the step
        from index i + 1 of the same chain.  A host loop passes `history_valid=False` on its first step, wherever it starts."""
        idx = self._index(_scalar_index(i, "an index"), "sampling_step")
        valid = self._history_valid(history, history_valid)
        x = x_tau_i.detach().to(torch.float32).contiguous().clone()
        with torch.no_grad():
            eps = self._eps(x, self.tau[idx].reshape(1))
        return self._dpm_update(x, eps, idx, self._history(x, history), valid)

    def denoise_once(self, x: Tensor, i: int) -> Tensor:
        """one first-order step from loop index i as a new tensor (no history travels between calls: chains run through `decode`)"""
        i = self._index(i, "denoise_once")
        done = self._once_via_runner(x, i)
        if done is not None:
            return done
        out = x.detach().to(torch.float32).contiguous().clone()
        with torch.no_grad():
            eps = self._eps(out, self.tau_tensor(i, out.device))
        return self._dpm_update(out, eps, i, torch.empty_like(out), False)

    def _eager_chain(self, x: Tensor, start: int, recorder=None) -> Tensor:
        """the host loop, bit-identical to the captured chain: the same update on the same scalars, the history valid after the first step"""
        hist = torch.empty_like(x)
        return walk(x, start, start, lambda k, i: self._dpm_update(x, self._eps(x, self.tau_tensor(i, x.device)), i, hist, k > 0), recorder)

    def _decode_chain(self, x: Tensor, start: int, recorder=None) -> Tensor:
        runner = self._buffered_runner("_runner", x.shape, x.device)
        if runner is None:
            return self._eager_chain(x, start, recorder)
        runner.x.copy_(x)
        return runner.run(start, start, recorder).clone()

    @torch.no_grad()
    def decode(self, x: Tensor, start: Optional[int] = None, history=None) -> Tensor:
        r"""x_0 from x_{tau_start} (start = n_steps by default): `start` solver steps, the first of them first order.  `history`: a
        HistoryRecorder for the chain's frames (not the x0 history of `sampling_step`)"""
        return self._decode(x, start, history)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """the n_steps chain from pure noise; nothing but x_T is drawn.  `history`: a HistoryRecorder for the chain's frames"""
        return self.decode(gaussian(img_size, device=self.beta.device), history=history)
