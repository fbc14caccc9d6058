"""Progressive distillation (Salimans & Ho, ICLR 2022, Algorithm 2) over the HIP kernels: a student that samples in N steps is trained
on what its frozen teacher does in 2N.  The reference project has no such method.

The grids are the ones `GeneralizedDDIM(..., tau_schedule="linear")` uses: tau = linear_tau(T, 2N), and the student's own grid
linear_tau(T, N)[i] == tau[2i].  Student index i in 1..N stands for t = tau[2i], m = tau[2i-1], e = tau[2i-2].  Per image:

    z_t = alpha_t x0 + sigma_t eps                                  (dmme_distill_noise: dmme_q_sample's bits)
    x1  = the teacher's x0 estimate at (z_t, t)
    z_m = alpha_m x1 + (sigma_m / sigma_t)(z_t - alpha_t x1)          (dmme_distill_mid)
    x2  = the teacher's x0 estimate at (z_m, m)
    x~  = w1 x1 + w2 x2,  w1 = (s_m - s_t) / (s_e - s_t),  w2 = (s_e - s_m) / (s_e - s_t),  s = alpha / sigma
    target = the student's parameterisation of x~ at (z_t, t)        (dmme_distill_target)

x~ is the image for which ONE DDIM step from z_t lands where the teacher's two steps do; the paper states it as the quotient
(z_e - r z_t) / (alpha_e - r alpha_t), r = sigma_e / sigma_t, which subtracts nearly equal numbers.  Substituting the two steps gives the
convex combination above (both weights positive, sum 1, (0, 1) where e = 0); z_e is never formed.  The weights and every other scalar are
folded on the host in float64 and rounded once (include/dmme_hip.h: dmme_distill_*)."""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian_like, uniform_int
from ..equations.ddim import linear_tau
from .ddim import GeneralizedDDIM
from .ddpm import DDPM

ROW = 12  # floats per table row: p0 p1 | p0' p1' | m0 m1 | w1 w2 | q0 q1 | two spare


def distill_grid(timesteps: int, steps: int) -> np.ndarray:
    """int64 [2N+1]: the teacher's grid tau = linear_tau(T, 2N), 0 = tau_0 < ... < tau_2N = T.  Refuses 2N > T and any grid whose points
    are not distinct."""
    T, N = int(timesteps), int(steps)
    if N < 1:
        raise ValueError(f"steps = {steps!r}; the student samples in at least 1 step")
    if 2 * N > T:
        raise ValueError(f"steps = {N}: the teacher's {2 * N} steps do not fit a process of {T} timesteps")
    tau = linear_tau(T, 2 * N).numpy().astype(np.int64)
    if tau[0] != 0 or tau[-1] != T or not bool((np.diff(tau) > 0).all()):
        raise ValueError(f"steps = {N}: the grid linear_tau({T}, {2 * N}) has points that are not distinct")
    return tau


def _x0_pair(prediction: str, alpha, sigma) -> Tuple[float, float]:
    """(p0, p1) with x0 = p0 out + p1 z for a network that predicts `prediction`"""
    if prediction == "eps":
        return -sigma / alpha, 1.0 / alpha
    if prediction == "x0":
        return 1.0, 0.0
    return -sigma, alpha


def distill_rows(alpha_bar, steps: int, prediction: str) -> Tuple[np.ndarray, np.ndarray]:
    """(rows float64 [N+1][12], tt int64 [N+1][2]) of include/dmme_hip.h: dmme_distill_*.  Row 0 is NaN (tt[0] = (0, 0)): no index 0."""
    if prediction not in _lib.PREDICTIONS:
        raise ValueError(f"prediction = {prediction!r}; use one of {tuple(_lib.PREDICTIONS)}")
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    N = int(steps)
    tau = distill_grid(ab.size - 1, N)
    alpha, sigma = np.sqrt(ab), np.sqrt(1.0 - ab)
    rows = np.zeros((N + 1, ROW), dtype=np.float64)
    rows[0] = np.nan
    tt = np.zeros((N + 1, 2), dtype=np.int64)
    for i in range(1, N + 1):
        t, m, e = int(tau[2 * i]), int(tau[2 * i - 1]), int(tau[2 * i - 2])
        r = rows[i]
        r[0], r[1] = _x0_pair(prediction, alpha[t], sigma[t])
        r[2], r[3] = _x0_pair(prediction, alpha[m], sigma[m])
        r[5] = sigma[m] / sigma[t]
        r[4] = alpha[m] - r[5] * alpha[t]
        if e == 0:
            r[6], r[7] = 0.0, 1.0
        else:
            st, sm, se = alpha[t] / sigma[t], alpha[m] / sigma[m], alpha[e] / sigma[e]
            r[6], r[7] = (sm - st) / (se - st), (se - sm) / (se - st)
        if prediction == "eps":
            r[8], r[9] = -alpha[t] / sigma[t], 1.0 / sigma[t]
        elif prediction == "x0":
            r[8], r[9] = 1.0, 0.0
        else:
            r[8], r[9] = -1.0 / sigma[t], alpha[t] / sigma[t]
        tt[i] = (t, m)
    return rows, tt


def _check_one_plane(net: nn.Module, what: str) -> None:
    """the refusal of dmme_unet_plan_set_prediction: one output plane, no labels"""
    cin, cout = getattr(net, "in_channels", None), getattr(net, "out_channels", None)
    if hasattr(net, "null_label") or (cin is not None and cout is not None and cin != cout):
        raise NotImplementedError(f"progressive distillation: the {what} must be an unconditional network with one output plane; conditional "
                                  "(classifier-free) and learned-variance networks are out of scope")


class ProgressiveDistillation(DDPM):
    """`self.model` is the student, trained by `training_step`; `teacher` is frozen, in eval mode, kept out of `parameters()` and
    `state_dict()`, and follows `.to(device)`.  Both predict `prediction`.  A saved checkpoint is an ordinary checkpoint of the student."""

    def __init__(self, student: nn.Module, teacher: nn.Module, timesteps: int = 1000, steps: int = 512, *, prediction: str = "v", clip_x0: bool = False,
                 loss_weight: str = "truncated-snr", snr_gamma: float = 5.0) -> None:
        _check_one_plane(student, "student")
        _check_one_plane(teacher, "teacher")
        if student is teacher:
            raise ValueError("progressive distillation: the student and the teacher are two networks (the teacher stays frozen)")
        super().__init__(student, timesteps, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma)
        object.__setattr__(self, "teacher", teacher)  # (not a registered submodule: no parameters(), no state_dict() entry)
        self._freeze_teacher()
        self.clip_x0 = bool(clip_x0)
        self.register_buffer("_status", torch.zeros(1, dtype=torch.int32), persistent=False)
        self.steps = 0
        self._set_steps(steps)

    def _freeze_teacher(self) -> None:
        self.teacher.eval()
        for p in self.teacher.parameters():
            p.requires_grad_(False)

    def _set_steps(self, steps: int) -> None:
        """the fp32 / int64 device tables of an N-step student, folded in float64 from alpha_bar and rounded once"""
        ab64 = self.alpha_bar.detach().reshape(-1).to(torch.float64).cpu().numpy()
        rows, tt = distill_rows(ab64, steps, self.prediction)
        dev = self.alpha_bar.device
        self.steps = int(steps)
        self.register_buffer("_rows", torch.from_numpy(rows.astype(np.float32)).reshape(-1).contiguous().to(dev), persistent=False)
        self.register_buffer("_tt", torch.from_numpy(tt).reshape(-1).contiguous().to(dev), persistent=False)

    def _apply(self, fn, *a, **kw):
        self.teacher._apply(fn, *a, **kw)
        return super()._apply(fn, *a, **kw)

    # ------------------------------------------------------------------ one step
    def _teacher_out(self, z: Tensor, t: Tensor) -> Tensor:
        with torch.no_grad():
            out = self.teacher(z, t)
        out = out.detach().to(torch.float32).contiguous()
        if tuple(out.shape) != tuple(z.shape):
            raise ValueError(f"progressive distillation: a teacher output of shape {tuple(out.shape)} for images {tuple(z.shape)} (one output plane only)")
        return out

    def distill_target(self, x_0: Tensor, index: Optional[Tensor] = None, noise: Optional[Tensor] = None):
        """(z_t, t, target, index): the noised images, their timesteps and the student's regression target - the noise launch, a teacher
        forward, the mid launch, a teacher forward, the target launch.  `index` (one student index in 1..N per image) / `noise` may be
        injected; by default index ~ uniform{1..N} and noise ~ N(0, I)."""
        x0 = x_0.detach().to(torch.float32).contiguous()
        dev, B, chw, N = x0.device, x0.size(0), x0[0].numel(), self.steps
        if index is None:
            index = uniform_int(1, N + 1, B, device=dev)
        if noise is None:
            noise = gaussian_like(x0)
        if index.numel() != B:
            raise ValueError(f"progressive distillation: {index.numel()} indices for {B} images")
        if not index.is_cuda and B and not (1 <= int(index.min()) and int(index.max()) <= N):
            raise ValueError(f"progressive distillation: a student index outside 1..{N}")
        idx = index.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        z = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(z.shape) != tuple(x0.shape):
            raise ValueError(f"progressive distillation: noise of shape {tuple(z.shape)} for images {tuple(x0.shape)}")
        lib, s = _lib.lib(), _lib.stream_ptr()
        z_t, z_m, target = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        tm = torch.empty((2, B), dtype=torch.int64, device=dev)
        t, m = tm[0], tm[1]
        _lib.check(lib.dmme_distill_noise(_lib.ptr(x0), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(self._tt), _lib.ptr(self._sqrt_alpha_bar),
                                          _lib.ptr(self._sqrt_one_minus_alpha_bar), N, B, chw, _lib.ptr(z_t), _lib.ptr(t), _lib.ptr(m), _lib.ptr(self._status), s),
                   "dmme_distill_noise")
        out1 = self._teacher_out(z_t, t)
        _lib.check(lib.dmme_distill_mid(self._pred, int(self.clip_x0), _lib.ptr(z_t), _lib.ptr(out1), _lib.ptr(self._rows), _lib.ptr(idx), N, B, chw, _lib.ptr(z_m), s),
                   "dmme_distill_mid")
        out2 = self._teacher_out(z_m, m)
        _lib.check(lib.dmme_distill_target(self._pred, int(self.clip_x0), _lib.ptr(z_t), _lib.ptr(out1), _lib.ptr(z_m), _lib.ptr(out2), _lib.ptr(self._rows),
                                           _lib.ptr(idx), N, B, chw, _lib.ptr(target), s), "dmme_distill_target")
        return z_t, t, target, idx

    def training_step(self, x_0: Tensor, index: Optional[Tensor] = None, noise: Optional[Tensor] = None) -> Tensor:
        """the distillation loss of one batch: the student's output at (z_t, t) against `distill_target`, weighted by `loss_weight` at t"""
        z_t, t, target, _ = self.distill_target(x_0, index, noise)
        return self._loss(self.model(z_t, t), target, t)

    def check_indices(self) -> None:
        """raises where a student index outside 1..N reached the device since the last call (synchronises: reads the status word)"""
        if int(self._status.item()) != 0:
            self._status.zero_()
            raise ValueError(f"progressive distillation: a student index outside 1..{self.steps} reached the device")

    # ------------------------------------------------------------------ stages
    @torch.no_grad()
    def halve(self):
        """the student becomes the next stage's teacher (its weights are copied on the device) and samples in N/2 steps from here on"""
        N = self.steps
        if N % 2 != 0:
            raise ValueError(f"halve: the student samples in {N} steps, an odd number")
        student, teacher = self.model, self.teacher
        if hasattr(student, "flat_parameters") and hasattr(teacher, "flat_parameters"):
            src, dst = student.flat_parameters(), teacher.flat_parameters()
            if src.numel() != dst.numel():
                raise ValueError("halve: the student and the teacher are networks of different sizes")
            dst.copy_(src)  # (the buffer's version moves: the teacher's next forward re-packs and re-folds)
        else:
            teacher.load_state_dict(student.state_dict())
        self._freeze_teacher()
        self._set_steps(N // 2)
        return self

    def sampler(self, **kw) -> GeneralizedDDIM:
        """the sampler the student is trained for: the deterministic paper-form DDIM chain over its N-point linear grid"""
        return GeneralizedDDIM(self.model, self.timesteps, self.steps, "linear", eta=0.0, prediction=self.prediction, **kw).to(self.alpha_bar.device)

    def distill_meta(self) -> dict:
        """what a checkpoint records next to the student's weights (checkpoint.py) and `trainer sample` reads back"""
        return {"steps": int(self.steps), "tau_schedule": "linear", "prediction": self.prediction}
