"""Consistency distillation (Song, Dhariwal, Chen & Sutskever 2023, Algorithm 2) over the HIP kernels, on the discrete grid and with the
boundary scalings that Latent Consistency Models made standard (Luo et al. 2023): ONE training run, after which the student samples in
K = 1, 2 or 4 network evaluations from the same weights.  The reference project has no such method.

The grid is tau = linear_tau(T, N), the one `GeneralizedDDIM(..., "linear")` samples on.  Index i in 1..N stands for t = tau[i],
m = tau[i-1]; m = 0 exactly when i = 1.  With sd = sigma_data and s = timestep_scaling, per image:

    cs(t) = sd^2 / ((s t)^2 + sd^2),   co(t) = s t / sqrt((s t)^2 + sd^2)            cs(0) = 1, co(0) = 0
    x0(z, t; out) = p0 out + p1 z                                                  distill.py's _x0_pair for eps / x0 / v
    f(z, t; out)  = cs(t) z + co(t) x0(z, t; out)                                  the consistency function; f(z, 0; .) = z

    z_t   = alpha_t x_0 + sigma_t eps                                              (dmme_distill_noise)
    x1    = the frozen teacher's x0 estimate at (z_t, t)                           [clamped to [-1, 1] iff clip_x0]
    zh_m  = alpha_m x1 + (sigma_m / sigma_t)(z_t - alpha_t x1)                      (dmme_distill_mid; zh_m = x1 where m = 0)
    f_tgt = f(zh_m, m; target network at (zh_m, max(m, 1)))                        (dmme_cm_target; no grad, x0 clamped iff clip_x0)
    loss  = (1/B) sum_b d(f(z_t, t; student(z_t, t))_b, f_tgt_b)                    (dmme_cm_loss)

d is the pseudo-Huber metric sqrt(S_b + c^2) - c over one image's sum of squares S_b (default, c = 0.00054 sqrt(chw)) or S_b / chw.
Every scalar is folded on the host in float64 and rounded once (include/dmme_hip.h: dmme_cm_*)."""

from __future__ import annotations

import copy
import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian_like, uniform_int
from ..equations.ddim import linear_tau
from .ddim import GeneralizedDDIM
from .ddpm import DDPM
from .distill import _x0_pair

ROW = 12  # floats per table row: p0 p1 | p0' p1' | m0 m1 | cs co | cs' co' | two spare
HUBER_C = 0.00054  # the pseudo-Huber constant per sqrt(chw) (Song & Dhariwal 2023)


def consistency_grid(timesteps: int, steps: int) -> np.ndarray:
    """int64 [N+1]: tau = linear_tau(T, N), 0 = tau_0 < ... < tau_N = T.  Refuses N > T and any grid whose points are not distinct."""
    T, N = int(timesteps), int(steps)
    if N < 1:
        raise ValueError(f"steps = {steps!r}; the grid has at least 1 step")
    if N > T:
        raise ValueError(f"steps = {N}: the grid does not fit a process of {T} timesteps")
    tau = linear_tau(T, N).numpy().astype(np.int64)
    if tau[0] != 0 or tau[-1] != T or not bool((np.diff(tau) > 0).all()):
        raise ValueError(f"steps = {N}: the grid linear_tau({T}, {N}) has points that are not distinct")
    return tau


def boundary_scalings(t, sigma_data: float = 0.5, timestep_scaling: float = 10.0) -> Tuple[float, float]:
    """(cs(t), co(t)) in float64: LCM's scalings_for_boundary_conditions on this project's indices (t = 0 is the clean image)"""
    st, sd2 = float(timestep_scaling) * float(t), float(sigma_data) ** 2
    return sd2 / (st * st + sd2), st / math.sqrt(st * st + sd2)


def _check_scalings(sigma_data, timestep_scaling) -> Tuple[float, float]:
    sd, s = float(sigma_data), float(timestep_scaling)
    if not (sd > 0.0 and math.isfinite(sd)) or not (s > 0.0 and math.isfinite(s)):
        raise ValueError(f"sigma_data = {sigma_data!r}, timestep_scaling = {timestep_scaling!r}; two positive numbers")
    return sd, s


def consistency_rows(alpha_bar, steps: int, prediction: str, sigma_data: float = 0.5, timestep_scaling: float = 10.0) -> Tuple[np.ndarray, np.ndarray]:
    """(rows float64 [N+1][12], tt int64 [N+1][2]) of include/dmme_hip.h: dmme_cm_*.  Row 0 is NaN (tt[0] = (0, 0)): no index 0.  The
    unprimed slots are taken at t, the primed ones at the true m; tt[i] = (t, max(m, 1)): column 1 is the timestep the target network is
    evaluated at, the rows are what carry m = 0 - there (m0, m1) = (1, 0), (cs', co') = (1, 0) and (p0', p1') = (-0, 1) for an eps or v
    network ((1, 0) for an x0 network, as at every timestep), with no division by sigma anywhere."""
    if prediction not in _lib.PREDICTIONS:
        raise ValueError(f"prediction = {prediction!r}; use one of {tuple(_lib.PREDICTIONS)}")
    sd, s = _check_scalings(sigma_data, timestep_scaling)
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    N = int(steps)
    tau = consistency_grid(ab.size - 1, N)
    alpha, sigma = np.sqrt(ab), np.sqrt(1.0 - ab)
    rows = np.zeros((N + 1, ROW), dtype=np.float64)
    rows[0] = np.nan
    tt = np.zeros((N + 1, 2), dtype=np.int64)
    for i in range(1, N + 1):
        t, m = int(tau[i]), int(tau[i - 1])
        r = rows[i]
        r[0], r[1] = _x0_pair(prediction, alpha[t], sigma[t])
        r[2], r[3] = _x0_pair(prediction, alpha[m], sigma[m])
        r[5] = sigma[m] / sigma[t]
        r[4] = alpha[m] - r[5] * alpha[t]
        r[6], r[7] = boundary_scalings(t, sd, s)
        r[8], r[9] = boundary_scalings(m, sd, s)
        tt[i] = (t, max(m, 1))
    return rows, tt


def consistency_sampler_rows(alpha_bar, sample_steps: int, sigma_data: float = 0.5, timestep_scaling: float = 10.0):
    """float64 [K+1][3]: (k0, k1, k2) of multistep consistency sampling on linear_tau(T, K), in the eps form a chain sees behind the
    prediction adapter: for the step a = tau[i] -> p = tau[i-1], x' = alpha_p f(x, a) + sigma_p z with x0 = (x - sigma_a eps) / alpha_a:

        k0 = alpha_p (cs(a) + co(a) / alpha_a),   k1 = -alpha_p co(a) sigma_a / alpha_a,   k2 = sigma_p   (0 for the last step)

    Row 0 is (1, 0, 0): index 0 is never stepped from."""
    sd, s = _check_scalings(sigma_data, timestep_scaling)
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    K = int(sample_steps)
    tau = consistency_grid(ab.size - 1, K)
    alpha, sigma = np.sqrt(ab), np.sqrt(1.0 - ab)
    out = np.zeros((K + 1, 3), dtype=np.float64)
    out[0, 0] = 1.0
    for i in range(1, K + 1):
        a, p = int(tau[i]), int(tau[i - 1])
        cs, co = boundary_scalings(a, sd, s)
        out[i] = (alpha[p] * (cs + co / alpha[a]), -alpha[p] * co * sigma[a] / alpha[a], sigma[p] if p > 0 else 0.0)
    return out


def _check_one_plane(net: nn.Module, what: str) -> None:
    """the refusal of dmme_unet_plan_set_prediction: one output plane, no labels"""
    cin, cout = getattr(net, "in_channels", None), getattr(net, "out_channels", None)
    if hasattr(net, "null_label") or (cin is not None and cout is not None and cin != cout):
        raise NotImplementedError(f"consistency distillation: the {what} must be an unconditional network with one output plane; conditional "
                                  "(classifier-free) and learned-variance networks are out of scope")


def _freeze(net: nn.Module) -> None:
    net.eval()
    for p in net.parameters():
        p.requires_grad_(False)


def _clone_network(net: nn.Module) -> nn.Module:
    """a second network of the same class and size with the same weights (a dmme_amd UNet: without the plans it has built; they hold
    device buffers and library handles, and the copy builds its own)"""
    held = {k: net.__dict__.pop(k) for k in ("_plans", "_flat_grad", "_bucket_hook", "_grad_reducer") if k in net.__dict__}
    try:
        for k, v in held.items():
            net.__dict__[k] = {} if k == "_plans" else None
        twin = copy.deepcopy(net)
    finally:
        net.__dict__.update(held)
    twin.__dict__.pop("_grad_reducer", None)
    return twin


class ConsistencyDistillation(DDPM):
    """`self.model` is the student, trained by `training_step`; `teacher` is frozen, in eval mode, kept out of `parameters()` and
    `state_dict()`, and follows `.to(device)`.  Both predict `prediction` (v is recommended: see `ConsistencySampler`).

    The target network: with `target_decay == 0` it is the student itself, evaluated under no_grad in eval mode BEFORE the student's
    training forward of the same step (so the workspace the backward reads is the training forward's); the student's training mode is
    restored afterwards.  With `target_decay > 0` it is a third network of the same size, `self.target`, held like the teacher and
    initialised from the student; `after_step()` moves it towards the student, target = decay target + (1 - decay) student
    (dmme_ema_lerp on the flat parameter buffers), and `target_decay == 1` never moves it.  The target network is not part of a
    checkpoint: resuming from one restarts the target from the student's loaded weights (call `reset_target()` after loading into an
    existing process; the trainer builds the process after loading, which has the same effect)."""

    def __init__(self, student: nn.Module, teacher: nn.Module, timesteps: int = 1000, steps: int = 50, *, prediction: str = "v", clip_x0: bool = False,
                 metric: str = "pseudo-huber", huber_c: Optional[float] = None, target_decay: float = 0.0, sigma_data: float = 0.5,
                 timestep_scaling: float = 10.0) -> None:
        _check_one_plane(student, "student")
        _check_one_plane(teacher, "teacher")
        if student is teacher:
            raise ValueError("consistency distillation: the student and the teacher are two networks (the teacher stays frozen)")
        if metric not in _lib.CM_METRICS:
            raise ValueError(f"metric = {metric!r}; use one of {tuple(_lib.CM_METRICS)}")
        if huber_c is not None and (isinstance(huber_c, bool) or not (float(huber_c) > 0.0 and math.isfinite(float(huber_c)))):
            raise ValueError(f"huber_c = {huber_c!r}; a positive number (default: {HUBER_C} sqrt(chw))")
        if isinstance(target_decay, bool) or not 0.0 <= float(target_decay) <= 1.0:
            raise ValueError(f"target_decay = {target_decay!r}; a number in [0, 1]")
        sd, s = _check_scalings(sigma_data, timestep_scaling)
        consistency_grid(timesteps, steps)  # (refuses before anything is built)
        super().__init__(student, timesteps, prediction=prediction)
        object.__setattr__(self, "teacher", teacher)  # (not a registered submodule: no parameters(), no state_dict() entry)
        _freeze(teacher)
        self.clip_x0 = bool(clip_x0)
        self.metric, self._metric = metric, _lib.CM_METRICS[metric]
        self.huber_c = None if huber_c is None else float(huber_c)
        self.target_decay = float(target_decay)
        self.sigma_data, self.timestep_scaling = sd, s
        object.__setattr__(self, "target", None)
        if self.target_decay > 0.0:
            object.__setattr__(self, "target", _clone_network(student))
            _freeze(self.target)
        self.register_buffer("_status", torch.zeros(1, dtype=torch.int32), persistent=False)
        ab64 = self.alpha_bar.detach().reshape(-1).to(torch.float64).cpu().numpy()
        rows, tt = consistency_rows(ab64, steps, self.prediction, sd, s)
        self.steps = int(steps)
        self.register_buffer("_rows", torch.from_numpy(rows.astype(np.float32)).reshape(-1).contiguous(), persistent=False)
        self.register_buffer("_tt", torch.from_numpy(tt).reshape(-1).contiguous(), persistent=False)

    def _apply(self, fn, *a, **kw):
        self.teacher._apply(fn, *a, **kw)
        if self.target is not None:
            self.target._apply(fn, *a, **kw)
        return super()._apply(fn, *a, **kw)

    # ------------------------------------------------------------------ one step
    def _nograd_out(self, net: nn.Module, z: Tensor, t: Tensor, what: str) -> Tensor:
        with torch.no_grad():
            out = net(z, t)
        out = out.detach().to(torch.float32).contiguous()
        if tuple(out.shape) != tuple(z.shape):
            raise ValueError(f"consistency distillation: a {what} output of shape {tuple(out.shape)} for images {tuple(z.shape)} (one output plane only)")
        return out

    def _target_out(self, z: Tensor, t: Tensor) -> Tensor:
        """the target network's raw output at (z, t), no grad: `self.target`, or the student itself in eval mode (its mode restored)"""
        if self.target is not None:
            return self._nograd_out(self.target, z, t, "target network")
        student = self.model
        was_training = student.training
        student.eval()
        try:
            return self._nograd_out(student, z, t, "student").clone()  # (a copy: the training forward that follows owns the network's buffers)
        finally:
            student.train(was_training)

    def huber_constant(self, chw: int) -> float:
        """c of the pseudo-Huber metric for images of chw elements: `huber_c`, or 0.00054 sqrt(chw)"""
        return self.huber_c if self.huber_c is not None else HUBER_C * math.sqrt(float(chw))

    def consistency_target(self, x_0: Tensor, index: Optional[Tensor] = None, noise: Optional[Tensor] = None):
        """(z_t, t, f_target, index): the noised images, their timesteps and the target network's consistency function one teacher step
        down the grid - the noise launch, a teacher forward, the mid launch, a target-network forward, the target launch.  `index` (one
        grid index in 1..N per image) / `noise` may be injected; by default index ~ uniform{1..N} and noise ~ N(0, I)."""
        x0 = x_0.detach().to(torch.float32).contiguous()
        dev, B, chw, N = x0.device, x0.size(0), x0[0].numel(), self.steps
        if index is None:
            index = uniform_int(1, N + 1, B, device=dev)
        if noise is None:
            noise = gaussian_like(x0)
        if index.numel() != B:
            raise ValueError(f"consistency distillation: {index.numel()} indices for {B} images")
        if not index.is_cuda and B and not (1 <= int(index.min()) and int(index.max()) <= N):
            raise ValueError(f"consistency distillation: a grid index outside 1..{N}")
        idx = index.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        z = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(z.shape) != tuple(x0.shape):
            raise ValueError(f"consistency distillation: noise of shape {tuple(z.shape)} for images {tuple(x0.shape)}")
        lib, s = _lib.lib(), _lib.stream_ptr()
        z_t, z_m, f_target = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        tm = torch.empty((2, B), dtype=torch.int64, device=dev)
        t, m = tm[0], tm[1]
        _lib.check(lib.dmme_distill_noise(_lib.ptr(x0), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(self._tt), _lib.ptr(self._sqrt_alpha_bar),
                                          _lib.ptr(self._sqrt_one_minus_alpha_bar), N, B, chw, _lib.ptr(z_t), _lib.ptr(t), _lib.ptr(m), _lib.ptr(self._status), s),
                   "dmme_distill_noise")
        out1 = self._nograd_out(self.teacher, z_t, t, "teacher")
        _lib.check(lib.dmme_distill_mid(self._pred, int(self.clip_x0), _lib.ptr(z_t), _lib.ptr(out1), _lib.ptr(self._rows), _lib.ptr(idx), N, B, chw, _lib.ptr(z_m), s),
                   "dmme_distill_mid")
        out_m = self._target_out(z_m, m)
        _lib.check(lib.dmme_cm_target(int(self.clip_x0), _lib.ptr(z_m), _lib.ptr(out_m), _lib.ptr(self._rows), _lib.ptr(idx), N, B, chw, _lib.ptr(f_target), s),
                   "dmme_cm_target")
        return z_t, t, f_target, idx

    def training_step(self, x_0: Tensor, index: Optional[Tensor] = None, noise: Optional[Tensor] = None) -> Tensor:
        """the consistency loss of one batch: f of the student's output at (z_t, t) against `consistency_target` under the metric"""
        from ..autograd import consistency_loss_apply

        z_t, t, f_target, idx = self.consistency_target(x_0, index, noise)
        return consistency_loss_apply(self.model(z_t, t), z_t, f_target, self._rows, idx, self.steps, self._metric, self.huber_constant(z_t[0].numel()))

    def check_indices(self) -> None:
        """raises where a grid index outside 1..N reached the device since the last call (synchronises: reads the status word)"""
        if int(self._status.item()) != 0:
            self._status.zero_()
            raise ValueError(f"consistency distillation: a grid index outside 1..{self.steps} reached the device")

    # ------------------------------------------------------------------ the target network's moving average
    @torch.no_grad()
    def after_step(self) -> None:
        """call after every optimiser step: target = decay target + (1 - decay) student.  Nothing to do at decay 0 (the target is the
        student) and at decay 1 (the target never moves)."""
        if self.target is None or self.target_decay >= 1.0:
            return
        lib, s = _lib.lib(), _lib.stream_ptr()
        student, target = self.model, self.target
        if hasattr(student, "flat_parameters") and hasattr(target, "flat_parameters"):
            pairs = [(target.flat_parameters(), student.flat_parameters())]
        else:
            pairs = list(zip(target.parameters(), student.parameters()))
        for dst, src in pairs:
            if dst.numel() != src.numel() or dst.dtype != torch.float32 or src.dtype != torch.float32 or not (dst.is_contiguous() and src.is_contiguous()):
                raise ValueError("after_step: the target and the student hold contiguous fp32 parameters of the same sizes")
            if dst.numel():
                _lib.check(lib.dmme_ema_lerp(_lib.ptr(dst), _lib.ptr(src), dst.numel(), self.target_decay, s), "dmme_ema_lerp")
        if hasattr(target, "mark_params_updated"):
            target.mark_params_updated()  # (the buffer's version moves: the target's next forward re-packs and re-folds)

    @torch.no_grad()
    def reset_target(self) -> None:
        """the target network restarts from the student's current weights (after loading a checkpoint into the student)"""
        if self.target is None:
            return
        student, target = self.model, self.target
        if hasattr(student, "flat_parameters") and hasattr(target, "flat_parameters"):
            target.flat_parameters().copy_(student.flat_parameters())
        else:
            target.load_state_dict(student.state_dict())
        _freeze(target)

    # ------------------------------------------------------------------ sampling
    def sampler(self, sample_steps: int = 1, **kw) -> "ConsistencySampler":
        """the K-step sampler of the student (K divides N): multistep consistency sampling over linear_tau(T, K)"""
        return ConsistencySampler(self.model, self.timesteps, sample_steps, self.steps, prediction=self.prediction, sigma_data=self.sigma_data,
                                  timestep_scaling=self.timestep_scaling, **kw).to(self.alpha_bar.device)

    def consistency_meta(self) -> dict:
        """what a checkpoint records next to the student's weights (checkpoint.py) and `trainer sample` reads back"""
        return {"steps": int(self.steps), "prediction": self.prediction, "sigma_data": float(self.sigma_data), "timestep_scaling": float(self.timestep_scaling)}


class ConsistencySampler(GeneralizedDDIM):
    r"""Multistep consistency sampling (Song et al. 2023, Algorithm 1) of a consistency-distilled network in K evaluations: a
    `GeneralizedDDIM(model, T, K, "linear", eta=0)` whose reverse rows are replaced by

        x' = alpha_p f(x, a) + sigma_p z       for the step a = tau[i] -> p = tau[i-1];  the last step (p = 0) returns f(x, a)

    folded in float64 in the eps form the chain sees behind the prediction adapter (`consistency_sampler_rows`).  It runs on the
    DMME_CHAIN_GDDIM kind: the captured step, history grids and `threshold=` work as for every GDDIM chain, and noise is drawn where
    k2 != 0.  K must divide the N of the training grid, so that every timestep visited is one the student was trained at
    (linear_tau(T, K) == linear_tau(T, N)[::N/K]).  `encode` and `interpolate` raise: a consistency map has no forward direction.

    Use a v-prediction network: with an eps network the one-step sample divides by alpha_T, and 1 / alpha_T (157 on the linear schedule
    at T = 1000) multiplies the network's error."""

    def __init__(self, model: nn.Module, timesteps: int = 1000, sample_steps: int = 1, train_steps: Optional[int] = None, *, prediction: str = "v",
                 sigma_data: float = 0.5, timestep_scaling: float = 10.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        K = int(sample_steps)
        N = K if train_steps is None else int(train_steps)
        if K < 1 or N < 1 or N % K != 0:
            raise ValueError(f"sample_steps = {sample_steps!r} does not divide the training grid's {N} steps")
        tau_n, tau_k = consistency_grid(timesteps, N), consistency_grid(timesteps, K)
        if not np.array_equal(tau_k, tau_n[:: N // K]):
            raise ValueError(f"sample_steps = {K}: linear_tau({timesteps}, {K}) leaves the training grid linear_tau({timesteps}, {N})")
        sd, s = _check_scalings(sigma_data, timestep_scaling)
        super().__init__(model, timesteps, K, "linear", 0.0, prediction=prediction, threshold=threshold, threshold_percentile=threshold_percentile)
        self.train_steps, self.sigma_data, self.timestep_scaling = N, sd, s
        ab = self.alpha_bar.reshape(-1).to(torch.float64).cpu().numpy()
        rows = consistency_sampler_rows(ab, K, sd, s)
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        self._rev_rows = [(f32(k0), f32(k1), f32(k2), 0.0) for k0, k1, k2 in rows]
        self._draws = any(r[2] != 0.0 for r in self._rev_rows)

    def encode(self, x0: Tensor, upto: Optional[int] = None) -> Tensor:
        raise NotImplementedError("ConsistencySampler.encode: a consistency map has no forward direction")

    def interpolate(self, xa: Tensor, xb: Tensor, weights) -> Tensor:
        raise NotImplementedError("ConsistencySampler.interpolate: a consistency map has no forward direction")
