"""Improved DDPM (cosine schedule, learned variance, hybrid loss) over the HIP kernels.

Drop-in for the reference's `dmme.diffusion_models.IDDPM` (src/dmme/diffusion_models/iddpm.py:16-164): same
constructor, buffers and methods.  The model returns (N, 2C, H, W) = (eps, v); the variance interpolation, the
reverse update, L_simple, L_vlb (discrete NLL at t == 1, KL elsewhere, stop-gradient on eps) and their gradient
w.r.t. the network output are fused HIP kernels (dmme_iddpm_step, dmme_iddpm_loss).

Beyond the reference, the three things Nichol & Dhariwal 2021 use those parts for: `generate(..., sample_steps=K)` (a strided chain
that keeps the learned variance, section 4), `t_sampler="loss-second-moment"` (importance-sampled timesteps for L_vlb, section 3.3)
and `bits_per_dim` (the paper's metric, the full variational bound)."""

from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, gaussian_like, pad, philox_reserve, uniform_int
from ..equations.iddpm import cosine_schedule, interpolate_variance, process_coefficients, respaced_coefficients, space_timesteps
from .ddpm import DDPM, ChainRunner

NoiseVariance = namedtuple("NoiseVariance", ["noise", "variance"])
BitsPerDim = namedtuple("BitsPerDim", ["total", "prior", "terms"])
TimestepDraw = namedtuple("TimestepDraw", ["t", "weight", "rows"])

T_SAMPLERS = ("uniform", "loss-second-moment")
TS_HISTORY = 10          # losses kept per timestep (the paper's code)
TS_UNIFORM_PROB = 0.001  # share of the draw that stays uniform once the history is full


class IDDPM(DDPM):
    def __init__(
        self,
        model: nn.Module,
        timesteps: int = 1000,
        loss_type="hybrid",
        gamma=0.001,
        schedule: str = "cosine",
        offset=0.008,
        start: float = 0.0001,
        end: float = 0.02,
        t_sampler: str = "uniform",
        *,
        prediction: str = "eps",
        loss_weight: str = "uniform",
        snr_gamma: float = 5.0,
    ) -> None:
        if prediction != "eps" or loss_weight != "uniform":
            raise ValueError(f"IDDPM predicts (eps, v-interpolated variance) and trains on its hybrid loss: prediction = {prediction!r} / loss_weight = "
                             f"{loss_weight!r} are not supported (only 'eps' / 'uniform'); x0 / v networks run under DDPM, DDIM, DPMSolverPP, RePaint and the guided processes")
        super().__init__(model, timesteps, start, end)
        if t_sampler not in T_SAMPLERS:
            raise ValueError(f"t_sampler = {t_sampler!r}; use one of {T_SAMPLERS}")
        self.t_sampler = t_sampler
        self.loss_type = loss_type
        self.gamma = gamma
        if schedule == "cosine":
            alpha_bar = cosine_schedule(timesteps, offset).reshape(-1, 1, 1, 1)
            # clip to prevent singularities near t = T; the front pad is 1, not 0 (reference :51-52)
            beta = torch.clip(1 - alpha_bar[1:] / alpha_bar[:-1], 0, 0.999)
            beta = pad(beta, value=1)
            alpha = 1 - beta
            self.register_buffer("beta", beta, persistent=False)
            self.register_buffer("alpha", alpha, persistent=False)
            self.register_buffer("alpha_bar", alpha_bar, persistent=False)
            self.register_buffer("_sqrt_alpha_bar", torch.sqrt(alpha_bar).reshape(-1).contiguous(), persistent=False)
            self.register_buffer("_sqrt_one_minus_alpha_bar", torch.sqrt(1 - alpha_bar).reshape(-1).contiguous(), persistent=False)
        elif schedule != "linear":
            raise NotImplementedError
        coef = process_coefficients(self.beta, self.alpha, self.alpha_bar)
        self.register_buffer("_coef", coef.contiguous(), persistent=False)  # device table of the loss kernel
        self._coef_host = coef.tolist()                                      # python floats of the sampler kernel
        self.last_draw: Optional[TimestepDraw] = None
        if t_sampler == "loss-second-moment":
            # the resampler's state travels in the state_dict (and so in checkpoints); nothing is registered in "uniform" mode
            self.register_buffer("_ts_hist", torch.zeros(timesteps + 1, TS_HISTORY, dtype=torch.float32))
            self.register_buffer("_ts_count", torch.zeros(timesteps + 1, dtype=torch.int32))
            self.register_buffer("_ts_p", torch.zeros(timesteps + 1, dtype=torch.float32), persistent=False)   # last draw's probabilities (logging)
            self.register_buffer("_ts_status", torch.zeros(1, dtype=torch.int32), persistent=False)           # set by a kernel that skipped an entry

    # ------------------------------------------------------------------ training
    def draw_timesteps(self, count: int):
        r"""(t, weight), `count` of each, from the loss-second-moment resampler (dmme_tsampler_draw): uniform over 1..T with weight 1
        until every timestep has TS_HISTORY losses, then p_t proportional to sqrt(E[L_t^2]) (mixed with TS_UNIFORM_PROB of uniform)
        and weight 1/(T p_t), which keeps the weighted loss an unbiased estimate of the uniform one.  The range includes T, unlike
        the reference's `uniform_int(1, T)`: a timestep that is never drawn would keep the history from ever filling.  The uniforms
        come from the device's Philox stream at torch's CUDA generator state; `self._ts_p` keeps the probabilities of the draw."""
        if self.t_sampler != "loss-second-moment":
            raise RuntimeError('draw_timesteps needs t_sampler="loss-second-moment"')
        dev = self._ts_hist.device
        seed, off = philox_reserve(dev, count)
        t = torch.empty(count, dtype=torch.int64, device=dev)
        weight = torch.empty(count, dtype=torch.float32, device=dev)
        _lib.check(
            _lib.lib().dmme_tsampler_draw(_lib.ptr(self._ts_hist), _lib.ptr(self._ts_count), self.timesteps, TS_HISTORY, TS_UNIFORM_PROB, seed, off,
                                          count, _lib.ptr(t), _lib.ptr(weight), _lib.ptr(self._ts_p), _lib.stream_ptr()),
            "dmme_tsampler_draw",
        )
        return t, weight

    def check_t_sampler(self) -> None:
        """synchronising check of the resampler's status word: raises if a training step met a timestep outside 1..T or a non-finite
        per-image loss (such entries are skipped, never stored)"""
        if self.t_sampler == "loss-second-moment" and int(self._ts_status.item()) != 0:
            self._ts_status.zero_()
            raise _lib.DmmeError("loss-second-moment resampler: a timestep outside 1..T or a non-finite per-image loss was skipped")

    def _training_step_resampled(self, x_0: Tensor, t: Optional[Tensor], noise: Optional[Tensor], weight: Optional[Tensor]):
        r"""the step of t_sampler="loss-second-moment", without a host synchronisation: Philox span, dmme_tsampler_draw, dmme_q_sample, the
        model, dmme_iddpm_loss_rows (loss = mean_b weight_b row_b and its gradient), dmme_tsampler_update with the unweighted rows.
        Data parallel: each rank keeps its own history and draws from it; the estimate is unbiased on every rank, so the averaged
        gradient is too, and no collective is added."""
        from ..autograd import iddpm_loss_rows_apply

        if self.loss_type not in ("vlb", "hybrid"):
            return None
        B = x_0.size(0)
        if t is None:
            t, drawn = self.draw_timesteps(B)
            weight = drawn if weight is None else weight
        if noise is None:
            noise = gaussian_like(x_0)
        x0, t, x_t, target = self._noised(x_0, t, noise)
        model_output = self.model(x_t, t)
        w_simple, w_vlb = (0.0, 1.0) if self.loss_type == "vlb" else (1.0, float(self.gamma))
        loss, rows = iddpm_loss_rows_apply(model_output, x_t, x0, target, t, self._coef, self.timesteps, weight, w_simple, w_vlb, self._ts_status)
        _lib.check(
            _lib.lib().dmme_tsampler_update(_lib.ptr(self._ts_hist), _lib.ptr(self._ts_count), self.timesteps, TS_HISTORY, _lib.ptr(t), _lib.ptr(rows[2]), B,
                                            _lib.ptr(self._ts_status), _lib.stream_ptr()),
            "dmme_tsampler_update",
        )
        self.last_draw = TimestepDraw(t, weight, rows)
        return loss

    def training_step(self, x_0: Tensor, t: Optional[Tensor] = None, noise: Optional[Tensor] = None, weight: Optional[Tensor] = None):
        r"""hybrid loss L_simple + gamma L_vlb, or L_vlb alone (reference: diffusion_models/iddpm.py:62-116).
        As in the reference, any other `loss_type` (e.g. "simple") falls through and returns None.
        `t` / `noise` may be injected for parity tests.  With t_sampler="loss-second-moment" the timesteps are importance-sampled and
        the loss is weighted (`_training_step_resampled`); there an injected `t` bypasses the draw with weight 1, `weight` (tests)
        replaces the weights, and `last_draw` keeps (t, weight, per-image rows) of the step."""
        from ..autograd import iddpm_loss_apply

        if self.t_sampler == "loss-second-moment":
            return self._training_step_resampled(x_0, t, noise, weight)
        if weight is not None:
            raise ValueError('per-image weights need t_sampler="loss-second-moment"')
        if t is None:
            t = uniform_int(1, self.timesteps, x_0.size(0), device=x_0.device)
        if noise is None:
            noise = gaussian_like(x_0)
        x0, t, x_t, target = self._noised(x_0, t, noise)
        model_output = self.model(x_t, t)
        if self.loss_type == "vlb":
            return iddpm_loss_apply(model_output, x_t, x0, target, t, self._coef, 0.0, 1.0)
        if self.loss_type == "hybrid":
            return iddpm_loss_apply(model_output, x_t, x0, target, t, self._coef, 1.0, float(self.gamma))
        return None

    # ------------------------------------------------------------------ sampling
    _chain_kind = _lib.CHAIN_IDDPM

    def _chain_tables(self):
        T = self.timesteps
        finite = lambda v: v if v == v and abs(v) != float("inf") else 0.0  # row 0 is never stepped from
        rows = [tuple(finite(v) for v in self._coef_host[t][:4]) for t in range(T + 1)]
        return T, rows, list(range(T + 1))

    def _respaced_tables(self, sample_steps: int):
        """`_chain_tables` of the chain over K = sample_steps timesteps: loop index k stands for timestep s_k (t_table = [0, s_1 .. s_K]),
        row k for the step s_k -> s_{k-1}.  s_1 = 1, so the chain kernel's "no noise at t == 1" falls on the last step unchanged."""
        steps = space_timesteps(self.timesteps, sample_steps)
        rows = [tuple(r) for r in respaced_coefficients(self.alpha_bar, steps).tolist()]
        return len(steps), rows, [0] + steps

    def respaced_runner(self, x: Tensor, sample_steps: int, use_graph: bool = True) -> Optional[ChainRunner]:
        """the replayable step of the K-step chain, bound to the image buffer `x`: one runner slot per K (None where `chain_runner` is)"""
        K = int(sample_steps)
        return self.chain_runner(x, use_graph, slot=f"_runner_k{K}", spec=lambda: (_lib.CHAIN_IDDPM, self._respaced_tables(K)))

    @torch.no_grad()
    def generate(self, img_size, sample_steps: Optional[int] = None, history=None) -> Tensor:
        """the full T-step chain from pure noise, or with `sample_steps` = K the strided chain over K << T timesteps with the learned
        variance (Nichol & Dhariwal 2021, section 4): K network evaluations instead of T, graph-replayed like the full chain.
        `history`: a HistoryRecorder for the chain's frames"""
        if sample_steps is None:
            return super().generate(img_size, history=history)
        K, rows, ttab = self._respaced_tables(int(sample_steps))
        dev = self.beta.device
        x_t = gaussian(img_size, device=dev)
        runner = self._buffered_runner(f"_runner_k{K}", img_size, dev, spec=lambda: (_lib.CHAIN_IDDPM, (K, rows, ttab)))  # (on the full chain's buffer)
        return self._run_chain(runner, x_t, K, K, lambda k: self._reverse_update(x_t, self._eps(x_t, self.timestep_tensor(ttab[k], dev)), ttab[k], None, rows[k]), history)

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def bits_per_dim(self, x_0: Tensor, noise: Optional[Tensor] = None) -> BitsPerDim:
        r"""the variational bound on -log p(x_0) in bits/dim (the paper's NLL metric): (total[B], prior[B], terms[B, T]) with
        terms[:, t-1] = L_{t-1} (the discrete NLL for t = 1, KL(q(x_{t-1} | x_t, x_0) || p_theta) above), prior = KL(q(x_T | x_0) || N(0, I))
        and total = prior + sum_t terms, each a mean over the image's elements divided by ln 2.  An eager loop over t = T .. 1 of
        dmme_q_sample, the model and dmme_iddpm_loss_rows (no gradient, w_vlb = 1); `noise` (T, B, C, H, W): noise[t-1] is the draw
        of step t (default: fresh normals).  Nothing is read back inside the loop; the kernels' status word is read once at the end."""
        T, B = self.timesteps, x_0.size(0)
        x0 = x_0.detach().to(torch.float32).contiguous()
        dev, chw = x0.device, x0[0].numel()
        lib = _lib.lib()
        loss = torch.empty(3, dtype=torch.float32, device=dev)
        rows = torch.empty((3, B), dtype=torch.float32, device=dev)
        scratch = torch.empty(64 * B, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        terms = torch.empty((T, B), dtype=torch.float32, device=dev)
        prior = torch.empty(B, dtype=torch.float32, device=dev)
        coef = self._coef.to(device=dev, dtype=torch.float32).contiguous()
        for step in range(T, 0, -1):
            t = torch.full((B,), step, dtype=torch.int64, device=dev)
            _, _, x_t, target = self._noised(x0, t, gaussian_like(x0) if noise is None else noise[step - 1])
            out = self.model(x_t, t).detach().to(torch.float32).contiguous()
            _lib.check(
                lib.dmme_iddpm_loss_rows(_lib.ptr(out), _lib.ptr(x_t), _lib.ptr(x0), _lib.ptr(target), _lib.ptr(t), _lib.ptr(coef), T, None, B, chw, 0.0, 1.0,
                                         _lib.ptr(loss), _lib.ptr(rows), None, 1.0, _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr()),
                "dmme_iddpm_loss_rows",
            )
            terms[step - 1] = rows[1] / math.log(2.0)
        _lib.check(lib.dmme_iddpm_prior_rows(_lib.ptr(x0), B, chw, float(self.alpha_bar.reshape(-1)[T]), _lib.ptr(prior), _lib.stream_ptr()), "dmme_iddpm_prior_rows")
        prior = prior / math.log(2.0)
        if int(status.item()) != 0:
            raise _lib.DmmeError("bits_per_dim: a timestep left the coefficient table")
        terms = terms.t().contiguous()
        return BitsPerDim(prior + terms.sum(dim=1), prior, terms)

    def _reverse_update(self, x_t: Tensor, model_output: Tensor, t: int, noise: Optional[Tensor], row=None) -> Tensor:
        """`row`: the scalars of a strided chain's step in place of the full chain's at t"""
        if noise is None:
            noise = gaussian_like(x_t)  # drawn even when t == 1, then unused (reference :144-149)
        c = self._coef_host[t] if row is None else row
        _lib.check(
            _lib.lib().dmme_iddpm_step(_lib.ptr(x_t), _lib.ptr(model_output), _lib.ptr(noise), c[0], c[1], c[2], c[3], int(t != 1), x_t.size(0), x_t[0].numel(), _lib.stream_ptr()),
            "dmme_iddpm_step",
        )
        return x_t

    def forward_model(self, x_t: Tensor, t: Tensor, beta_t: Tensor, alpha_bar_t: Tensor, alpha_bar_t_minus_one: Tensor) -> NoiseVariance:
        """model call + variance interpolation as tensors (reference: diffusion_models/iddpm.py:152-164); API parity only --
        sampling_step / training_step use the fused kernels instead."""
        noise_in_x_t, v = self.model(x_t, t).chunk(2, dim=1)
        beta_tilde_t = (1 - alpha_bar_t_minus_one) / (1 - alpha_bar_t) * beta_t
        return NoiseVariance(noise_in_x_t, interpolate_variance(v, beta_t, beta_tilde_t))
