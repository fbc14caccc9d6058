"""Classifier-free guidance (Ho & Salimans 2021) over the HIP kernels.

One class-conditional network (`models.ConditionalUNet`) is trained with its label replaced by the null label with probability
`p_uncond`; at sampling time its prediction with the label, e_c, and with the null label, e_u, are mixed,

    e^ = e_u + s (e_c - e_u)            s = guidance_scale; s = 1: plain conditional sampling; Ho & Salimans' w = s - 1

and the DDPM or paper-form DDIM update runs on e^.  Both predictions come out of ONE forward at batch 2B (conditional half, then
unconditional half); the update writes its result into both halves.  `generate` replays one captured graph per step
(dmme_cfg_chain_step).  At s == 1 the unconditional half is not computed at all: batch B, the base kind's update.

The guidance scale rides in column 3 of the chain tables, which both base kinds leave free: a per-step schedule of s is a table."""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, gaussian_like, philox_reserve, uniform_int
from ..diffusion_models.ddim import GeneralizedDDIM
from ..diffusion_models.dpm_solver import DPMSolverPP, _row_arg
from ..diffusion_models.chain import ChainRunner, walk
from ..diffusion_models.ddpm import DDPM, _scalar_index
from ..models.cond import ConditionalUNet, class_labels

__all__ = ["ClassifierFreeDDPM", "ClassifierFreeDDIM", "ClassifierFreeDPMSolver", "CFGChainRunner"]

_BASE_KIND = {_lib.CHAIN_DDPM_CFG: _lib.CHAIN_DDPM, _lib.CHAIN_GDDIM_CFG: _lib.CHAIN_GDDIM, _lib.CHAIN_DPMPP_CFG: _lib.CHAIN_DPMPP}


class CFGChainRunner(ChainRunner):
    """ChainRunner over a `ConditionalUNet` with the labels in a static device buffer (`y`).

    guidance_scale != 1: plan, image buffer `x` and `y` are of batch 2B (conditional half, unconditional half) and the captured step
    is dmme_cfg_chain_step.  guidance_scale == 1: batch B, the conditional forward followed by the base kind's update.
    The DPM-Solver++ kinds run their own entry points and carry `hist`, the previous x0 prediction of the B images."""

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        model = process.model
        if not isinstance(model, ConditionalUNet):
            raise TypeError("classifier-free sampling needs a ConditionalUNet")
        if model.training:
            raise RuntimeError("classifier-free sampling runs the network in eval mode")
        self.batched = process.guidance_scale != 1.0
        kind, tables = spec if spec is not None else (process._chain_kind, process._chain_tables())
        if not self.batched:
            kind = _BASE_KIND[kind]
        elif x.shape[0] % 2:
            raise ValueError("CFGChainRunner: the image buffer holds 2B images")
        super().__init__(process, x, use_graph, (kind, tables))
        self.dpmpp = _BASE_KIND.get(kind, kind) == _lib.CHAIN_DPMPP
        self.images = x.shape[0] // 2 if self.batched else x.shape[0]
        self.hist = torch.empty_like(x[:self.images]) if self.dpmpp else None
        self.noise_numel = self.images * x[0].numel()  # the normals of ONE half: what an unguided chain at batch B draws
        self.y = torch.full((x.shape[0],), model.null_label, dtype=torch.int64, device=x.device)
        self.status = model.label_status(x.device)

    def _carried(self):
        return super()._carried() + ([self.hist] if self.dpmpp else [])

    def _call(self, packed):
        lib, plan = _lib.lib(), self.plan
        if self.batched and self.dpmpp:
            _lib.check(
                lib.dmme_cfg_dpmpp_chain_step(plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.y), _lib.ptr(self.out), _lib.ptr(plan.workspace),
                                              _lib.ptr(self.status), _lib.ptr(self.hist), _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state), _lib.stream_ptr()),
                "dmme_cfg_dpmpp_chain_step",
            )
        elif self.batched:
            _lib.check(
                lib.dmme_cfg_chain_step(plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.y), _lib.ptr(self.out), _lib.ptr(plan.workspace),
                                        _lib.ptr(self.status), self.kind, _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state), _lib.stream_ptr()),
                "dmme_cfg_chain_step",
            )
        else:
            t_dev = self.state[1:2]  # the loop state's second word: t
            _lib.check(
                lib.dmme_unet_forward_cond(plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(t_dev), 1, _lib.ptr(self.y), _lib.ptr(self.out),
                                           _lib.ptr(plan.workspace), None, 0, _lib.ptr(self.status), _lib.stream_ptr()),
                "dmme_unet_forward_cond",
            )
            if self.pred != _lib.PRED_EPS:  # (no chain-step entry point on this path: the adapter's launch is made here, where theirs sits)
                _lib.check(
                    lib.dmme_pred_to_eps(self.pred, _lib.ptr(self.out), _lib.ptr(self.x), _lib.ptr(self.pred_ab), self.process.timesteps, _lib.ptr(t_dev), 1,
                                         self.images, self.x[0].numel(), _lib.stream_ptr()),
                    "dmme_pred_to_eps",
                )
            if self.thr != _lib.THRESHOLD_NONE:  # (... and so is the thresholding stage's)
                _lib.check(
                    lib.dmme_x0_threshold(self.thr, _lib.ptr(self.out), _lib.ptr(self.x), _lib.ptr(self.thr_tab), self.process.timesteps, _lib.ptr(t_dev), 1,
                                          self.images, self.x[0].numel(), 1, 1, 1.0, self.thr_k, self.thr_frac, _lib.ptr(self.thr_scratch), _lib.stream_ptr()),
                    "dmme_x0_threshold",
                )
            if self.dpmpp:
                _lib.check(
                    lib.dmme_chain_update_dpmpp(_lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.hist), _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state),
                                                self.images, self.x[0].numel(), 1, _lib.stream_ptr()),
                    "dmme_chain_update_dpmpp",
                )
            else:
                _lib.check(
                    lib.dmme_chain_update(self.kind, _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state),
                                          self.images, self.x[0].numel(), _lib.stream_ptr()),
                    "dmme_chain_update",
                )


class _ClassifierFree:
    """shared parts of the three classifier-free samplers (the chain tables and the eager updates come from the sampler)"""

    guidance_scale: float
    p_uncond: float
    _runner_class = CFGChainRunner

    def _init_cfg(self, guidance_scale: float, p_uncond: float):
        if not isinstance(self.model, ConditionalUNet):
            raise TypeError("classifier-free guidance needs a ConditionalUNet (models.ConditionalUNet)")
        p = float(p_uncond)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p_uncond must lie in [0, 1], got {p}")
        self.set_guidance_scale(guidance_scale)
        self.p_uncond = p

    def set_guidance_scale(self, guidance_scale: float):
        """another s for the chains that follow (a cached runner is keyed by it: the next `generate` builds tables with the new column)"""
        self.guidance_scale = float(np.float32(guidance_scale))  # (what the fp32 tables carry)
        return self

    def _with_scale(self, tables):
        n, rows, ttab = tables
        return n, [(r[0], r[1], r[2], self.guidance_scale) for r in rows], ttab

    def _replayable(self, x: Tensor) -> bool:
        return True  # (what the step cannot run on is refused where the runner is built)

    def _runner_key(self, x: Tensor, use_graph: bool):
        return super()._runner_key(x, use_graph) + (self.guidance_scale,)

    # ------------------------------------------------------------------ training
    def drop_labels(self, y: Tensor) -> Tensor:
        """y with each label replaced by the null label with probability p_uncond, drawn on the device (dmme_label_dropout)"""
        model = self.model
        B, dev = y.numel(), y.device
        out = torch.empty_like(y)
        seed, off = philox_reserve(dev, B)
        _lib.check(_lib.lib().dmme_label_dropout(_lib.ptr(y), B, model.num_classes, self.p_uncond, (seed ^ 0x5DEECE66D) & 0xFFFFFFFFFFFFFFFF, off, _lib.ptr(out),
                                                 _lib.ptr(model.label_status(dev)), _lib.stream_ptr()), "dmme_label_dropout")
        return out

    def training_step(self, x_0: Tensor, y, t: Optional[Tensor] = None, noise: Optional[Tensor] = None, drop: Optional[Tensor] = None) -> Tensor:
        r"""L_simple of eps_theta(x_t, t, y') with y' = null where the label is dropped (Ho & Salimans 2021, Algorithm 1).

        `t` / `noise` / `drop` (bool per image: True drops) may be injected for tests.  Labels given on the host are range-checked
        there; labels already on the device are checked by the kernels (`model.check_labels()` reads their status word)."""
        model = self.model
        B, dev, K = x_0.size(0), x_0.device, model.num_classes
        if isinstance(y, Tensor) and y.is_cuda:
            labels = y.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
            if labels.numel() != B:
                raise ValueError(f"expected {B} labels, got {labels.numel()}")
        else:
            labels = class_labels(y, B, K, dev)
        if t is None:
            t = uniform_int(1, self.timesteps, B, device=dev)
        if noise is None:
            noise = gaussian_like(x_0)
        if drop is not None:
            d = torch.as_tensor(drop).reshape(-1).to(device=dev, dtype=torch.bool)
            labels = torch.where(d, torch.full_like(labels, K), labels)
        elif self.p_uncond > 0.0:
            labels = self.drop_labels(labels)
        _, t, x_t, target = self._noised(x_0, t, noise)
        return self._loss(model(x_t, t, labels, check_labels=False), target, t)

    # ------------------------------------------------------------------ sampling
    def _predict(self, x_t: Tensor, t_dev: Tensor, y) -> Tuple[Tensor, Tensor, int]:
        """(x, eps, B): the image buffer the update runs on (2B images where both halves are needed, else B) and the network output"""
        model = self.model
        if model.training:
            raise RuntimeError("classifier-free sampling runs the network in eval mode")
        B = x_t.shape[0]
        labels = class_labels(y, B, model.num_classes, x_t.device)
        x = x_t.detach().to(torch.float32).contiguous()
        if self.guidance_scale == 1.0:
            x = x.clone()
        else:
            x = torch.cat([x, x], dim=0)
            labels = torch.cat([labels, torch.full_like(labels, model.null_label)])
        batched = self.guidance_scale != 1.0
        with torch.no_grad():
            eps = self._eps(x, t_dev, labels, check_labels=False, _threshold=not batched).to(torch.float32).contiguous()
            if batched and self._thr != _lib.THRESHOLD_NONE:  # (both halves: the x0 of the mixed prediction is what gets clipped)
                eps = self._threshold_eps(eps, x[:B], t_dev, halves=2, guidance_scale=self.guidance_scale)
        return x, eps, B

    def _cfg_update(self, x: Tensor, eps: Tensor, B: int, row, add_noise: bool, z: Optional[Tensor]) -> Tensor:
        _lib.check(_lib.lib().dmme_cfg_step(self._chain_kind, _lib.ptr(x), _lib.ptr(eps), _lib.ptr(z), row[0], row[1], row[2], self.guidance_scale, int(add_noise), B,
                                            x[0].numel(), _lib.stream_ptr()), "dmme_cfg_step")
        return x[:B]

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], y, history=None) -> Tensor:
        """the guided chain from pure noise (`chain_length()` steps), one captured graph per step; `history`: a HistoryRecorder for its frames"""
        dev, n_steps = self.beta.device, self.chain_length()
        model = self.model
        B = int(img_size[0])
        labels = class_labels(y, B, model.num_classes, dev)
        x_t = gaussian(img_size, device=dev)
        batched = self.guidance_scale != 1.0
        shape = ((2 * B) if batched else B,) + tuple(img_size[1:])
        runner = self._buffered_runner("_cfg_runner", shape, dev, buf="_cfg_buf")
        runner.x[:B].copy_(x_t)
        runner.y[:B].copy_(labels)
        if batched:
            runner.x[B:].copy_(x_t)
            runner.y[B:].fill_(model.null_label)
        out = runner.run(n_steps, n_steps, history)[:B].clone()  # (a recorder keeps the first B images of the 2B the buffer holds)
        model.check_labels()
        return out

    def forward(self, x: Tensor, t: Tensor, y) -> Tensor:
        """the raw network output (eps, x0 or v, as `prediction` says), not converted"""
        return self.model(x, t, y)


def _needs_labels(name: str):
    def refuse(self, *a, **kw):
        raise NotImplementedError(f"{type(self).__name__}.{name} has no labelled form: use sampling_step(x, i, y) / generate(img_size, y)")

    refuse.__name__ = name
    return refuse


class ClassifierFreeDDPM(_ClassifierFree, DDPM):
    """DDPM training and sampling with classifier-free guidance: x_{t-1} = mu(x_t, e^) + sqrt(beta_t) z (no noise at t = 1); `generate`
    runs the T-step chain."""

    _chain_kind = _lib.CHAIN_DDPM_CFG

    def __init__(self, model: nn.Module, timesteps: int = 1000, guidance_scale: float = 1.0, p_uncond: float = 0.1, start: float = 0.0001, end: float = 0.02, *,
                 prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, start, end, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        self._init_cfg(guidance_scale, p_uncond)

    def _chain_tables(self):
        return self._with_scale(super()._chain_tables())

    def sampling_step(self, x_t: Tensor, t: Tensor, y, noise: Optional[Tensor] = None) -> Tensor:
        """one guided draw from p(x_{t-1} | x_t, y); t has shape (1,)"""
        step = _scalar_index(t, "a timestep")
        x, eps, B = self._predict(x_t, self.timestep_tensor(step, x_t.device), y)
        if self.guidance_scale == 1.0:
            return self._reverse_update(x, eps, step, noise)
        z = gaussian_like(x_t) if noise is None else noise.detach().to(device=x.device, dtype=torch.float32).contiguous()  # (drawn at t == 1 too, unused)
        return self._cfg_update(x, eps, B, (self._c1[step], self._c2[step], self._sigma[step]), step != 1, z)

    denoise_once = _needs_labels("denoise_once")


class ClassifierFreeDDIM(_ClassifierFree, GeneralizedDDIM):
    """Paper-form DDIM (Song et al. 2021, eq. 12, any eta) with classifier-free guidance: x' = (k0 x + k1 e^) + k2 z; `generate` runs
    the S-step strided chain."""

    _chain_kind = _lib.CHAIN_GDDIM_CFG

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 50, tau_schedule: str = "quadratic", eta: float = 0.0,
                 guidance_scale: float = 1.0, p_uncond: float = 0.1, *, prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, sub_timesteps, tau_schedule, eta, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        self._init_cfg(guidance_scale, p_uncond)

    def _chain_tables(self):
        return self._with_scale(super()._chain_tables())

    def sampling_step(self, x_tau_i: Tensor, i: Tensor, y, noise: Optional[Tensor] = None) -> Tensor:
        r"""x_{tau_{i-1}} from x_{tau_i} with guidance; i has shape (1,); `noise` replaces the drawn normals"""
        idx = self._index(_scalar_index(i, "an index"), "sampling_step")
        x, eps, B = self._predict(x_tau_i, self.tau[idx].reshape(1), y)
        row = self._rev_rows[idx]
        if self.guidance_scale == 1.0:
            return self._gddim_update(x, eps, row, noise, self._draws)
        if noise is None and self._draws:  # a chain that draws takes its span at every step, whether or not k2 uses it
            noise = gaussian_like(x_tau_i)
        z = None if noise is None else noise.detach().to(device=x.device, dtype=torch.float32).contiguous()
        if z is None and row[2] != 0.0:
            raise ValueError("a step with k2 != 0 needs noise")
        return self._cfg_update(x, eps, B, row, row[2] != 0.0, z)

    denoise_once, encode, decode, interpolate = (_needs_labels(n) for n in ("denoise_once", "encode", "decode", "interpolate"))


class ClassifierFreeDPMSolver(_ClassifierFree, DPMSolverPP):
    """DPM-Solver++(2M) with classifier-free guidance: the solver's update on e^ = e_u + s (e_c - e_u); the history holds B images;
    `generate` runs the n_steps chain."""

    _chain_kind = _lib.CHAIN_DPMPP_CFG

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 20, tau_schedule: str = "logsnr", order: int = 2, clip_x0: bool = False,
                 alpha_bar: Optional[Tensor] = None, guidance_scale: float = 1.0, p_uncond: float = 0.1, *, prediction: str = "eps", loss_weight: str = "uniform",
                 snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, sub_timesteps, tau_schedule, order, clip_x0, alpha_bar, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        self._init_cfg(guidance_scale, p_uncond)

    def _scaled_rows(self):
        """the rows with the guidance scale in column 6, rebuilt only when the scale changed"""
        if getattr(self, "_rows_scale", None) != self.guidance_scale:
            self._rows_s, self._rows_scale = self._make_rows(self.guidance_scale), self.guidance_scale
        return self._rows_s

    def _chain_tables(self):
        return self.n_steps, list(self._scaled_rows()), list(self._tau_host)

    def _guided_update(self, x: Tensor, eps: Tensor, B: int, i: int, hist: Tensor, valid: bool) -> Tensor:
        """in place on x (2B images where s != 1, else B) and hist (B images); returns the B images"""
        if self.guidance_scale == 1.0:
            return self._dpm_update(x, eps, i, hist, valid)
        _lib.check(_lib.lib().dmme_cfg_dpmpp_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(hist), _row_arg(self._scaled_rows()[i]), int(valid), B,
                                                  x[0].numel(), _lib.stream_ptr()), "dmme_cfg_dpmpp_step")
        return x[:B]

    def sampling_step(self, x_tau_i: Tensor, i: Tensor, y, history: Optional[Tensor] = None, history_valid: bool = False) -> Tensor:
        r"""x_{tau_{i-1}} from x_{tau_i} with guidance; i has shape (1,); `history` / `history_valid` as in `DPMSolverPP.sampling_step` (B images)"""
        idx = self._index(_scalar_index(i, "an index"), "sampling_step")
        valid = self._history_valid(history, history_valid)
        x, eps, B = self._predict(x_tau_i, self.tau[idx].reshape(1), y)
        return self._guided_update(x, eps, B, idx, self._history(x[:B], history), valid)

    denoise_once, decode = (_needs_labels(n) for n in ("denoise_once", "decode"))

    def _eager_generate(self, x_T: Tensor, y) -> Tensor:
        """the host loop over the eager twins, bit-identical to the captured chain of `generate`"""
        x, hist = x_T.clone(), torch.empty_like(x_T)

        def step(k, i):
            xb, eps, B = self._predict(x, self.tau_tensor(i, x.device), y)
            x.copy_(self._guided_update(xb, eps, B, i, hist, k > 0))

        return walk(x, self.n_steps, self.n_steps, step)
