"""Classifier guidance over the HIP kernels.

The reference ships classifier guidance as an unfinished sketch (src/dmme/guidance/classifier.py, tests/test_guidance.py):
`ClassifierGuidedDDPM` / `ClassifierGuidedDDIM` import modules that do not exist.  This module keeps its class names and follows
the method the sketch reaches for, Dhariwal & Nichol 2021 ("Diffusion Models Beat GANs"), Algorithm 1 (DDPM) and Algorithm 2 (DDIM),
with two deliberate deviations from the sketch:

- the gradient is d sum_i log p(y_i | x_i, t) / d x, row by row: the sketch's `log_probs[:, y]` builds a B x B matrix and mixes
  every image's label into every image's gradient;
- the DDPM step takes the gradient at x_t, before the step (Algorithm 1); the sketch takes it at x_{t-1}, after the step.

Pieces:
- `EncoderClassifier`: the noise-aware classifier (the ADM "half UNet"): the DDPM UNet's time MLP, input_conv, down_layers and
  middle_layers (same state_dict keys and layouts: encoder weights copy over from a `UNet`), then the head `out` = GroupNorm ->
  SiLU -> mean over H x W -> Linear(C_top, num_classes).  A DMME_ARCH_CLASSIFIER plan in the library.
- `classifier_loss`: cross-entropy of the classifier on x_0 noised at t ~ uniform_int(1, T), with a HIP backward.
- `ClassifierGuidedDDPM` / `ClassifierGuidedDDIM`: `sampling_step(x_t, t, y)` and `generate(img_size, y)`; `generate` replays
  one captured graph per step (UNet forward, classifier forward, log-softmax gradient, input-only backward, guided update).
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, gaussian_like, philox_reserve, uniform_int
from ..diffusion_models.ddim import DDIM
from ..diffusion_models.chain import ChainRunner, ChainTables
from ..diffusion_models.ddpm import DDPM, _scalar_index
from ..models.cond import class_labels
from ..models.ddpm import UNet

__all__ = ["EncoderClassifier", "ClassifierGuidedDDPM", "ClassifierGuidedDDIM", "GuidedChainRunner", "classifier_loss", "cross_entropy_apply",
           "ClassifierFreeDDPM", "ClassifierFreeDDIM", "ClassifierFreeDPMSolver", "CFGChainRunner"]


from .cfg import CFGChainRunner, ClassifierFreeDDIM, ClassifierFreeDDPM, ClassifierFreeDPMSolver  # noqa: E402,F401  (classifier-free guidance: no classifier at all)


def _labels(y, B: int, K: int, device) -> Tensor:
    """int64 device labels of shape (B,), refused (ValueError) when outside [0, K)"""
    return class_labels(y, B, K, device, null=False)


def _check_status(status: Tensor, what: str):
    if int(status.item()) != 0:
        raise ValueError(f"{what}: a class label outside [0, num_classes) reached the device (its rows are NaN)")


def _check_precision(precision: str):
    if _lib.dtype_code(precision) not in (_lib.F32, _lib.BF16, _lib.F16):
        raise _lib.DmmeError(f"EncoderClassifier runs in fp32, bf16 or fp16, not {precision!r} (the library refuses it: DMME_ERR_UNSUPPORTED)")


class EncoderClassifier(UNet):
    r"""Noise-aware classifier p(y | x_t, t): the encoder half of the DDPM UNet plus a pooled linear head.

    Constructor arguments are `UNet`'s plus `num_classes`; `dropout` defaults to 0.  `forward(x, t)` returns fp32 logits of shape
    (B, num_classes).  Precision "fp32", "bf16" or "fp16" ("bf16x3" / "fp16r32" raise DmmeError when a plan is built)."""

    def __init__(
        self,
        in_channels: int = 3,
        pos_dim: int = 128,
        emb_dim: int = 512,
        num_groups: int = 32,
        dropout: float = 0.0,
        channels_per_depth: Sequence[int] = (128, 256, 256, 256),
        num_blocks: int = 2,
        attention_depths: Sequence[int] = (2,),
        precision: str = "fp32",
        num_classes: int = 10,
    ):
        if int(num_classes) < 1:
            raise ValueError("num_classes must be >= 1")
        _check_precision(precision)
        super().__init__(in_channels, pos_dim, emb_dim, num_groups, dropout, channels_per_depth, num_blocks, attention_depths, precision,
                         _arch=_lib.ARCH_CLASSIFIER, _num_classes=int(num_classes))
        self.num_classes = int(num_classes)
        self.out_channels = self.num_classes

    def _out_shape(self, B: int, H: int, W: int) -> Tuple[int, ...]:
        return (B, self.num_classes)

    def set_precision(self, precision: str):
        _check_precision(precision)
        return super().set_precision(precision)

    def input_grad(self, x: Tensor, t: Tensor, y, scale: float = 1.0) -> Tensor:
        """scale * d sum_i log p(y_i | x_i, t) / d x (fp32, shape of x), through the input-only backward: the parameters' gradient
        buffer is left untouched and no weight gradient is computed"""
        B = x.shape[0]
        labels = _labels(y, B, self.num_classes, x.device)
        logits, saved = self._forward_impl(x, t, want_ctx=True)
        dlog = torch.empty_like(logits)
        status = torch.zeros(1, dtype=torch.int32, device=x.device)
        _lib.check(_lib.lib().dmme_log_softmax_grad(_lib.ptr(logits), _lib.ptr(labels), B, self.num_classes, 1, float(scale), None, _lib.ptr(dlog),
                                                    _lib.ptr(status), _lib.stream_ptr()), "dmme_log_softmax_grad")
        dx = self._backward_input_impl(saved, dlog)
        _check_status(status, "EncoderClassifier.input_grad")
        return dx


class _CrossEntropyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: Tensor, labels: Tensor):
        lg = logits.detach().to(torch.float32).contiguous()
        B, K = lg.shape
        loss = torch.empty(1, dtype=torch.float32, device=lg.device)
        d = torch.empty_like(lg) if logits.requires_grad else None
        # (labels were range-checked on the host by cross_entropy_apply: no status word needed)
        _lib.check(_lib.lib().dmme_log_softmax_grad(_lib.ptr(lg), _lib.ptr(labels), B, K, 0, 1.0, _lib.ptr(loss), _lib.ptr(d), None, _lib.stream_ptr()),
                   "dmme_log_softmax_grad")
        ctx.d = d
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        d = ctx.d
        ctx.d = None
        return (d * grad_out if d is not None else None), None


def cross_entropy_apply(logits: Tensor, y) -> Tensor:
    """mean_i -log softmax(logits_i)[y_i] (F.cross_entropy) with the HIP log-softmax kernel"""
    labels = _labels(y, logits.shape[0], logits.shape[1], logits.device)
    return _CrossEntropyFunction.apply(logits, labels)


def classifier_loss(classifier: EncoderClassifier, diffusion: DDPM, x_0: Tensor, y, t: Optional[Tensor] = None, noise: Optional[Tensor] = None) -> Tensor:
    """Cross-entropy of the noise-aware classifier on x_t = q_sample(x_0, t, noise), t ~ uniform_int(1, T) per image by default
    (as DDPM.training_step draws it); `t` / `noise` may be injected.  The backward runs through HIP into the classifier's flat
    gradient buffer (works with optim.FusedAdam)."""
    if t is None:
        t = uniform_int(1, diffusion.timesteps, x_0.size(0), device=x_0.device)
    if noise is None:
        noise = gaussian_like(x_0)
    _, t, x_t, _ = diffusion._noised(x_0, t, noise, target=False)
    return cross_entropy_apply(classifier(x_t, t), y)


class GuidedChainRunner(ChainRunner):
    """ChainRunner whose captured step is dmme_guided_chain_step: UNet forward, classifier forward, log-softmax gradient,
    input-only backward and the guided update, with the labels in a static device buffer (`y`)."""

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        cls = process.classifier
        if process.model.training or cls.training:
            raise RuntimeError("guided sampling runs the UNet and the classifier in eval mode")
        super().__init__(process, x, use_graph, spec)
        B, _, H, W = x.shape
        self.cls = cls
        self.cls_plan = cls._plan_for(B, H, W, x.device)
        self.y = torch.zeros(B, dtype=torch.int64, device=x.device)
        self.logits = torch.empty((B, cls.num_classes), dtype=torch.float32, device=x.device)
        self.dlog = torch.empty_like(self.logits)
        self.grad = torch.empty_like(x)
        self.status = torch.zeros(1, dtype=torch.int32, device=x.device)

    def _weights_key(self):
        cp = self.cls_plan
        return super()._weights_key() + (getattr(cp, "packed_version", None), getattr(cp, "packed_bwd_version", None))

    def _call(self, packed):
        if self.cls.training:
            raise RuntimeError("guided sampling runs the classifier in eval mode")
        cp = self.cls_plan
        cls_packed = self.cls._bwd_buffers(cp)
        _lib.check(
            _lib.lib().dmme_guided_chain_step(self.plan.h, _lib.ptr(packed), cp.h, _lib.ptr(cls_packed), _lib.ptr(cp.packed_bwd), _lib.ptr(self.x),
                                              _lib.ptr(self.out), _lib.ptr(self.plan.workspace), _lib.ptr(cp.workspace), _lib.ptr(cp.bws), _lib.ptr(self.y),
                                              _lib.ptr(self.logits), _lib.ptr(self.dlog), _lib.ptr(self.grad), _lib.ptr(self.status), self.kind,
                                              _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state), _lib.stream_ptr()),
            "dmme_guided_chain_step",
        )
        cp.overwritten()  # (the UNet's plan is `_launch`'s; it alone is told the prediction: the classifier's predicts no noise)

    def step(self):
        self.cls._bwd_buffers(self.cls_plan)  # (re-packs outside any capture when the classifier's parameters changed)
        return super().step()


class _Guided:
    """shared parts of the two guided samplers (`_n_steps`, `_index_t` and the chain tables come from the sampler)"""

    classifier: EncoderClassifier
    guidance_scale: float

    _runner_class = GuidedChainRunner

    def _replayable(self, x: Tensor) -> bool:
        return True  # (there is no eager chain to fall back to: what the step cannot run on is refused where the runner is built)

    def _runner_key(self, x: Tensor, use_graph: bool):
        return super()._runner_key(x, use_graph) + (self.classifier, self.classifier._dtype, self.guidance_scale)

    def _guided_runner(self, img_size, dev) -> GuidedChainRunner:
        return self._buffered_runner("_grunner", img_size, dev, buf="_gbuf")

    def _eager_update(self, x: Tensor, eps: Tensor, g: Tensor, index: int, noise: Optional[Tensor]) -> Tensor:
        dev = x.device
        tabs = getattr(self, "_gtabs", None)
        if tabs is None or tabs.key != (dev, self.guidance_scale):
            _, rows, ttab = self._chain_tables()
            tabs = self._gtabs = ChainTables(rows, ttab, dev)
            tabs.key = (dev, self.guidance_scale)
        if self._chain_kind == _lib.CHAIN_DDIM_GUIDED or noise is not None:
            seed, off = 0, 0
        else:
            seed, off = philox_reserve(dev, x.numel())  # (drawn even at t == 1, then unused: the reference's order)
        z = None if noise is None else noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        tabs.set(index, seed, off)
        _lib.check(_lib.lib().dmme_chain_update_guided(self._chain_kind, _lib.ptr(x), _lib.ptr(eps), _lib.ptr(g), _lib.ptr(z), _lib.ptr(tabs.coef), _lib.ptr(tabs.ttab),
                                                       _lib.ptr(tabs.state), x.shape[0], x[0].numel(), _lib.stream_ptr()), "dmme_chain_update_guided")
        return x

    def _guided_step(self, x_t: Tensor, index: int, t_dev: Tensor, y, noise: Optional[Tensor]) -> Tensor:
        with torch.no_grad():
            eps = self._eps(x_t, t_dev).to(torch.float32).contiguous()
            g = self.classifier.input_grad(x_t, t_dev, y)
        x = x_t.detach().to(torch.float32).clone().contiguous()
        return self._eager_update(x, eps, g, index, noise)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], y, history=None) -> Tensor:
        """the guided chain from pure noise (`chain_length()` steps), one captured graph per step; `history`: a HistoryRecorder for its frames"""
        dev, n_steps = self.beta.device, self.chain_length()
        x_t = gaussian(img_size, device=dev)
        labels = _labels(y, img_size[0], self.classifier.num_classes, dev)
        runner = self._guided_runner(img_size, dev)
        runner.x.copy_(x_t)
        runner.y.copy_(labels)
        runner.status.zero_()
        out = runner.run(n_steps, n_steps, history).clone()
        _check_status(runner.status, "generate")
        return out


class ClassifierGuidedDDPM(_Guided, DDPM):
    """DDPM sampling with classifier guidance (Dhariwal & Nichol 2021, Algorithm 1):
    x_{t-1} = mu(x_t, t) + s beta_t grad_x log p(y | x_t, t) + sqrt(beta_t) z  (no noise at t = 1; the mean shift stays); `generate` runs
    the T-step chain."""

    _chain_kind = _lib.CHAIN_DDPM_GUIDED

    def __init__(self, model: nn.Module, classifier: EncoderClassifier, timesteps: int = 1000, guidance_scale: float = 1.0, start: float = 0.0001,
                 end: float = 0.02, *, prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, start, end, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        self.classifier = classifier
        self.guidance_scale = float(guidance_scale)

    def _chain_tables(self):
        T, rows, ttab = super()._chain_tables()
        sb = (torch.tensor(self.guidance_scale, dtype=torch.float32) * self.beta.reshape(-1).to(torch.float32).cpu()).tolist()  # fp32 s * beta_t
        return T, [(r[0], r[1], r[2], sb[t]) for t, r in enumerate(rows)], ttab

    def sampling_step(self, x_t: Tensor, t: Tensor, y, noise: Optional[Tensor] = None) -> Tensor:
        """one guided draw from p(x_{t-1} | x_t, y); t has shape (1,)"""
        step = _scalar_index(t, "a timestep")
        return self._guided_step(x_t, step, self.timestep_tensor(step, x_t.device), y, noise)


class ClassifierGuidedDDIM(_Guided, DDIM):
    """DDIM sampling with classifier guidance (Dhariwal & Nichol 2021, Algorithm 2):
    eps' = eps - s sqrt(1 - abar_tau_i) grad_x log p(y | x_tau_i, tau_i), then the DDIM update with eps'; `generate` runs the S-step
    strided chain."""

    _chain_kind = _lib.CHAIN_DDIM_GUIDED

    def __init__(self, model: nn.Module, classifier: EncoderClassifier, timesteps: int = 1000, sub_timesteps: int = 50, tau_schedule: str = "quadratic",
                 guidance_scale: float = 1.0, *, prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, sub_timesteps, tau_schedule, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        self.classifier = classifier
        self.guidance_scale = float(guidance_scale)

    def _chain_tables(self):
        S, rows, ttab = super()._chain_tables()
        s = torch.tensor(self.guidance_scale, dtype=torch.float32)
        return S, [(r[0], r[1], float(s * torch.tensor(r[0], dtype=torch.float32)), 0.0) for r in rows], ttab

    def sampling_step(self, x_tau_i: Tensor, i: Tensor, y) -> Tensor:
        """x_{tau_{i-1}} from x_{tau_i} with guidance; i has shape (1,)"""
        idx = _scalar_index(i, "an index")
        return self._guided_step(x_tau_i, idx, self.tau_tensor(idx, x_tau_i.device), y, None)
