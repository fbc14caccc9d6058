"""Class-conditional UNet eps_theta(x_t, t, y) for classifier-free guidance (Ho & Salimans 2021).

The DDPM UNet plus one parameter: `label_emb.weight` of shape (num_classes + 1, emb_dim), appended behind the 305 entries of `UNet`,
so an unconditional state_dict is a prefix of a conditional one.  Row `num_classes` is the null label.  The label row enters the
time embedding in the ADM form (Dhariwal & Nichol 2021): c_b = SiLU(W2 h1 + b2 + E[y_b]).  A DMME_ARCH_DDPM_COND plan in the library
(include/dmme_hip.h); fp32, bf16 and fp16."""

from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from .. import _lib
from .ddpm import UNet, _Plan


def _check_precision(precision: str):
    if _lib.dtype_code(precision) not in (_lib.F32, _lib.BF16, _lib.F16):
        raise _lib.DmmeError(f"ConditionalUNet runs in fp32, bf16 or fp16, not {precision!r} (the library refuses it: DMME_ERR_UNSUPPORTED)")


def class_labels(y, B: int, K: int, device, null: bool = True) -> Tensor:
    """int64 device labels of shape (B,), refused (ValueError) when outside [0, K] (null: K is the null label of a conditional network)
    or outside [0, K) (a classifier's classes).  The one host-side label check of the package (guidance._labels is its [0, K) form)."""
    y = torch.as_tensor(y).reshape(-1).to(torch.int64)
    if y.numel() != B:
        raise ValueError(f"expected {B} labels, got {y.numel()}")
    lo, hi = int(y.min().item()), int(y.max().item())  # (where the labels live: host labels cost no device synchronisation)
    if lo < 0 or hi > K or (hi == K and not null):
        rng = f"[0, {K}] ({K} is the null label)" if null else f"[0, {K})"
        raise ValueError(f"class labels must lie in {rng}; got values in [{lo}, {hi}]")
    return y.to(device=device).contiguous()


class ConditionalUNet(UNet):
    r"""`UNet` with a class label: constructor arguments are `UNet`'s plus `num_classes`, `forward(x, c, y)` takes int64 labels in
    [0, num_classes]; `null_label == num_classes` stands for "no class".  `label_emb.weight` is initialised N(0, 1) (nn.Embedding)."""

    def __init__(
        self,
        in_channels: int = 3,
        pos_dim: int = 128,
        emb_dim: int = 512,
        num_groups: int = 32,
        dropout: float = 0.1,
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
                         _arch=_lib.ARCH_DDPM_COND, _num_classes=int(num_classes))
        self.num_classes = int(num_classes)
        with torch.no_grad():
            nn.init.normal_(self.label_emb.weight)
        self._labels: Optional[Tensor] = None  # the labels of the forward being launched
        self._status: Optional[Tensor] = None

    @property
    def null_label(self) -> int:
        return self.num_classes

    def set_precision(self, precision: str):
        _check_precision(precision)
        return super().set_precision(precision)

    def label_status(self, device) -> Tensor:
        """device int32[1] the kernels set when a label outside [0, num_classes] reaches them (that image's output is NaN)"""
        st = self._status
        if st is None or st.device != torch.device(device):
            st = self._status = torch.zeros(1, dtype=torch.int32, device=device)
        return st

    def check_labels(self):
        """synchronise and raise ValueError if a label outside [0, num_classes] reached the device since the last check"""
        st = self._status
        if st is not None and int(st.item()) != 0:
            st.zero_()
            raise ValueError("ConditionalUNet: a class label outside [0, num_classes] reached the device (its images are NaN)")

    def forward(self, x: Tensor, c: Tensor, y, check_labels: bool = True) -> Tensor:
        r"""eps_theta(x, c, y).  x: (N, C, H, W) on an MI355X; c: timesteps of shape (N,) or (1,); y: N labels in [0, num_classes].
        `check_labels=False` skips the host-side range check (one read-back) for labels produced on the device; the kernels still
        never index the table with them unclamped and raise `label_status`."""
        if not isinstance(x, Tensor) or not x.is_cuda:
            raise _lib.DmmeError("ConditionalUNet.forward needs a GPU tensor: the HIP denoiser has no CPU fallback")
        B = x.shape[0]
        if check_labels:
            labels = class_labels(y, B, self.num_classes, x.device)
        else:
            labels = y.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
            if labels.numel() != B:
                raise ValueError(f"expected {B} labels, got {labels.numel()}")
        self._labels = labels
        try:
            return super().forward(x, c)
        finally:
            self._labels = None

    def input_grad(self, x: Tensor, c: Tensor, y, d_out: Tensor) -> Tensor:
        """d_out . d eps_theta(x, c, y) / d x (fp32, shape of x) through the input-only backward (dmme_unet_backward_input_cond): no
        weight gradient is computed and the parameters' gradient buffer is left untouched.  c of shape (1,) is accepted."""
        self._labels = class_labels(y, x.shape[0], self.num_classes, x.device)
        try:
            _, saved = self._forward_impl(x, c, want_ctx=True)
        finally:
            self._labels = None
        return self._backward_input_impl(saved, d_out)

    def graphed_forward(self, x_static: Tensor, t_static: Tensor) -> Tensor:
        raise _lib.DmmeError("ConditionalUNet has no label-less graphed forward: sample through guidance.ClassifierFreeDDPM / ClassifierFreeDDIM")

    # ------------------------------------------------------------------ the launches, with labels
    def _launch_forward(self, plan: _Plan, packed, xin, t, y, masks, want_ctx):
        labels = self._labels
        if labels is None:
            raise _lib.DmmeError("ConditionalUNet: a forward without labels (call the module as model(x, c, y))")
        plan.labels = labels  # (what a backward on this plan's workspace differentiates; guarded by the plan's generation stamp)
        _lib.check(
            plan.lib.dmme_unet_forward_cond(plan.h, _lib.ptr(packed), _lib.ptr(xin), _lib.ptr(t), int(t.numel()), _lib.ptr(labels), _lib.ptr(y),
                                            _lib.ptr(plan.workspace), _lib.ptr(masks), int(want_ctx), _lib.ptr(self.label_status(xin.device)), _lib.stream_ptr()),
            "dmme_unet_forward_cond",
        )

    def _launch_backward(self, plan: _Plan, packed, xin, t, d, masks, g, dx, cb):
        _lib.check(
            plan.lib.dmme_unet_backward_cond(plan.h, _lib.ptr(packed), _lib.ptr(plan.packed_bwd), _lib.ptr(xin), _lib.ptr(t), int(t.numel()), _lib.ptr(plan.labels),
                                             _lib.ptr(d), _lib.ptr(plan.workspace), _lib.ptr(plan.bws), _lib.ptr(masks), _lib.ptr(g), _lib.ptr(dx), _lib.stream_ptr(),
                                             cb if cb is not None else _lib.BUCKET_FN(0), None),
            "dmme_unet_backward_cond",
        )

    def _launch_backward_input(self, plan: _Plan, packed, xin, t, d, masks, dx):
        _lib.check(
            plan.lib.dmme_unet_backward_input_cond(plan.h, _lib.ptr(packed), _lib.ptr(plan.packed_bwd), _lib.ptr(xin), _lib.ptr(t), int(t.numel()),
                                                   _lib.ptr(plan.labels), _lib.ptr(d), _lib.ptr(plan.workspace), _lib.ptr(plan.bws), _lib.ptr(masks), _lib.ptr(dx),
                                                   _lib.stream_ptr()),
            "dmme_unet_backward_input_cond",
        )
