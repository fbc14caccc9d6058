"""Autograd glue for the training path: torch.autograd only sees two opaque nodes (the UNet
and the MSE loss); everything inside them is HIP (dmme_unet_forward / dmme_unet_backward /
dmme_mse_loss).  Parameter gradients are accumulated by the library straight into the
model's flat fp32 gradient buffer (every `param.grad` is a view of it)."""

from __future__ import annotations

import torch
from torch import Tensor

from . import _lib


class _UNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, anchor: Tensor, model, c: Tensor):
        y, saved = model._forward_impl(x, c, want_ctx=True)
        ctx.model = model
        ctx.saved = saved
        ctx.want_dx = bool(x.requires_grad)
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        # parameter gradients: accumulated by the library into model.flat_grad() (param.grad views); the gradient with respect
        # to the input image (guidance, sensitivity tests) is returned to autograd when x required it
        dx = ctx.model._backward_impl(ctx.saved, dy, want_dx=ctx.want_dx)
        ctx.saved = None
        return (dx.to(ctx.x_dtype) if dx is not None else None), None, None, None


def unet_apply(model, x: Tensor, c: Tensor) -> Tensor:
    """eps = UNet(x, c) with a HIP backward; `anchor` only ties the node into the graph."""
    anchor = next(p for p in model.parameters() if p.requires_grad)
    return _UNetFunction.apply(x, anchor, model, c)


class _MSEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eps: Tensor, target: Tensor):
        e = eps.detach().to(torch.float32).contiguous()
        tg = target.detach().to(torch.float32).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=e.device)
        scratch = torch.empty(1024, dtype=torch.float32, device=e.device)
        d_eps = torch.empty_like(e) if eps.requires_grad else None
        _lib.check(_lib.lib().dmme_mse_loss(_lib.ptr(e), _lib.ptr(tg), e.numel(), _lib.ptr(loss), _lib.ptr(d_eps), 1.0, _lib.ptr(scratch), _lib.stream_ptr()), "dmme_mse_loss")
        ctx.d_eps = d_eps
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        d = ctx.d_eps
        ctx.d_eps = None
        return (d * grad_out if d is not None else None), None


def mse_loss_apply(eps: Tensor, target: Tensor) -> Tensor:
    """simple_loss (reference: equations/ddpm/losses.py:5-13): mean((target - eps)^2) over all elements."""
    return _MSEFunction.apply(eps, target)


class _WeightedMSEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out: Tensor, target: Tensor, w_table: Tensor, t: Tensor):
        o = out.detach().to(torch.float32).contiguous()
        tg = target.detach().to(torch.float32).contiguous()
        B = o.size(0)
        loss = torch.empty(1, dtype=torch.float32, device=o.device)
        scratch = torch.empty(64 * B, dtype=torch.float32, device=o.device)
        d_out = torch.empty_like(o) if out.requires_grad else None
        _lib.check(_lib.lib().dmme_mse_loss_rows(_lib.ptr(o), _lib.ptr(tg), _lib.ptr(w_table), _lib.ptr(t), B, o[0].numel(), _lib.ptr(loss), _lib.ptr(d_out), 1.0,
                                                 _lib.ptr(scratch), _lib.stream_ptr()), "dmme_mse_loss_rows")
        ctx.d_out = d_out
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        d = ctx.d_out
        ctx.d_out = None
        return (d * grad_out if d is not None else None), None, None, None


def weighted_mse_loss_apply(out: Tensor, target: Tensor, w_table: Tensor, t: Tensor) -> Tensor:
    """mean over all elements of w_table[t_b] (out - target)^2: the MSE with a weight per image's timestep (min-SNR-gamma), with a HIP
    gradient (dmme_mse_loss_rows).  w_table: fp32, indexed by t; t: one timestep per image, each inside the table (checked here only
    for host tensors: a device t is the caller's, as drawn by `training_step`)."""
    dev = out.device
    w = w_table.detach().to(device=dev, dtype=torch.float32).contiguous()
    if t.numel() != out.shape[0] or target.shape != out.shape:
        raise ValueError(f"weighted_mse_loss_apply: output {tuple(out.shape)}, target {tuple(target.shape)}, {t.numel()} timesteps")
    if not t.is_cuda and t.numel() and not (0 <= int(t.min()) and int(t.max()) < w.numel()):
        raise ValueError(f"weighted_mse_loss_apply: a timestep outside the weight table's 0..{w.numel() - 1}")
    return _WeightedMSEFunction.apply(out, target, w, t.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous())


class _IDDPMLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model_out: Tensor, x_t: Tensor, x_0: Tensor, target: Tensor, t: Tensor, coef: Tensor, w_simple: float, w_vlb: float):
        o = model_out.detach().to(torch.float32).contiguous()
        B = o.size(0)
        loss = torch.empty(3, dtype=torch.float32, device=o.device)
        scratch = torch.empty(1024, dtype=torch.float32, device=o.device)
        d_out = torch.empty_like(o) if model_out.requires_grad else None
        _lib.check(
            _lib.lib().dmme_iddpm_loss(_lib.ptr(o), _lib.ptr(x_t), _lib.ptr(x_0), _lib.ptr(target), _lib.ptr(t), _lib.ptr(coef), B, x_t[0].numel(),
                                       w_simple, w_vlb, _lib.ptr(loss), _lib.ptr(d_out), 1.0, _lib.ptr(scratch), _lib.stream_ptr()),
            "dmme_iddpm_loss",
        )
        ctx.d_out = d_out
        ctx.parts = loss
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        d = ctx.d_out
        ctx.d_out = None
        return (d * grad_out if d is not None else None), None, None, None, None, None, None, None


def iddpm_loss_apply(model_out: Tensor, x_t: Tensor, x_0: Tensor, target: Tensor, t: Tensor, coef: Tensor, w_simple: float, w_vlb: float) -> Tensor:
    """w_simple * L_simple + w_vlb * L_vlb (reference: diffusion_models/iddpm.py:92-116, equations/iddpm/losses.py:40-98)."""
    return _IDDPMLossFunction.apply(model_out, x_t, x_0, target, t, coef.to(device=model_out.device, dtype=torch.float32).contiguous(), w_simple, w_vlb)


class _IDDPMLossRowsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model_out: Tensor, x_t: Tensor, x_0: Tensor, target: Tensor, t: Tensor, coef: Tensor, timesteps: int, weight, w_simple: float,
                w_vlb: float, status):
        o = model_out.detach().to(torch.float32).contiguous()
        B = o.size(0)
        loss = torch.empty(3, dtype=torch.float32, device=o.device)
        rows = torch.empty((3, B), dtype=torch.float32, device=o.device)
        scratch = torch.empty(64 * B, dtype=torch.float32, device=o.device)
        d_out = torch.empty_like(o) if model_out.requires_grad else None
        _lib.check(
            _lib.lib().dmme_iddpm_loss_rows(_lib.ptr(o), _lib.ptr(x_t), _lib.ptr(x_0), _lib.ptr(target), _lib.ptr(t), _lib.ptr(coef), int(timesteps),
                                            _lib.ptr(weight), B, x_t[0].numel(), w_simple, w_vlb, _lib.ptr(loss), _lib.ptr(rows), _lib.ptr(d_out), 1.0,
                                            _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr()),
            "dmme_iddpm_loss_rows",
        )
        ctx.d_out = d_out
        ctx.parts = loss
        ctx.mark_non_differentiable(rows)
        return loss[0], rows

    @staticmethod
    def backward(ctx, grad_out: Tensor, _grad_rows):
        d = ctx.d_out
        ctx.d_out = None
        return (d * grad_out if d is not None else None), None, None, None, None, None, None, None, None, None, None


def iddpm_loss_rows_apply(model_out: Tensor, x_t: Tensor, x_0: Tensor, target: Tensor, t: Tensor, coef: Tensor, timesteps: int, weight,
                          w_simple: float, w_vlb: float, status=None):
    """(importance-weighted loss, rows (3, B)): dmme_iddpm_loss_rows.  loss = mean_b weight_b rows[2][b]; rows = per-image L_simple, L_vlb and
    w_simple L_simple + w_vlb L_vlb, unweighted and outside the autograd graph; the gradient carries weight_b.  `status`: device int32[1]
    the kernel sets when a t lies outside [1, timesteps]."""
    dev = model_out.device
    if weight is not None:
        weight = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    return _IDDPMLossRowsFunction.apply(model_out, x_t, x_0, target, t, coef.to(device=dev, dtype=torch.float32).contiguous(), timesteps, weight,
                                        w_simple, w_vlb, status)


class _ConsistencyLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out: Tensor, z_t: Tensor, f_target: Tensor, rows: Tensor, idx: Tensor, steps: int, metric: int, c: float):
        o = out.detach().to(torch.float32).contiguous()
        B = o.size(0)
        loss = torch.empty(1, dtype=torch.float32, device=o.device)
        scratch = torch.empty(65 * B, dtype=torch.float32, device=o.device)
        d_out = torch.empty_like(o) if out.requires_grad else None
        _lib.check(_lib.lib().dmme_cm_loss(int(metric), _lib.ptr(z_t), _lib.ptr(o), _lib.ptr(f_target), _lib.ptr(rows), _lib.ptr(idx), int(steps), B, o[0].numel(),
                                           float(c), _lib.ptr(loss), _lib.ptr(None), _lib.ptr(d_out), 1.0, _lib.ptr(scratch), _lib.stream_ptr()), "dmme_cm_loss")
        ctx.d_out = d_out
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        d = ctx.d_out
        ctx.d_out = None
        return (d * grad_out if d is not None else None), None, None, None, None, None, None, None


def consistency_loss_apply(out: Tensor, z_t: Tensor, f_target: Tensor, rows: Tensor, idx: Tensor, steps: int, metric: int, c: float) -> Tensor:
    """the consistency-distillation loss (1/B) sum_b d(f(z_t, t; out)_b, f_target_b) with a HIP gradient with respect to the student's raw
    output `out` (dmme_cm_loss): f is the boundary-conditioned consistency function of the table row of image b's grid index, d the
    pseudo-Huber metric (metric 0, constant c > 0) or the per-image mean of squares (metric 1).  rows: the fp32 device table
    [steps+1][12] of diffusion_models.consistency_rows; idx: one grid index per image (an index outside 1..steps gives a NaN loss)."""
    dev = out.device
    if z_t.shape != out.shape or f_target.shape != out.shape or idx.numel() != out.shape[0]:
        raise ValueError(f"consistency_loss_apply: output {tuple(out.shape)}, images {tuple(z_t.shape)}, target {tuple(f_target.shape)}, {idx.numel()} indices")
    if rows.numel() != 12 * (int(steps) + 1):
        raise ValueError(f"consistency_loss_apply: a table of {rows.numel()} floats for {steps} steps")
    if not idx.is_cuda and idx.numel() and not (1 <= int(idx.min()) and int(idx.max()) <= int(steps)):
        raise ValueError(f"consistency_loss_apply: a grid index outside 1..{int(steps)}")
    prep = lambda v: v.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    return _ConsistencyLossFunction.apply(out, prep(z_t), prep(f_target), prep(rows).reshape(-1), idx.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous(),
                                          int(steps), int(metric), float(c))
