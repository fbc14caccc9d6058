"""Block-local parity of the 16-bit (and fp32) backward pass, as the plan drives it.

One training step runs through the library (train mode, injected Dropout2d masks, distinct images and timesteps, loss
L = 1/2 sum (y - z)^2 so that dL/dy = y - z is O(1) and no 16-bit gradient sinks into the subnormals).  Then every block of the
layer graph (oracle.unet.build_graph / oracle.iddpm.build_graph) is differentiated ON ITS OWN by torch autograd in float64 on
the CPU, fed with what the kernels themselves saw: the block's stored inputs (debug_activation of the producers; an up
ResBlock reads the concat of h and the skip), the time embedding, the block's dropout mask and dY = debug_gradient(block)
(the output conv: the loss gradient itself).  Rounding error therefore does not pile up across 30 blocks and the bounds can
be tight.  The reference rounds operands where the kernels round them (test_gpu_ops._ref_conv's convention): inputs as
stored, conv / linear weights in the 16-bit type, the activated input of every conv, the conv1 output and the attention's
normalised input, qkv and context (oracle.*.res_block's `q` hook).  The rounding is straight-through, so the reference's
gradients themselves are not rounded.

Compared per block: every parameter gradient the block owns (p.grad), the gradient of every named tensor against the sum of
its consumers' VJPs (concat gradients split at the channel boundary: stride-2 zero insertion, the upsample's 2x2 sum, the
GroupNorm backward, grad_acc, the pending-residual merge and the direct data gradient all sit on that path), and the time
MLP's parameter gradients against the VJP of d(temb) = sum over blocks, pushed through oracle time_embedding.

Error measure: relative L2 ||g - g_ref|| / ||g_ref|| per tensor, worst per role; bounds per (role, precision) below.
"""

import time
from typing import Dict

import pytest
import torch
import torch.nn.functional as F

from oracle import iddpm as OI
from oracle import synth
from oracle import unet as O
from tests.block_local import _rounder, _shapes, _walk, _wround

torch.set_num_threads(min(16, torch.get_num_threads()))

# ---- roles -------------------------------------------------------------------------------------------------------------------------
# exact_w: weight gradients whose operands are exactly what the kernel multiplied: dY as stored (the block's own, or the loss
#          gradient) x the stored / re-rounded activation - conv2 and the residual 1x1 of a block without attention, the down / up
#          conv, the input and the output conv.
# exact_b: the column sums of dY of those convs.
# inner_w / inner_b: everything whose dY is an internal 16-bit gradient of the kernel, or whose operand the reference recomputes:
#          conv1, the time-projection rows, and in a block with attention conv2, the residual 1x1, qkv and proj (the context is
#          recomputed from the stored qkv and re-rounded).
# gn:      GroupNorm gamma / beta.
# dgrad:   gradients of the named tensors (debug_gradient).
# time:    condition.1 / condition.3 (the time MLP).
ROLES = ("exact_w", "exact_b", "inner_w", "inner_b", "gn", "dgrad", "time")

# Bounds on the relative L2 error of the worst tensor of each role, ~2x the worst value measured on an MI355X over the batches of the
# matrix (bf16: B = 128 / 5 / 1 and IDDPM-64 B = 32 / 3; fp16: B = 128 / 3; fp32: B = 3), measured relative L2 (max-abs / max):
#   bf16  exact_w 2.3e-4 (9.8e-4), exact_b 9.2e-8 (1.3e-7), inner_w 3.9e-3 (6.3e-3), inner_b 3.9e-3 (6.3e-3), gn 4.4e-3 (7.4e-3),
#         dgrad 4.3e-3 (8.0e-3), time 2.2e-3 (B = 1; 4.4e-4 at B = 128)
#   fp16  exact_w 8.4e-5 (2.9e-4), exact_b 3.3e-7 (3.5e-7), inner_w 5.1e-4 (8.6e-4), inner_b 5.3e-4 (8.9e-4), gn 6.8e-4 (1.0e-3),
#         dgrad 5.4e-4 (9.7e-4), time 2.0e-4
#   fp32  every role <= 1.6e-6 (1.8e-6 max-abs); exact_b 1.2e-7 (1.6e-7)
# exact_w / exact_b sit at fp32 accumulation level (the weight gradients add the rare re-rounding flips of the recomputed GroupNorm +
# SiLU operand); the 16-bit rounding of ONE internal gradient (2^-9 bf16, 2^-12 fp16, relative) is what separates inner from exact.
# The max-abs error over max |g_ref| of a role is held at 2x its L2 bound; for exact_w, whose max-abs statistic is 4x its L2 error,
# that sets the L2 bound (bf16 1e-3, fp16 2e-4).
BOUNDS = {
    "bf16": {"exact_w": 1e-3, "exact_b": 3e-7, "inner_w": 8e-3, "inner_b": 8e-3, "gn": 8e-3, "dgrad": 8e-3, "time": 4e-3},
    "fp16": {"exact_w": 2e-4, "exact_b": 1e-6, "inner_w": 1e-3, "inner_b": 1e-3, "gn": 1.2e-3, "dgrad": 1e-3, "time": 4e-4},
    "fp32": {"exact_w": 4e-6, "exact_b": 4e-7, "inner_w": 4e-6, "inner_b": 4e-6, "gn": 4e-6, "dgrad": 4e-6, "time": 4e-6},
}


def block_reference(arch, cfg, sd, precision, x_in, t, acts, dys, gy, masks):
    """Block-local float64 VJPs.  acts: name -> stored activation (incl. "condition"); dys: name -> the kernel's gradient of that
    tensor (dY of the block that produces it); gy: dL/dy of the network output.  Returns (param grads, named-tensor gradients as
    sums over consumers, the mutated conv2 weight gradients of the sensitivity check)."""
    q, wq = _rounder(precision), _wround(precision)
    M = OI if arch == "iddpm" else O
    g = M.build_graph(cfg)
    sdq = {}
    for k, v in sd.items():
        if k == "condition.0.embeddings":
            sdq[k] = v.double()
        elif v.dim() >= 2:
            sdq[k] = wq(v).requires_grad_(True)
        else:
            sdq[k] = v.double().requires_grad_(True)
    leaf = lambda v: v.detach().to(torch.float64).clone().requires_grad_(True)  # (a fresh leaf per consumer)
    temb = leaf(acts["condition"])
    dsum: Dict[str, torch.Tensor] = {}
    mutated = {}  # conv2 weight gradient of the first ResBlock at every resolution, with image B // 2 dropped from dY
    ci = M._conv2_index(cfg)

    def add(name, v):
        dsum[name] = v if name not in dsum else dsum[name] + v

    seq, last = _walk(g)
    for n, ins in seq:
        leaves = [leaf(acts[k]) for k in ins]
        x = leaves[0] if len(leaves) == 1 else torch.cat(leaves, 1)
        if n.kind == "res":
            m = masks[n.prefix].double() if masks is not None else None
            y = M.res_block(sdq, cfg, n, x, temb, m, q)
        elif n.kind == "down":
            y = F.conv2d(x, sdq[n.prefix + ".weight"], sdq[n.prefix + ".bias"], stride=2, padding=1)
        else:
            y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), sdq[n.prefix + ".conv.weight"], sdq[n.prefix + ".conv.bias"], padding=1)
        dy = dys[n.prefix].double()
        if n.kind == "res" and dy.shape[0] > 1 and y.shape[-1] not in {v[0] for v in mutated.values()}:
            dmut = dy.clone()
            dmut[dy.shape[0] // 2] = 0
            key = f"{n.prefix}.conv2.{ci}.weight"
            (w,) = torch.autograd.grad(y, sdq[key], dmut, retain_graph=True)
            mutated[key] = (y.shape[-1], n.attn, w)
        y.backward(dy)
        for k, lf in zip(ins, leaves):
            add(k, lf.grad)
    # output conv: GroupNorm + SiLU, rounded, conv; its dY is the loss gradient as the kernel stored it
    xl = leaf(acts[last])
    h = q(F.silu(F.group_norm(xl, cfg.num_groups, sdq["output_conv.0.weight"], sdq["output_conv.0.bias"], eps=1e-5)))
    y = F.conv2d(h, sdq["output_conv.2.weight"], sdq["output_conv.2.bias"], padding=1)
    y.backward(q(gy.double()))
    add(last, xl.grad)
    # input conv: the 3-channel network input stays fp32
    xi = x_in.double()
    y = F.conv2d(xi, sdq["input_conv.weight"], sdq["input_conv.bias"], padding=1)
    y.backward(dys["input_conv"].double())
    # time MLP: d(temb) summed over the blocks, through the oracle's time embedding (fp64, 16-bit Linear weights)
    te = O.time_embedding(sdq, t.double())
    te.backward(temb.grad)
    grads = {k: v.grad for k, v in sdq.items() if v.requires_grad}
    return grads, dsum, mutated


def _role(name, attn_blocks):
    if name.startswith("condition."):
        return "time"
    if name.startswith("output_conv.0") or ".conv1.0." in name or ".conv2.0." in name or ".norm." in name:
        return "gn"
    w = name.endswith(".weight")
    if ".conv1.2." in name or ".condition.0." in name or ".attention." in name or any(name.startswith(b + ".") for b in attn_blocks):
        return "inner_w" if w else "inner_b"
    return "exact_w" if w else "exact_b"


def _rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300)), float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _run_case(arch, precision, B, H, expect_routes):
    """one training step through the library + the block-local reference; returns the per-role worst errors"""
    import dmme_amd
    from dmme_amd.models import iddpm
    from tests.gpu_util import bwd_summary

    if arch == "iddpm":
        cfg = OI.IUNetConfig(attention_depths=(3, 4))
        sd = OI.make_state_dict(cfg, 41)
        masks = OI.make_drop_masks(cfg, B, 7)
        names = OI.res_block_names(cfg)
        net = iddpm.UNet(attention_depths=(3, 4), precision=precision)
        T = 4000
    else:
        cfg = O.UNetConfig()
        sd = O.make_state_dict(cfg, 23)
        masks = O.make_drop_masks(cfg, B, 5)
        names = O.res_block_names(cfg)
        net = dmme_amd.UNet(precision=precision)
        T = 1000
    net.load_state_dict(sd)
    net.cuda().train()
    net.inject_dropout_masks(torch.cat([masks[k].reshape(-1) for k in names]).cuda())
    x = synth.normal(11, (B, 3, H, H))  # distinct images, distinct timesteps
    z = synth.normal(12, (B, net.out_channels, H, H))
    t = (torch.arange(B) * 997 + 13) % T
    y = net(x.cuda(), t.cuda())
    gy = (y.detach() - z.cuda()).contiguous()  # L = 1/2 sum (y - z)^2
    y.backward(gy)
    torch.cuda.synchronize()
    net._last_plan.check()
    g = (OI if arch == "iddpm" else O).build_graph(cfg)
    shapes = _shapes(g, B, H)
    acts = {k: net.debug_activation(k).view(s).cpu() for k, s in shapes.items()}
    acts["condition"] = net.debug_activation("condition").view(B, cfg.emb_dim).cpu()
    dys = {k: net.debug_gradient(k).view(s).cpu() for k, s in shapes.items()}
    pgrad = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    bw = bwd_summary(net, B, H)
    for key, lo in expect_routes.items():
        assert int(bw.get(key, 0)) >= lo, (key, bw)

    t0 = time.time()
    ref, dsum, mutated = block_reference(arch, cfg, sd, precision, x, t, acts, dys, gy.cpu(), masks)
    print(f"\n{arch} {precision} B={B}: fp64 block-local reference {time.time() - t0:.1f} s")
    n_par = sum(1 for _, p in net.named_parameters())
    assert len(ref) == n_par and set(dsum) == set(shapes), (len(ref), n_par, set(dsum) ^ set(shapes))
    attn_blocks = {n.prefix for n, _ in _walk(g)[0] if n.attn}
    worst = {r: (0.0, "") for r in ROLES}
    worst_max = {r: (0.0, "") for r in ROLES}

    def note(r, k, got, want):
        rel, mx = _rel(got, want)
        if rel > worst[r][0]:
            worst[r] = (rel, k)
        if mx > worst_max[r][0]:
            worst_max[r] = (mx, k)

    for k, gr in ref.items():
        note(_role(k, attn_blocks), k, pgrad[k], gr)
    for k, gr in dsum.items():
        note("dgrad", k, dys[k], gr)
    print(f"{arch} {precision} B={B} worst relative L2 (max-abs / max) per role:",
          {r: f"{worst[r][0]:.2e} ({worst_max[r][0]:.2e}) {worst[r][1]}" for r in ROLES})
    # sensitivity: the first ResBlock at every resolution; its conv2 weight gradient against a reference that lost ONE image's dY
    # (1/B of the sum) must fail its role's bound - the comparison tells the kernel from one that drops an image (or a 64-pixel
    # tile or split-K chunk of that weight)
    margins = {}
    for key, (hw, attn, w) in mutated.items():
        bound = BOUNDS[precision][_role(key, attn_blocks)]
        good, _ = _rel(pgrad[key], ref[key])
        bad, _ = _rel(pgrad[key], w)
        margins[f"{hw}x{hw}{' attn' if attn else ''} {key}"] = (good, bad, bound)
    print(f"{arch} {precision} B={B} sensitivity, conv2 weight: error vs reference / vs reference without image {B // 2} / bound:",
          {k: f"{a:.2e} / {b:.2e} / {c:.0e} ({b / c:.1f}x bound)" for k, (a, b, c) in margins.items()})
    for r in ROLES:
        bound = BOUNDS[precision][r]
        assert worst[r][0] <= bound, f"{arch} {precision} B={B}: {r} relative L2 {worst[r][0]:.3e} > {bound:.1e} at {worst[r][1]}"
        assert worst_max[r][0] <= 2 * bound, f"{arch} {precision} B={B}: {r} max-abs / max {worst_max[r][0]:.3e} > {2 * bound:.1e} at {worst_max[r][1]}"
    return margins


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------
# the grouped backward launches that the benchmark configuration runs (dmme_unet_plan_bwd_summary)
B128_ROUTES = {"wgrad_group3x3_jobs": 1000, "wgrad_group1x1_layers": 20, "colsum_group_jobs": 1, "bias_group_jobs": 1, "dgrad[conv3x3_ws2_kernel<11>]": 18}
CASES = [
    # (arch, precision, batch, map, routes that must have run, sensitivity asserted)
    ("ddpm", "bf16", 128, 32, B128_ROUTES, True),
    ("ddpm", "bf16", 5, 32, {"wgrad_group3x3_jobs": 1}, False),
    ("ddpm", "bf16", 1, 32, {"wgrad_group3x3_jobs": 1}, False),
    ("ddpm", "fp16", 128, 32, B128_ROUTES, True),
    ("ddpm", "fp16", 3, 32, {"wgrad_group3x3_jobs": 1}, False),
    ("ddpm", "fp32", 3, 32, {}, False),
    ("iddpm", "bf16", 32, 64, {"wgrad_group3x3_jobs": 1000, "dgrad[conv3x3_ws2_kernel<11>]": 10}, True),
    ("iddpm", "bf16", 3, 64, {"wgrad_group3x3_jobs": 1}, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("arch,precision,B,H,routes,sens", CASES, ids=[f"{c[0]}-{c[1]}-b{c[2]}" for c in CASES])
def test_block_local_backward_parity(arch, precision, B, H, routes, sens):
    margins = _run_case(arch, precision, B, H, routes)
    assert len(margins) == (4 if B > 1 else 0), margins  # one ResBlock per resolution (four depths in both networks)
    for k, (good, bad, bound) in margins.items():
        assert good <= bound, (k, good, bound)
        if sens:
            assert bad > bound, f"{k}: a reference without one of {B} images is within the bound ({bad:.3e} <= {bound:.1e})"


def test_block_local_reference_reassembles_the_network_gradient():
    """CPU: the block-local reference (no rounding) applied to the oracle's own activations and gradients gives back autograd of the
    whole network - every parameter gradient and every named tensor's gradient (the consumer sums, the concat split, the time MLP)"""
    for arch in ("ddpm", "iddpm"):
        M = OI if arch == "iddpm" else O
        cfg = OI.TINY_ATTN if arch == "iddpm" else O.TINY
        B, H = 3, 16
        sd = M.make_state_dict(cfg, 3)
        sdd = {k: v.double().requires_grad_(k != "condition.0.embeddings") for k, v in sd.items()}
        masks = M.make_drop_masks(cfg, B, 4)
        x = synth.normal(5, (B, cfg.in_channels, H, H)).double()
        t = torch.tensor([3, 500, 999])
        cap = {}
        y = M.unet_forward(sdd, cfg, x, t.double(), drop_masks={k: v.double() for k, v in masks.items()}, capture=cap)
        for v in cap.values():
            v.retain_grad()
        gy = synth.normal(6, tuple(y.shape)).double()
        y.backward(gy)
        acts = {k: v.detach() for k, v in cap.items()}
        dys = {k: v.grad for k, v in cap.items() if k != "condition"}
        ref, dsum, _ = block_reference(arch, cfg, sd, "fp32", x, t, acts, dys, gy, masks)
        for k, v in sdd.items():
            if v.requires_grad:
                assert _rel(ref[k], v.grad)[0] < 1e-12, (arch, k)
        assert set(dsum) == set(dys), (arch, set(dys) ^ set(dsum))
        for k in dsum:
            assert _rel(dsum[k], dys[k])[0] < 1e-12, (arch, k)
