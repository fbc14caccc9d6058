"""Block-local parity of the forward pass and of the GroupNorm statistics it keeps, as the plan drives them - the forward twin of
tests/test_gpu_block_grads.py.

One forward runs through the library.  Then every node of the layer graph (input conv, every ResBlock with or without attention, the
down / up convs, the output conv) is recomputed in float64 on the CPU from what the kernels themselves stored - debug_activation of
the node's producers (an up ResBlock: the concat) and `condition` - and compared with the node's stored output, so rounding error
does not pile up across 30 blocks and a bound can be tight.  The reference rounds where the kernels round (oracle.*.res_block's `q`
hook, 16-bit weights) and runs on picked images only (tests/block_local.py: pick_images; the IDDPM head merge reads other images'
rows, attention_sources).

Each case runs under three weight sets (tests/stress_weights.py): the default synthetic weights, `peaked` (a sharp softmax in every
attention block: logit standard deviation ~3, mean top probability >= 0.2) and `offset` (GroupNorm inputs at |mean| / std up to 8.7).
With the default weights the softmax is almost uniform and the norms' inputs almost centred (tests/test_stress_regime.py asserts
both regimes on the CPU): neither a wrong key weighting nor a cancelling variance would move any network-level figure by its bound.

What keeps a bound honest: under `peaked` every "res+attention" node is also compared with two MUTATED references built from the
same stored inputs - a uniform softmax, and scores x 1.05 - and those must fail the node's bound.

The second half reads the {mean, rstd} rows a train-mode forward keeps for the backward (debug_norm_stats) and compares them with
float64 statistics of the norm's stored input, under `offset` and the default weights, with every GroupNorm route switched in turn.
"""

import ctypes as C
import time

import pytest
import torch

from oracle import iddpm as OI
from oracle import synth
from oracle import unet as O
from tests import block_local as BL
from tests import stress_weights as SW

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

ROLES = ("in", "res", "res+attention", "down", "up", "out")

# Bounds per (precision, role): (max-abs error over max |want|, relative RMS), 2x the worst value measured on an MI355X against the
# float64 block-local reference over the whole matrix below (three weight sets, the five attention switches included); the maximum is
# an extreme-value statistic that moves with tile shapes.  Measured worst, max-abs / max (relative RMS):
#   bf16    in 3.59e-3 (1.66e-3), res 5.72e-3 (2.22e-3), res+attention 9.76e-3 (4.06e-3; B = 5, DMME_NO_LVL, peaked), down 3.40e-3 (1.68e-3),
#           up 3.72e-3 (1.71e-3), out 3.18e-4 (5.86e-5)
#   fp16    in 3.29e-4 (2.08e-4), res 4.52e-4 (2.14e-4), res+attention 9.45e-4 (3.83e-4), down 4.01e-4 (2.10e-4), up 4.64e-4 (2.08e-4),
#           out 7.47e-5 (1.27e-5)
#   bf16x3  in 2.67e-7 (1.22e-7), res 6.85e-6 (6.07e-6), res+attention 1.97e-5 (9.33e-6; peaked), down 5.48e-6 (4.61e-6), up 5.60e-6 (4.71e-6),
#           out 8.15e-6 (7.57e-6)
#   fp32    every role <= 2.65e-6 (1.71e-6)
# The relative RMS of a 16-bit conv node is the rounding of its stored output (bf16 1.66e-3, fp16 2.08e-4: a uniform error of half a unit
# in the last place over a binade); the network output is fp32, its error the rare re-rounding flips of the activated operand.
# fp32 keeps the project's 1e-5 of max(1, |want| max) and is not re-measured upward.
BOUNDS = {
    "bf16": {"in": (7.2e-3, 3.4e-3), "res": (1.2e-2, 4.5e-3), "res+attention": (2.0e-2, 8.2e-3), "down": (6.8e-3, 3.4e-3), "up": (7.5e-3, 3.5e-3),
             "out": (6.4e-4, 1.2e-4)},
    "fp16": {"in": (6.6e-4, 4.2e-4), "res": (9.1e-4, 4.3e-4), "res+attention": (1.9e-3, 7.7e-4), "down": (8.1e-4, 4.2e-4), "up": (9.3e-4, 4.2e-4),
             "out": (1.5e-4, 2.6e-5)},
    "bf16x3": {"in": (5.4e-7, 2.5e-7), "res": (1.4e-5, 1.3e-5), "res+attention": (4.0e-5, 1.9e-5), "down": (1.1e-5, 9.3e-6), "up": (1.2e-5, 9.5e-6),
               "out": (1.7e-5, 1.6e-5)},
}
FP32_ATOL = 1e-5
# Under `peaked` the two mutated references must FAIL these bounds (either measure outside), in every block with attention and every
# precision.  Measured: the uniform softmax 0.22 .. 0.67 of the maximum; scores x 1.05 1.0e-2 .. 2.9e-2 of the maximum, relative RMS 8.7e-3 ..
# 1.7e-2.  fp32, fp16, bf16x3 (bounds 1e-5 .. 1.9e-3): both measures fail by 5x and more.  bf16: the max-abs bound of 2.0e-2 leaves scores x
# 1.05 room only in four of the six DDPM blocks (2.1e-2 .. 2.9e-2; down_layers.4 1.8e-2 .. 1.9e-2 and the 4x4 middle block 1.1e-2 .. 1.4e-2
# stay inside, as does every IDDPM block but two), so there the relative RMS decides - a stable statistic, not an extreme value: 8.7e-3
# (IDDPM middle_layers.0) .. 1.7e-2 against the bound of 8.2e-3, with the kernel's own 2.4e-3 .. 4.1e-3.  The margins are printed.


def _setup(arch, precision, fixture):
    import dmme_amd
    from dmme_amd.models import iddpm

    if arch == "iddpm":
        cfg = OI.IUNetConfig(attention_depths=(3, 4))
        sd = SW.FIXTURES[fixture](OI.make_state_dict(cfg, 41), cfg)
        net = iddpm.UNet(attention_depths=(3, 4), precision=precision)
        T = 4000
    else:
        cfg = O.UNetConfig()
        sd = SW.FIXTURES[fixture](O.make_state_dict(cfg, 23), cfg)
        net = dmme_amd.UNet(precision=precision)
        T = 1000
    net.load_state_dict(sd)
    return cfg, sd, net.cuda(), T


def _level_info(net):
    from dmme_amd import _lib

    plan = net._last_plan
    buf = C.create_string_buffer(2048)
    _lib.check(plan.lib.dmme_unet_plan_level_info(plan.h, buf, 2048), "level_info")
    return buf.value.decode()


def _read(net, arch, cfg, B, H, pick):
    """stored activations of the images the reference needs (sorted list `have`), the graph"""
    g = (OI if arch == "iddpm" else O).build_graph(cfg)
    have = BL.images_needed(arch, cfg, pick, B)
    idx = torch.tensor(have, device="cuda")
    acts = {k: net.debug_activation(k).view(s)[idx].cpu() for k, s in BL._shapes(g, B, H).items()}
    acts["condition"] = net.debug_activation("condition").view(B, cfg.emb_dim)[idx].cpu()
    return g, have, acts


def _err(got, want):
    d = (got.double() - want).abs()
    top = float(want.abs().max())
    return float(d.max()) / top, float(d.pow(2).sum().sqrt() / want.pow(2).sum().sqrt()), float(d.max()), top


def _assert_routes(net, arch, precision, B, H, env):
    """the kernels the case exists for did run (plan labels, level-engine runs)"""
    from tests.gpu_util import fwd_labels

    labels = fwd_labels(net, B, H)
    attn = [l for l in labels if l.startswith("attn_")]
    info = _level_info(net)
    has = lambda s: any(s in l for l in labels)  # noqa: E731
    if arch == "iddpm":
        assert len(attn) == 11 and all(l.endswith(",heads>") for l in attn), attn  # multi-head attention at 256 and 64 tokens
        assert info.startswith("runs=0"), info
        return
    assert len(attn) + (0 if "DMME_NO_LVL" in env or precision in ("fp32", "bf16x3") else 1) == 6, (attn, info)
    n16 = [l for l in attn if "s16" not in l]  # the five 16x16 blocks (the 4x4 middle block: the level engine, or attn_s16_kernel)
    if precision in ("fp32", "bf16x3"):  # their own attention kernels
        assert len(n16) == 5 and all(l == ("attn_x3_kernel" if precision == "bf16x3" else "attn_generic_kernel<float>") for l in n16), attn
        assert info.startswith("runs=0"), info
        return
    if "DMME_NO_LVL" in env:
        assert info.startswith("runs=0"), info
    else:
        assert info.startswith("runs=3") and "err=1" not in info, info  # (B = 5, 1: partial pixel groups, a 4x4 group is 4 images)
    if "DMME_NO_ATTN_FULL" in env:
        assert not has("attn_full_kernel"), attn
    elif B >= 128 and "DMME_NO_ATTN_PROJ" not in env:
        assert len(n16) == 5 and all(l.startswith("attn_full_kernel") and l.endswith(",proj>") for l in n16), attn
        assert has("conv3x3_ws2_kernel") and has("(norm finished by its producers' epilogues)") and has("(norm finished by its consumer's parameter fill)"), labels
    else:
        # below 128 rows the whole-row launch would leave compute units idle: launch_attention splits the keys over the waves
        # (attn_split_kernel, attn_mfma.hip) unless no_attn_split - same plan label
        assert len(n16) == 5 and all(l.startswith("attn_full_kernel<") and not l.endswith(",proj>") for l in n16), attn


def _forward_case(arch, precision, B, H, fixture, env=None):
    """one eval-mode forward + the block-local float64 reference on the picked images; prints the per-role table and returns it with
    the mutation margins of the blocks with attention"""
    from tests.gpu_util import route_env

    env = dict(env or {})
    cfg, sd, net, T = _setup(arch, precision, fixture)
    net.eval()
    x = synth.normal(11, (B, 3, H, H))  # distinct images, distinct timesteps
    t = (torch.arange(B) * 997 + 13) % T
    with route_env(env), torch.no_grad():
        y = net(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        net._last_plan.check()
        _assert_routes(net, arch, precision, B, H, env)
    pick = BL.pick_images(B)
    g, have, acts = _read(net, arch, cfg, B, H, pick)
    t0 = time.time()
    ref = BL.forward_reference(arch, cfg, sd, precision, x, acts, None, pick, B, BL.MUTATIONS, have=have)
    secs = time.time() - t0
    rows = [have.index(b) for b in pick]
    got = {k: v[rows] for k, v in acts.items() if k != "condition"}
    got["output"] = y.float().cpu()[pick]
    roles = BL.node_roles(g)
    assert set(ref) == set(got) == set(roles)
    worst = {r: [0.0, 0.0, "", 0.0, 0.0] for r in ROLES}  # max-abs / max, relative RMS, node of the first, its max-abs error, its max |want|
    margins = {}
    for k, modes in ref.items():
        assert bool(torch.isfinite(got[k]).all()), k
        mx, rms, ab, top = _err(got[k], modes[None])
        w = worst[roles[k]]
        if mx > w[0]:
            w[0], w[2], w[3], w[4] = mx, k, ab, top
        w[1] = max(w[1], rms)
        if len(modes) > 1:
            margins[k] = {"good": (mx, rms, ab, top), **{m: _err(got[k], modes[m]) for m in BL.MUTATIONS}}
    tag = f"{arch} {precision} B={B} {fixture}" + (f" {'+'.join(env)}" if env else "")
    print(f"\n{tag}: fp64 block-local reference on images {pick}: {secs:.1f} s")
    print(f"{tag} worst max-abs / max (relative RMS) per role:", {r: f"{w[0]:.2e} ({w[1]:.2e}) {w[2]}" for r, w in worst.items()})
    print(f"{tag} blocks with attention, error vs reference / vs uniform softmax / vs scores x 1.05 (max-abs / max; relative RMS):",
          {k: f"{m['good'][0]:.2e} / {m['uniform'][0]:.2e} / {m['scale'][0]:.2e} (RMS {m['good'][1]:.2e} / {m['uniform'][1]:.2e} / {m['scale'][1]:.2e})" for k, m in margins.items()})
    return worst, margins


def _within(precision, role, mx, rms, ab, top):
    if precision == "fp32":
        return ab <= FP32_ATOL * max(1.0, top)
    b = BOUNDS[precision][role]
    return mx <= b[0] and rms <= b[1]


def _check_case(arch, precision, B, H, fixture, env=None):
    worst, margins = _forward_case(arch, precision, B, H, fixture, env)
    bad = []
    for r, (mx, rms, k, ab, top) in worst.items():
        if not _within(precision, r, mx, rms, ab, top):
            bad.append(f"{r}: max-abs / max {mx:.3e}, relative RMS {rms:.3e} at {k} (bound {BOUNDS.get(precision, {}).get(r, FP32_ATOL)})")
    assert len(margins) == (11 if arch == "iddpm" else 6)
    if fixture == "peaked":
        # a reference with a wrong softmax must be OUTSIDE the bound the kernel is held to
        for k, m in margins.items():
            for mode in BL.MUTATIONS:
                inside = _within(precision, "res+attention", *m[mode])
                if precision == "bf16" and mode == "scale":
                    b = BOUNDS["bf16"]["res+attention"]
                    print(f"  bf16 {k}: scores x 1.05 at {m[mode][0] / b[0]:.2f}x the max-abs bound, {m[mode][1] / b[1]:.2f}x the RMS bound")
                if inside:
                    bad.append(f"{k}: the reference with softmax mutation '{mode}' is within the bound ({m[mode][0]:.3e}, RMS {m[mode][1]:.3e})")
    assert not bad, f"{arch} {precision} B={B} {fixture} {env or ''}:\n  " + "\n  ".join(bad)


# ---- the matrix: the smallest shapes that still reach each route ---------------------------------------------------------------------
CASES = [
    # (arch, precision, batch, map)
    ("ddpm", "bf16", 128, 32),   # level engine runs=3, attn_full_kernel with the proj tail, conv3x3_ws2_kernel, norms finished by producer / consumer
    ("ddpm", "fp16", 128, 32),
    ("ddpm", "bf16", 5, 32),     # level engine with partial pixel groups, attn_split_kernel
    ("ddpm", "bf16", 1, 32),
    ("ddpm", "fp32", 3, 32),     # their own attention kernels
    ("ddpm", "bf16x3", 3, 32),   # attn_x3_kernel
    ("iddpm", "bf16", 32, 64),   # multi-head attention at 256 and 64 tokens
    ("iddpm", "bf16", 3, 64),
]
_ids = [f"{c[0]}-{c[1]}-b{c[2]}" for c in CASES]


@pytest.mark.parametrize("fixture", ["default", "peaked", "offset"])
@pytest.mark.parametrize("arch,precision,B,H", CASES, ids=_ids)
def test_block_local_forward_parity(arch, precision, B, H, fixture):
    _check_case(arch, precision, B, H, fixture)


# every attention implementation meets a sharp softmax inside the network
SWITCHES = [(128, "DMME_NO_LVL"), (5, "DMME_NO_LVL"), (128, "DMME_NO_ATTN_FULL"), (5, "DMME_NO_ATTN_SPLIT"), (128, "DMME_NO_ATTN_PROJ")]


@pytest.mark.parametrize("B,switch", SWITCHES, ids=[f"b{b}-{s}" for b, s in SWITCHES])
def test_block_local_forward_parity_attention_routes_under_peaked_weights(B, switch):
    _check_case("ddpm", "bf16", B, 32, "peaked", {switch: "1"})


# ---- GroupNorm statistics as the forward left them ----------------------------------------------------------------------------------
# Errors: |mean - mean64| * rstd64 and |rstd / rstd64 - 1| per (image, group), worst per norm, against float64 statistics of the norm's
# input on the picked images.  The kernels take their statistics from the values they STORE (the rounded outputs the consumer reads
# back), so where the input is a named tensor - <block>.conv1.0 and output_conv.0: the conv2 epilogue with its residual, the down / up
# convs, the concat, the attention-proj partials, the whole-image tiles, the level engine - the comparison is exact up to fp32
# arithmetic.  <block>.conv2.0 (IDDPM: <block>.norm) and <block>.attention.norm read an unnamed tensor that the reference recomputes, and
# the recomputed tensor differs from the kernel's at the recomputation's own rounding level: by at most one unit in the last place of
# its largest value, u = eps * max |x|, which moves the mean by <= u and rstd by <= u * rstd relative (d var <= 2 sigma u).  Those norms
# get u * rstd64 on top of the bound below, with eps = 2^-8 (bf16), 2^-11 (fp16), 2^-16 (bf16x3: the lo x lo products the three passes
# leave out) and 2^-23 (fp32: the accumulation order of the conv - tight, 1e-7 .. 1e-6).  So the 16-bit types see a cancellation
# only through the named norms; fp32 sees it through both.
# Bound: what the reference's own fp32 arithmetic gives on the same inputs - torch.native_group_norm in fp32 on the CPU against float64,
# per norm - times 4, with a floor of 4 ulp of fp32.  The margin covers another summation order; it does not cover a cancellation.
# Measured on an MI355X under `offset`: error / bound of the named norm nearest its bound, per route (default routes, DMME_NO_FUSED_GN,
# DMME_NO_GN_IN, DMME_NO_GN_DIRECT, DMME_NO_LVL); under the default weights every route has mean <= 1.3e-7 and rstd <= 2.8e-7 against 4.8e-7.
#   ddpm bf16 B = 128     mean 5.1e-7 / 7.8e-7, 3.3e-7 / 8.4e-7, 6.5e-7 / 1.1e-6, 5.1e-7 / 7.8e-7, 5.1e-7 / 7.8e-7; rstd <= 1.4e-7 / 4.8e-7
#   ddpm fp16 B = 128     mean 4.4e-7 / 1.2e-6, 2.8e-7 / 5.4e-7, 2.9e-7 / 1.1e-6, 4.4e-7 / 1.2e-6, 4.3e-7 / 8.7e-7; rstd <= 3.4e-7 / 4.8e-7
#   ddpm bf16 B = 5       mean 3.9e-7 / 8.9e-7, 3.5e-7 / 9.3e-7, 2.7e-7 / 6.1e-7, 3.9e-7 / 8.9e-7, 3.9e-7 / 8.1e-7; rstd <= 1.9e-7 / 4.8e-7
#   ddpm bf16 B = 1       mean 3.9e-7 / 5.4e-7, 2.0e-7 / 4.8e-7, 3.1e-7 / 6.7e-7, 3.9e-7 / 5.4e-7, 3.9e-7 / 5.4e-7; rstd <= 1.9e-7 / 4.8e-7
#   ddpm fp32 B = 3       mean 3.0e-7 / 4.8e-7 (DMME_NO_FUSED_GN 3.5e-7 / 7.4e-7); rstd <= 1.3e-7 / 4.8e-7
#   ddpm bf16x3 B = 3     mean 2.2e-7 / 4.8e-7 (DMME_NO_FUSED_GN 2.5e-7 / 4.8e-7); rstd <= 1.3e-7 / 4.8e-7
#   iddpm bf16 B = 32     mean 5.4e-7 / 6.9e-7, 1.1e-7 / 8.6e-7, 5.1e-7 / 1.1e-6, 5.4e-7 / 1.0e-6, 5.4e-7 / 6.9e-7; rstd <= 2.4e-7 / 4.8e-7
#   iddpm bf16 B = 3      mean 3.8e-7 / 5.4e-7, 1.2e-7 / 1.1e-6, 2.7e-7 / 6.3e-7, 3.8e-7 / 5.4e-7, 3.8e-7 / 5.4e-7; rstd <= 2.5e-7 / 4.8e-7
# Two routes were outside it when this test was written and were fixed with it: the fp32 conv epilogue's per-thread raw moments (fp32 and
# bf16x3 plans, every route but DMME_NO_FUSED_GN: rstd 7.4e-7 named, up to 1.1e-6 recomputed; conv_common.h now sums about the thread's
# first value), and the mean of the launched two-pass kernels at the IDDPM network's 64x64 concat (DMME_NO_FUSED_GN: 1.3e-6 / 8.2e-7 at
# B = 32, 6.2e-7 / 4.8e-7 at B = 3; gn_fast.hip now corrects the mean by the centred pass's first moment and merges chunks about a pivot).
# At |mean| / std = 8.7 half a unit in the last place of the mean alone is 4.8e-7 of a standard deviation: a route has room for about one
# more rounding of the mean.  Recomputed norms (default routes): 16-bit 2.5e-5 .. 8.6e-4 against 2e-3 .. 3.4e-2, bf16x3 7e-6 against 1.1e-4,
# fp32 mean 6.1e-7 / 2.2e-6, rstd 1.3e-7 / 1.3e-6.  precision="fp16r32" is not in the matrix: its plans keep the raw moments
# (ConvArgs::gn_raw_moments) so that the mode's fp16 rounding sequence, and the 1e-3 figures measured with it, stay as they are.
GN_SWITCHES = (None, "DMME_NO_FUSED_GN", "DMME_NO_GN_IN", "DMME_NO_GN_DIRECT", "DMME_NO_LVL")
ULP32 = 2.0**-23


def _stat_errors(mr, x, groups):
    """mr: the kernel's rows (n, G, 2); x: the norm's input (n, C, H, W) float64.  -> (kernel mean error, kernel rstd error, fp32 CPU
    mean error, fp32 CPU rstd error, u * rstd64), each the worst over (image, group)"""
    mean, rstd = BL.group_stats(x, groups)
    x32 = x.float()
    _, m32, r32 = torch.native_group_norm(x32, None, None, x32.shape[0], x32.shape[1], x32.shape[2] * x32.shape[3], groups, BL.EPS)
    em = float(((mr[..., 0].double() - mean).abs() * rstd).max())
    er = float((mr[..., 1].double() / rstd - 1).abs().max())
    rm = float(((m32.double() - mean).abs() * rstd).max())
    rr = float((r32.double() / rstd - 1).abs().max())
    flat = x.reshape(x.shape[0], groups, -1).abs().amax(-1)
    return em, er, rm, rr, float((flat * rstd).max())


def _stats_case(arch, precision, B, H, fixture):
    from tests.gpu_util import route_env

    cfg, sd, net, T = _setup(arch, precision, fixture)
    M = OI if arch == "iddpm" else O
    masks = M.make_drop_masks(cfg, B, 7)
    net.train()
    net.inject_dropout_masks(torch.cat([masks[k].reshape(-1) for k in M.res_block_names(cfg)]).cuda())
    x = synth.normal(11, (B, 3, H, H))
    t = (torch.arange(B) * 997 + 13) % T
    pick = BL.pick_images(B)
    eps_re = {"bf16": 2.0**-8, "fp16": 2.0**-11, "bf16x3": 2.0**-16, "fp32": 2.0**-23}[precision]
    bad, table = [], {}
    for sw in GN_SWITCHES:
        net._plans.clear()  # the switches are read when a plan is created
        with route_env({sw: "1"} if sw else {}):
            net(x.cuda(), t.cuda())  # with autograd: the form that keeps what a backward reads
            torch.cuda.synchronize()
            net._last_plan.check()
            info = _level_info(net)
        g, have, acts = _read(net, arch, cfg, B, H, pick)
        rows = [have.index(b) for b in pick]
        named = {n.prefix + ".conv1.0": torch.cat([acts[k][rows] for k in ins], 1).double() for n, ins in BL._walk(g)[0] if n.kind == "res"}
        named["output_conv.0"] = acts[BL._walk(g)[1]][rows].double()
        inputs = dict(named)
        if sw is None:  # the unnamed inputs too: the reference recomputes them (once per case)
            inputs = {}
            BL.forward_reference(arch, cfg, sd, precision, x, acts, masks, pick, B, norm_inputs=inputs, have=have)
            assert set(named) <= set(inputs)
            for k, v in named.items():
                assert torch.equal(inputs[k], v), k
        worst = {"named": [0.0, 0.0, 0.0, 0.0, ""], "recomputed": [0.0, 0.0, 0.0, 0.0, ""]}
        for k, xin in inputs.items():
            mr = net.debug_norm_stats(k).cpu()[pick]
            em, er, rm, rr, urel = _stat_errors(mr, xin, cfg.num_groups)
            kind = "named" if k in named else "recomputed"
            extra = 0.0 if kind == "named" else eps_re * urel
            bm, br = max(4 * rm, 4 * ULP32) + extra, max(4 * rr, 4 * ULP32) + extra
            w = worst[kind]
            if max(em / bm, er / br) >= max(w[0] / max(w[2], 1e-300), w[1] / max(w[3], 1e-300)):
                worst[kind] = [em, er, bm, br, k]
            if em > bm or er > br:
                bad.append(f"{sw or 'default routes'}: {k} ({kind}) mean error {em:.3e} (bound {bm:.3e}), rstd error {er:.3e} (bound {br:.3e})")
        table[sw or "default routes"] = {k: f"mean {w[0]:.2e} / {w[2]:.2e}, rstd {w[1]:.2e} / {w[3]:.2e} at {w[4]}" for k, w in worst.items() if w[4]}
        if arch == "ddpm" and precision in ("bf16", "fp16"):
            assert info.startswith("runs=0" if sw == "DMME_NO_LVL" else "runs=3"), (sw, info)
    print(f"\n{arch} {precision} B={B} {fixture}: GroupNorm statistics, worst error / bound per route:")
    for k, v in table.items():
        print(f"  {k}: {v}")
    assert not bad, f"{arch} {precision} B={B} {fixture}: {len(bad)} norms outside their bound:\n  " + "\n  ".join(bad[:40])


@pytest.mark.parametrize("fixture", ["default", "offset"])
@pytest.mark.parametrize("arch,precision,B,H", CASES, ids=_ids)
def test_groupnorm_statistics_as_the_forward_left_them(arch, precision, B, H, fixture):
    _stats_case(arch, precision, B, H, fixture)
