"""CPU: the two stress fixtures of tests/stress_weights.py put the network where the block-local forward test needs it, and the
oracle still agrees with the reference there.

With oracle.*.make_state_dict weights and synth.normal images the softmax of every attention block is almost uniform and the
GroupNorm inputs are almost centred, so a kernel that weights its keys wrongly, or statistics that cancel at |mean| >> std, stay under
the network-level bounds.  `peaked` and `offset` move the two regimes; here the regimes are ASSERTED on the fp32 oracle's own
activations (B = 2), the block-local effect of a wrong softmax is tabulated under both weight sets (the GPU test compares against the
same mutated references), and the oracle is held to the imported reference's output under `peaked` (tests/golden/unet_peaked.npz).
"""

import functools

import numpy as np
import pytest
import torch

from oracle import iddpm as OI
from oracle import synth
from oracle import unet as O
from tests import block_local as BL
from tests import stress_weights as SW

torch.set_num_threads(min(16, torch.get_num_threads()))

# (architecture, config, seed, map): the default UNet, and the 64x64 IDDPM network of the GPU matrix (multi-head attention at 256 and 64 tokens)
ARCHS = {"ddpm": (O, O.UNetConfig(), 23, 32), "iddpm": (OI, OI.IUNetConfig(attention_depths=(3, 4)), 41, 64)}


@functools.lru_cache(maxsize=None)
def _regime(arch, fixture):
    """the fp32 oracle at B = 2, then every node once more block-locally in float64 from the oracle's own activations: the softmax
    figures of every attention block, |group mean| / std of every GroupNorm's input, and the blocks' outputs under the two mutations"""
    M, cfg, seed, H = ARCHS[arch]
    sd = SW.FIXTURES[fixture](M.make_state_dict(cfg, seed), cfg)
    x = synth.normal(11, (2, 3, H, H))
    t = torch.tensor([13, 900])
    cap = {}
    with torch.no_grad():
        M.unet_forward(sd, cfg, x, t, capture=cap)
    figures, norm_inputs = {}, {}
    ref = BL.forward_reference(arch, cfg, sd, "fp32", x, cap, None, [0, 1], 2, BL.MUTATIONS, figures, norm_inputs)
    for k, v in cap.items():  # the block-local float64 walk reproduces the oracle it was fed from
        if k != "condition":
            assert float((ref[k][None] - v.double()).abs().max()) <= 1e-4 * max(1.0, float(v.abs().max())), (arch, fixture, k)
    ratio = {}
    for k, v in norm_inputs.items():
        mean, rstd = BL.group_stats(v, cfg.num_groups)
        ratio[k] = float((mean.abs() * rstd).max())
    sens = {}
    for k, modes in ref.items():
        if len(modes) > 1:
            top = float(modes[None].abs().max())
            sens[k] = {m: float((modes[m] - modes[None]).abs().max()) / top for m in BL.MUTATIONS}
    amax = max(float(v.abs().max()) for k, v in cap.items() if k != "condition")
    return figures, ratio, sens, amax


@pytest.mark.parametrize("arch", list(ARCHS))
def test_regimes_are_asserted_not_assumed(arch):
    fd, rd, _, ad = _regime(arch, "default")
    fp, _, _, _ = _regime(arch, "peaked")
    _, ro, _, ao = _regime(arch, "offset")
    for name, f in (("default", fd), ("peaked", fp)):
        print(f"\n{arch} {name}: softmax per attention block:", {k: f"keys {v['keys']} logit std {v['logit_std']:.2f} row range {v['row_range']:.1f} top p {v['top_p']:.3f}"
                                                                 for k, v in f.items()})
    for name, r, a in (("default", rd, ad), ("offset", ro, ao)):
        vals = sorted(r.values())
        print(f"{arch} {name}: |group mean| / std over {len(vals)} norms: max {vals[-1]:.2f} median {vals[len(vals) // 2]:.2f}; largest |activation| {a:.1f}")
    assert len(fp) == len(fd) >= 6
    for k, v in fp.items():
        assert v["top_p"] >= 0.2 and v["row_range"] >= 10, (arch, k, v)
    assert 4 <= max(ro.values()) <= 16, max(ro.values())
    # the contrast the fixtures exist for: the default weights stay far below both windows
    assert max(v["top_p"] for v in fd.values()) < 0.2 and max(rd.values()) < 4


@pytest.mark.parametrize("arch", list(ARCHS))
def test_a_wrong_softmax_shows_block_locally_under_peaked_weights(arch):
    """sensitivity table: per attention block, the block's output with a uniform softmax and with scores x 1.05, as a share of the
    output's maximum.  Under `peaked` the uniform softmax moves the output by tenths and a 5 % error of the scores by more than one
    bf16 rounding step (2^-7 of the maximum at worst: 2^-8 relative to a value, binade width 2), so a bf16 parity bound can tell both."""
    sd_, sp = _regime(arch, "default")[2], _regime(arch, "peaked")[2]
    for name, s in (("default", sd_), ("peaked", sp)):
        print(f"\n{arch} {name}: block output moved by (uniform softmax, scores x 1.05):", {k: f"{v['uniform']:.2e}, {v['scale']:.2e}" for k, v in s.items()})
    assert set(sp) == set(sd_) and len(sp) >= 6
    for k, v in sp.items():
        assert v["uniform"] >= 0.2, (arch, k, v)
        assert v["scale"] >= 2.0**-7, (arch, k, v)
        assert v["scale"] > sd_[k]["scale"], (arch, k, v, sd_[k])


def test_attention_local_is_the_oracles_attention_on_picked_images():
    """the restated attention block against oracle.unet.attention_block / oracle.iddpm.multi_head_attention: the whole batch, and a
    subset of a batch of 8 (the IDDPM head merge reads other images' rows: attention_sources)"""
    for arch in ("ddpm", "iddpm"):
        M = OI if arch == "iddpm" else O
        cfg = OI.TINY_ATTN if arch == "iddpm" else O.TINY
        heads = cfg.num_heads if arch == "iddpm" else 1
        g = M.build_graph(cfg)
        n = next(n for n, _ in BL._walk(g)[0] if n.attn)
        sd = {k: v.double() for k, v in SW.peaked(M.make_state_dict(cfg, 3), cfg).items()}
        p = n.prefix + ".attention"
        B = 8
        x = synth.normal(7, (B, n.c_out, 4, 4)).double()
        if arch == "iddpm":
            want = OI.multi_head_attention(sd, p, x, cfg.num_groups, heads)
        else:
            want = O.attention_block(sd, p, x, cfg.num_groups)
        for pick in (list(range(B)), BL.pick_images(B), [5]):
            src = BL.attention_sources(pick, B, heads)
            figures = {}
            got = BL.attention_local(sd, p, x[src], cfg.num_groups, heads, src, pick, B, modes=(None,) + BL.MUTATIONS, figures=figures)
            assert float((got[None] - want[pick]).abs().max()) < 1e-12, (arch, pick)
            assert float((got["uniform"] - want[pick]).abs().max()) > 1e-3 and float((got["scale"] - want[pick]).abs().max()) > 1e-6
    assert BL.pick_images(128) == [0, 1, 63, 64, 126, 127] and BL.pick_images(5) == [0, 1, 2, 3, 4] and BL.pick_images(32) == [0, 1, 15, 16, 30, 31]


def test_fixtures_touch_only_what_they_name():
    for arch, (M, cfg, seed, _) in ARCHS.items():
        sd = M.make_state_dict(cfg, seed)
        heads = cfg.num_heads if arch == "iddpm" else 1
        pk, of = SW.peaked(sd, cfg), SW.offset(sd, cfg)
        for k, v in sd.items():
            if ".qkv_proj." in k:
                d = v.shape[0] // (3 * heads)
                r = (pk[k] / v).reshape(heads, 3, d, -1)
                assert torch.allclose(r[:, :2], torch.full_like(r[:, :2], 3.0)) and torch.equal(r[:, 2], torch.ones_like(r[:, 2])), k
            else:
                assert torch.equal(pk[k], v), k
            moved = k.endswith(".bias") and sd[k[:-4] + "weight"].dim() == 4 and ".qkv_proj." not in k and not k.startswith("output_conv.")
            if moved:
                dlt = (of[k] - v).reshape(cfg.num_groups, -1)
                assert torch.allclose(dlt, dlt[:, :1].sign().expand_as(dlt), atol=1e-6), k  # (+-1, one sign per group)
            else:
                assert torch.equal(of[k], v), k
        assert torch.equal(SW.offset(sd, cfg)["input_conv.bias"], of["input_conv.bias"])  # frozen stream


def test_oracle_vs_reference_under_peaked_weights(golden):
    """the oracle against the imported reference where the softmax is sharp (tests/golden/unet_peaked.npz), fp32 at 1e-5"""
    g = golden("unet_peaked")
    cfg = O.UNetConfig()
    sd = SW.peaked(O.make_state_dict(cfg, int(g["peaked_seed"])), cfg, float(g["peaked_a"]))
    x = synth.normal(int(g["peaked_xseed"]), (2, 3, 32, 32))
    cap = {}
    with torch.no_grad():
        y = O.unet_forward(sd, cfg, x, torch.from_numpy(g["peaked_t"]), capture=cap)
    np.testing.assert_allclose(y.numpy(), g["peaked_y"], atol=1e-5, rtol=0)
    keys = [k for k in g.files if k.startswith("peaked_actdigest::")]
    assert len(keys) == len(cap)
    for k in keys:
        ok, err = synth.digest_close(cap[k.split("::")[1]], g[k], atol=1e-5, rtol=1e-5)
        assert ok, (k, err)
