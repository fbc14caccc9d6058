"""-m gpu: the device random streams against the numpy reference of their contract (tests/philox_ref.py): dmme_randn,
dmme_dropout_masks, the noise dmme_chain_update draws inside the kernel, and the spans the Python side reserves from torch's
generator for gaussian(), train-mode dropout and DDPM.generate.

The normals are compared at |dz| <= 1e-6 max(1, r), r the Box-Muller radius of the element's pair: the device's logf / sinf / cosf
sit a few fp32 ulps from the fp64 reference, while a wrong counter, key or layout gives O(1) differences.  The multipliers are
compared bit for bit."""

import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O
from tests import philox_ref as P

pytestmark = pytest.mark.gpu

Z_TOL = 1e-6  # |dz| / max(1, r)
SENTINEL = -7777.25  # fills the buffer past numel: a kernel that writes there is caught
PAD = 67
WORST = {}  # measured max |dz| / max(1, r) per check, printed at the end of the module


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in WORST.items():
        print(f"\n[random streams] max |dz| / max(1, r), {k}: {v:.3e}")


def _lib():
    from dmme_amd import _lib

    return _lib


def _z_err(got, seed, offset, scale=1.0, extra_rel=0.0):
    """max |got - scale z_ref| / (scale max(1, r)), after allowing extra_rel |scale z_ref| for the rounding of the scaled value"""
    z, r = P.normals(seed, offset, got.size, with_radius=True)
    want = scale * z
    slack = extra_rel * np.abs(want)
    return float((np.maximum(np.abs(got.astype(np.float64) - want) - slack, 0.0) / (abs(scale) * np.maximum(1.0, r))).max())


def _note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), err)


# ------------------------------------------------------------------------------------------ dmme_randn
@pytest.mark.parametrize("seed", [0, 1337, 2**63 + 12345])
@pytest.mark.parametrize("offset", [0, 2**32 - 3, 2**40 + 7])
@pytest.mark.parametrize("numel", [1, 2, 3, 5, 4099, 2**21 + 3])
def test_randn_vs_reference(numel, offset, seed):
    """dmme_randn against philox_ref.normals: short spans (the partial last quad), a span across the counter's low-word carry,
    counters and keys with non-zero high words, and 2^21 + 3 values (the launch's grid-stride loop takes a second trip).
    Nothing past numel is written."""
    L = _lib()
    buf = torch.full((numel + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(L.lib().dmme_randn(L.ptr(buf), numel, seed, offset, L.stream_ptr()), "dmme_randn")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[numel:] == np.float32(SENTINEL)).all(), "dmme_randn wrote past numel"
    got = out[:numel]
    assert np.isfinite(got).all() and np.abs(got).max() <= P.MAX_ABS_Z
    err = _z_err(got, seed, offset)
    _note("dmme_randn", err)
    assert err <= Z_TOL, f"numel={numel} offset={offset} seed={seed}: max |dz| / max(1, r) = {err:.3e}"


# ------------------------------------------------------------------------------------------ dmme_dropout_masks
def _cfg(channels, num_blocks, attention, p):
    L = _lib()
    cfg = L.UNetCfg()
    t = O.TINY
    cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout = t.in_channels, t.pos_dim, t.emb_dim, t.num_groups, p
    cfg.num_depths, cfg.num_blocks, cfg.num_attention_depths = len(channels), num_blocks, len(attention)
    for i, c in enumerate(channels):
        cfg.channels_per_depth[i] = c
    for i, d in enumerate(attention):
        cfg.attention_depths[i] = d
    cfg.arch, cfg.num_heads = 0, 1
    return cfg


def _plan_numel(cfg, B):
    """dmme_unet_plan_dropmask_numel of a host-only (B, 16, 16) plan"""
    import ctypes as C

    L = _lib()
    h = C.c_void_p()
    L.check(L.lib().dmme_unet_plan_create(C.byref(cfg), B, 16, 16, L.F32, -1, C.byref(h)), "dmme_unet_plan_create")
    n = int(L.lib().dmme_unet_plan_dropmask_numel(h))
    L.lib().dmme_unet_plan_destroy(h)
    return n


def _plan_masks(cfg, B, seed, offset):
    """(numel, multipliers) of dmme_dropout_masks for a (B, 16, 16) plan of cfg; the buffer past numel must stay untouched"""
    import ctypes as C

    L = _lib()
    lib = L.lib()
    h = C.c_void_p()
    L.check(lib.dmme_unet_plan_create(C.byref(cfg), B, 16, 16, L.F32, 0, C.byref(h)), "dmme_unet_plan_create")
    try:
        n = int(lib.dmme_unet_plan_dropmask_numel(h))
        buf = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        L.check(lib.dmme_dropout_masks(h, seed, offset, L.ptr(buf), L.stream_ptr()), "dmme_dropout_masks")
        torch.cuda.synchronize()
    finally:
        lib.dmme_unet_plan_destroy(h)
    out = buf.cpu().numpy()
    assert (out[n:] == np.float32(SENTINEL)).all(), "dmme_dropout_masks wrote past the plan's mask count"
    return n, out[:n]


# TINY (428 multipliers per image: every count a multiple of 4), a one-block TINY with widths (6, 10, 14) whose count leaves a
# partial last quad, and TINY at B = 4900 (2.1 M multipliers: the grid-stride loop's second trip)
PLANS = {
    "tiny": (O.TINY.channels_per_depth, O.TINY.num_blocks, O.TINY.attention_depths, 3),
    "tiny-odd": ((6, 10, 14), 1, (2,), 1),
    "tiny-big": (O.TINY.channels_per_depth, O.TINY.num_blocks, O.TINY.attention_depths, 4900),
}


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("offset", [2**32 - 7, 2**33 + 5])
def test_dropout_masks_bit_exact_p01(plan, offset):
    channels, blocks, attention, B = PLANS[plan]
    seed = 2**63 + 12345
    key = seed ^ P.DROPOUT_KEY_XOR
    n, got = _plan_masks(_cfg(channels, blocks, attention, 0.1), B, key, offset)
    if plan == "tiny-odd":
        assert n % 4 != 0
    if plan == "tiny-big":
        assert (n + 3) // 4 > 2048 * 256
    want = P.dropout_masks(key, offset, n, 0.1)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{bad.size} of {n} multipliers differ, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


@pytest.mark.parametrize("plan", ["tiny", "tiny-odd"])
def test_dropout_masks_bit_exact_p05_and_u_equal_to_p_drops(plan):
    """p = 0.5 under the key of seed 1337: the span holds a word whose uniform is exactly 0.5, and that element is dropped"""
    channels, blocks, attention, B = PLANS[plan]
    cfg = _cfg(channels, blocks, attention, 0.5)
    n = _plan_numel(cfg, B)
    # quad k of the span is counter offset + k: put the exact-0.5 word in the span's middle
    k = n // 8
    offset = P.HALF_CTR - k
    idx = 4 * k + P.HALF_WORD
    assert offset >= 2**32 and idx < n and P.uniforms(P.HALF_KEY, offset, n)[idx] == 0.5
    n2, got = _plan_masks(cfg, B, P.HALF_KEY, offset)
    assert n2 == n
    want = P.dropout_masks(P.HALF_KEY, offset, n, 0.5)
    assert want[idx] == 0.0
    assert got[idx] == 0.0, "u == p exactly must drop (u <= p)"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert set(np.unique(got).tolist()) <= {0.0, 2.0}


# ------------------------------------------------------------------------------------------ the chain kernel's own noise
def _chain_run(proc, first, B, chw, out, seed, offset):
    """dmme_chain_update at loop index `first` on x = 0: returns (x after the update, state words i, t, offset)"""
    L = _lib()
    lib = L.lib()
    _, rows, ttab = proc._chain_tables()
    coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).cuda()
    tt = torch.tensor(ttab, dtype=torch.int64).cuda()
    state = torch.zeros(8, dtype=torch.int64, device="cuda")
    x = torch.zeros(B * chw, dtype=torch.float32, device="cuda")
    L.check(lib.dmme_chain_set(L.ptr(state), first, L.ptr(tt), seed, offset, L.stream_ptr()), "dmme_chain_set")
    L.check(lib.dmme_chain_update(proc._chain_kind, L.ptr(x), L.ptr(out), L.ptr(coef), L.ptr(tt), L.ptr(state), B, chw, L.stream_ptr()),
            "dmme_chain_update")
    torch.cuda.synchronize()
    st = [int(v) for v in state[:3].cpu()]
    return x.cpu().numpy(), st, rows


# B * chw / 4 = 524290 quads: more than one launch's 2048 x 256 threads
CHAIN_B, CHAIN_CHW = 2, 2**20 + 4


@pytest.mark.parametrize("seed,offset", [(1337, 2**32 - 1000), (2**63 + 12345, 2**40 + 3)])
@pytest.mark.parametrize("kind", ["ddpm", "iddpm"])
def test_chain_update_noise_vs_reference(kind, seed, offset):
    """x = 0 and model_out = 0 (IDDPM: eps = 0, v = 0.3) leave x = fp32(sd z) with sd = sqrt(beta_t) (DDPM) or the learned-variance
    std (IDDPM): z against the reference at the state's offset.  At t == 1 x stays 0 and the offset still advances."""
    import dmme_amd

    B, chw = CHAIN_B, CHAIN_CHW
    n4 = B * chw // 4
    if kind == "ddpm":
        proc = dmme_amd.DDPM(torch.nn.Identity(), 50)
        out = torch.zeros(B * chw, dtype=torch.float32, device="cuda")
    else:
        proc = dmme_amd.IDDPM(torch.nn.Identity(), 50)
        v = np.float32(0.3)
        out = torch.cat([torch.zeros(chw), torch.full((chw,), float(v))] * B).cuda()
    x, st, rows = _chain_run(proc, 2, B, chw, out, seed, offset)
    assert st == [1, 1, offset + n4]
    c = [np.float32(r) for r in rows[2]]
    if kind == "ddpm":
        sd, extra = float(c[2]), 2.0**-24  # the product's rounding
    else:
        f = np.float32
        e = f(f(v * c[2]) + f(f(f(1) - v) * c[3]))
        sd, extra = math.sqrt(math.exp(float(e))), 4 * 2.0**-24  # expf, sqrtf and the product's rounding
    assert sd > 0
    err = _z_err(x, seed, offset, scale=sd, extra_rel=extra)
    _note(f"dmme_chain_update ({kind})", err)
    assert err <= Z_TOL, f"{kind}: max |dz| / max(1, r) = {err:.3e}"

    x1, st1, _ = _chain_run(proc, 1, B, chw, out, seed, offset)  # t == 1: no noise added
    assert st1 == [0, 0, offset + n4]
    assert (x1 == 0).all()


# ------------------------------------------------------------------------------------------ the spans the Python side reserves
def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


@pytest.mark.parametrize("s", [1337, 2**63 + 12345])
def test_gaussian_draws_the_generator_span(s):
    """dmme_amd.gaussian after torch.manual_seed(s): the values at (initial_seed, generator offset / 4), and the offset moves by
    4 ceil(numel / 4) per call - an odd shape, then an even one"""
    import dmme_amd

    torch.manual_seed(s)
    g = _gen()
    seed = g.initial_seed()
    assert seed == s
    off = g.get_offset()
    assert off % 4 == 0
    for shape in ((3, 5, 7), (2, 3, 4, 4)):
        n = math.prod(shape)
        z = dmme_amd.gaussian(shape, device="cuda")
        assert tuple(z.shape) == shape and z.dtype == torch.float32
        assert g.get_offset() == off + 4 * ((n + 3) // 4), shape
        torch.cuda.synchronize()
        err = _z_err(z.cpu().numpy().reshape(-1), seed, off // 4)
        _note("gaussian()", err)
        assert err <= Z_TOL, (shape, err)
        off = g.get_offset()


def _tiny_net(dropout):
    import dmme_amd

    cfg = dataclasses.replace(O.TINY, dropout=dropout)  # (the state_dict's layer indices depend on whether a Dropout2d exists)
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision="fp32")
    net.load_state_dict(O.make_state_dict(cfg, 11), strict=True)
    return net.cuda()


def test_train_forward_draws_the_masks_of_its_span():
    """a train-mode forward reserves ceil(numel / 4) quads and leaves in plan.masks exactly the reference's multipliers under the
    key initial_seed ^ 0x5DEECE66D at the offset it reserved; a second forward takes the next span.  With dropout = 0 nothing is
    drawn and the generator does not move."""
    net = _tiny_net(0.1).train()
    B = 3
    x = synth.normal(1, (B, 3, 32, 32)).cuda()
    t = torch.tensor([5, 100, 900]).cuda()
    torch.manual_seed(4242)
    g = _gen()
    key = g.initial_seed() ^ P.DROPOUT_KEY_XOR
    for _ in range(2):
        off = g.get_offset()
        net(x, t)
        plan = net._plan_for(B, 32, 32, x.device)
        n = plan.dropmask_numel
        assert n == B * 428
        assert g.get_offset() == off + 4 * ((n + 3) // 4)
        torch.cuda.synchronize()
        got = plan.masks.cpu().numpy()
        want = P.dropout_masks(key, off // 4, n, 0.1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

    net0 = _tiny_net(0.0).train()
    off = g.get_offset()
    net0(x, t)
    torch.cuda.synchronize()
    assert g.get_offset() == off
    assert net0._plan_for(B, 32, 32, x.device).masks is None


def test_generate_reserves_x_T_then_one_span_per_step(monkeypatch):
    """DDPM.generate moves the generator by quads(x_T) + T quads(x), its x_T is the reference at the first span, and the chain's
    state ends at the end of the span it reserved for its T steps"""
    import dmme_amd
    from dmme_amd.diffusion_models import ddpm as ddpm_mod

    drawn = []
    real = ddpm_mod.gaussian

    def spy(*args, **kwargs):
        out = real(*args, **kwargs)
        drawn.append(out.clone())
        return out

    monkeypatch.setattr(ddpm_mod, "gaussian", spy)
    net = _tiny_net(0.1).eval()
    T, shape = 6, (2, 3, 32, 32)
    proc = dmme_amd.DDPM(net, T).cuda()
    q = math.prod(shape) // 4
    torch.manual_seed(99)
    g = _gen()
    seed, off = g.initial_seed(), g.get_offset()
    proc.generate(shape)
    torch.cuda.synchronize()
    assert g.get_offset() == off + 4 * (q + T * q)
    assert len(drawn) == 1 and tuple(drawn[0].shape) == shape
    err = _z_err(drawn[0].cpu().numpy().reshape(-1), seed, off // 4)
    _note("DDPM.generate x_T", err)
    assert err <= Z_TOL, err
    assert proc._runner is not None
    assert int(proc._runner.state[2].cpu()) == off // 4 + q + T * q
