"""-m gpu: the paper-form DDIM sampler (dmme_amd.GeneralizedDDIM) on the MI355X - the update kind DMME_CHAIN_GDDIM and its eager twin,
the captured chains in both directions, dmme_slerp and `interpolate` - against the CPU restatement tests/ddim_ref.py.

Tolerances against the restatement are not fixed numbers.  The per-step gains of a chain multiply to 1/sqrt(abar_T) (about 157 at
T = 1000), so the rounding of early steps is amplified by the chain itself; the yardstick is therefore the restatement's own
float32-versus-float64 gap on the same inputs, computed on the CPU while the test runs (oracle.unet.unet_forward as the network),
and the GPU's fp32 result may sit at 4 x that gap from the float64 result at each checked index: the convolutions sum in another
order than the CPU's at every layer, so the two float32 runs are two draws of the same rounding process, not copies.  Every
comparison prints its gap, the GPU's error and the bound; the figures measured on the MI355X are in the tests' docstrings and in DESIGN.md section 8."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import ddim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 32, 32)
ETA_NOISY = 0.7
CHAINS = [(100, 5), (1000, 50)]


def _tiny(precision="fp32", seed=11):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision=precision)
    sd = O.make_state_dict(cfg, seed)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd, cfg


def _cpu_models(seed=11):
    """oracle.unet.unet_forward over the tiny network's weights, in float32 and with the same weights widened to float64"""
    cfg = O.TINY
    sd = O.make_state_dict(cfg, seed)
    sd64 = {k: v.to(torch.float64) if v.is_floating_point() else v for k, v in sd.items()}
    return {torch.float32: lambda x, t: O.unet_forward(sd, cfg, x, t), torch.float64: lambda x, t: O.unet_forward(sd64, cfg, x, t)}


def _maxabs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _check(tag, got, ref64, ref32):
    """GPU fp32 within 4 x (the restatement's float32-vs-float64 gap) of the float64 result; returns (gap, error)"""
    gap, err = _maxabs(ref32, ref64), _maxabs(got, ref64)
    print(f"{tag}: CPU fp32-vs-fp64 gap {gap:.3e}, GPU error {err:.3e}, bound {4 * gap:.3e} (|ref|max {float(ref64.abs().max()):.3f})")
    assert bool(torch.isfinite(got).all()) and err <= 4 * gap, tag
    return gap, err


def _keep(S):
    return (S, S - 1, 2, 1)


def _inputs():
    x_T = synth.normal(41, SHAPE)
    x0 = synth.uniform(42, SHAPE)  # image-like: [-1, 1]
    return x_T, x0


@functools.lru_cache(maxsize=None)
def _reference(T, S):
    """the restatement's chains in both precisions: noisy generation with injected z, encoding, and the round trip"""
    abar, tau = R.alpha_bar(T), R.tau(T, S)
    x_T, x0 = _inputs()
    noises = {i: synth.normal(500 + i, SHAPE) for i in range(1, S + 1)}
    out = {}
    with torch.no_grad():
        for dtype, model in _cpu_models().items():
            gen = R.generate(model, x_T, abar, tau, ETA_NOISY, noises, dtype=dtype, keep=_keep(S))
            enc = R.encode(model, x0, abar, tau, dtype=dtype, keep=_keep(S))
            rt = R.decode(model, enc[-1], abar, tau, 0.0, dtype=dtype, keep=_keep(S))
            out[dtype] = dict(gen=gen, enc=enc, rt=rt)
    return out, noises


def _gen_state():
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, int(gen.get_offset())


# ------------------------------------------------------------------------------------------ 1. the update kernel alone
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_chain_update_kind5_eager_twin_and_torch_expression_are_bit_equal(eta):
    """dmme_chain_update(DMME_CHAIN_GDDIM) (scalars, index and Philox offset from device memory, noise drawn in the kernel) against
    `_ddim_update` (dmme_gddim_step fed host scalars, normals from dmme_randn through torch's generator) and against the torch fp32
    expression (k0 x + k1 eps) + k2 z with z from dmme_randn at the same offsets: bit for bit over a whole index run, in both table
    directions, with the loop state checked after every step.  At eta = 0 torch's generator is not touched."""
    import dmme_amd
    from dmme_amd import _lib

    lib = _lib.lib()
    B, shape, S = 3, (3, 3, 16, 16), 5
    proc = dmme_amd.GeneralizedDDIM(torch.nn.Identity(), 100, S, eta=eta).cuda()
    for direction, (n, rows, ttab) in (("reverse", proc._chain_tables()), ("encode", proc._encode_tables())):
        draws = direction == "reverse" and eta > 0
        coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).cuda()
        tt = torch.tensor(ttab, dtype=torch.int64).cuda()
        state = torch.zeros(8, dtype=torch.int64, device="cuda")
        x = synth.normal(1, shape).cuda()
        twin, expr = x.clone(), x.clone()
        torch.manual_seed(1234)
        torch.cuda.manual_seed(1234)
        seed, off0 = _gen_state()
        off = off0 // 4
        quads = x.numel() // 4
        _lib.check(lib.dmme_chain_set(_lib.ptr(state), S, _lib.ptr(tt), seed, off, _lib.stream_ptr()))
        for i in range(S, 0, -1):
            out = synth.normal(100 + i, (B, 3, 16, 16)).cuda()
            k0, k1, k2, _ = rows[i]
            assert (k2 != 0.0) == (draws and ttab[i - 1] != 0), (direction, i)
            _lib.check(lib.dmme_chain_update(_lib.CHAIN_GDDIM, _lib.ptr(x), _lib.ptr(out), _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state), B, 3 * 16 * 16, _lib.stream_ptr()))
            z = torch.empty_like(x)
            _lib.check(lib.dmme_randn(_lib.ptr(z), z.numel(), seed, off + (S - i) * quads, _lib.stream_ptr()))
            proc._gddim_update(twin, out, rows[i], None, draws)  # (draws from torch's generator, which sits at the same offsets)
            m = k0 * expr + k1 * out
            expr = m + k2 * z if k2 != 0.0 else m
            torch.cuda.synchronize()
            assert torch.equal(x, twin), f"{direction}: chain kind and eager twin differ at loop index {i}"
            assert torch.equal(x, expr), f"{direction}: chain kind and the torch expression differ at loop index {i}"
            st = [int(v) for v in state[:4].cpu()]
            assert st == [i - 1, ttab[i - 1], off + (S - i + 1) * quads, seed], f"{direction}: state {st} after stepping to {i - 1}"
            assert int(state[4].cpu()) & 0xFFFFFFFF == 0  # ticket back to zero
        assert _gen_state()[1] == off0 + (S * x.numel() if draws else 0), direction
    # the injected-noise form of the chain kind equals the eager twin fed the same z
    n, rows, ttab = proc._chain_tables()
    coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).cuda()
    tt = torch.tensor(ttab, dtype=torch.int64).cuda()
    state = torch.zeros(8, dtype=torch.int64, device="cuda")
    x = synth.normal(2, shape).cuda()
    twin, out, zin = x.clone(), synth.normal(3, shape).cuda(), synth.normal(4, shape).cuda()
    _lib.check(lib.dmme_chain_set(_lib.ptr(state), S, _lib.ptr(tt), 1, 0, _lib.stream_ptr()))
    _lib.check(lib.dmme_chain_update_gddim(_lib.ptr(x), _lib.ptr(out), _lib.ptr(zin), _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state), B, 3 * 16 * 16, _lib.stream_ptr()))
    proc._gddim_update(twin, out, rows[S], zin)
    torch.cuda.synchronize()
    assert torch.equal(x, twin)


# ------------------------------------------------------------------------------------------ 2. captured chain vs eager loop
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_generate_through_the_captured_step_equals_the_eager_loop(eta):
    """`generate` (one hipGraph of UNet + update + state advance, replayed S times) against the eager host loop (per-step launches,
    host scalars, dmme_randn) under the same torch seed: bit-identical.  eta = 0 takes x_T and nothing else from torch's generator,
    eta > 0 one span per step; another seed through the same graph gives other samples when eta > 0."""
    import dmme_amd

    net, _, _ = _tiny()
    S = 7
    proc = dmme_amd.GeneralizedDDIM(net, 100, S, eta=eta).cuda()
    numel = int(np.prod(SHAPE))
    torch.manual_seed(77)
    before = _gen_state()[1]
    got = proc.generate(SHAPE).clone()
    assert _gen_state()[1] - before == numel * (1 + (S if eta > 0 else 0))
    assert proc._runner is not None and (proc._runner.graph is not None or getattr(net, "_graph_disabled", False))
    torch.manual_seed(77)
    x = dmme_amd.gaussian(SHAPE, device="cuda")
    with torch.no_grad():
        for i in range(S, 0, -1):
            proc._ddim_update(x, net(x, proc.tau_tensor(i, x.device)), i)
    assert torch.equal(got, x) and bool(torch.isfinite(got).all())
    graph = proc._runner.graph
    torch.manual_seed(78)
    other = proc.generate(SHAPE)
    assert proc._runner.graph is graph  # the same captured step served the second seed
    assert not torch.equal(other, got)
    if eta > 0:  # same x_T, another noise stream
        torch.manual_seed(77)
        x_T = dmme_amd.gaussian(SHAPE, device="cuda")
        torch.manual_seed(79)
        assert not torch.equal(proc.decode(x_T), got)


def test_lit_forward_takes_the_captured_path_and_matches_sampling_step():
    import dmme_amd

    net, _, _ = _tiny()
    x = synth.normal(3, SHAPE).cuda()
    for eta in (0.0, 0.5):
        lit = dmme_amd.LitDDIM(diffusion_model=dmme_amd.GeneralizedDDIM(net, 100, 5, eta=eta)).cuda().eval()
        with torch.no_grad():
            for i in (5, 2, 1):
                torch.manual_seed(9)
                a = lit(x, i)
                torch.manual_seed(9)
                b = lit.diffusion_model.sampling_step(x, torch.tensor([i], device="cuda"))
                assert torch.equal(a, b) and a.data_ptr() != x.data_ptr(), (eta, i)
        assert lit.diffusion_model._runner_once is not None


# ------------------------------------------------------------------------------------------ 3. against the CPU restatement
@pytest.mark.parametrize("T,S", CHAINS)
def test_chains_vs_cpu_restatement(T, S):
    """Noisy generation (eta = 0.7, the z of every step injected through `zin`), encoding and the round trip decode(encode(x0)) in
    fp32 against tests/ddim_ref.py in float64, at the indices S, S-1, 2, 1 (and their mirror when encoding) and at the chain's end;
    bound: 4 x the restatement's own float32-vs-float64 gap at that index (module docstring).  The round trip is held against the
    restatement's round trip, not against x0: 50 quadratic steps discretise with about 6 % relative RMS error on their own even under
    an exact predictor, and the random-weight network here is none.

    Measured on the MI355X, largest GPU error over the checked indices with the gap at that index (gap / GPU error / bound):
      (100, 5):   generate 1.47e-6 / 1.87e-6 / 5.87e-6, encode 5.77e-7 / 6.04e-7 / 2.31e-6, round trip 1.11e-6 / 1.95e-6 / 4.42e-6
      (1000, 50): generate 4.46e-4 / 4.46e-4 / 1.78e-3 (|x| reaches 650 under the random weights), encode 3.56e-6 / 3.06e-6 / 1.42e-5,
                  round trip 5.50e-4 / 7.02e-4 / 2.20e-3 (|x| reaches 160)
    The largest GPU error / gap ratio over every checked index was 1.9 (round trip (100, 5), index 2), against the 4 allowed."""
    import dmme_amd
    from dmme_amd import _lib

    lib = _lib.lib()
    ref, noises = _reference(T, S)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    net, _, _ = _tiny()
    x_T, x0 = _inputs()
    worst = {}

    def note(kind, gap_err):
        worst[kind] = max(worst.get(kind, (0.0, 0.0)), gap_err, key=lambda v: v[1])

    # noisy generation, eager launches with the noise injected (a captured step has one fixed `zin` address)
    proc = dmme_amd.GeneralizedDDIM(net, T, S, eta=ETA_NOISY).cuda()
    n, rows, ttab = proc._chain_tables()
    coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).cuda()
    tt = torch.tensor(ttab, dtype=torch.int64).cuda()
    state = torch.zeros(8, dtype=torch.int64, device="cuda")
    x = x_T.cuda()
    _lib.check(lib.dmme_chain_set(_lib.ptr(state), S, _lib.ptr(tt), 0, 0, _lib.stream_ptr()))
    with torch.no_grad():
        for i in range(S, 0, -1):
            eps = net(x, proc.tau_tensor(i, x.device)).contiguous()
            _lib.check(lib.dmme_chain_update_gddim(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(noises[i].cuda()), _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state),
                                                   SHAPE[0], int(np.prod(SHAPE[1:])), _lib.stream_ptr()))
            if i in _keep(S):
                note("generate", _check(f"generate ({T},{S}) eta {ETA_NOISY} after index {i}", x, r64["gen"][i], r32["gen"][i]))
    # encoding, through the captured step over the reversed tables
    det = dmme_amd.GeneralizedDDIM(net, T, S).cuda()
    runner = det._encode_runner(SHAPE, torch.device("cuda", torch.cuda.current_device()))
    runner.x.copy_(x0.cuda())
    runner.set(S, 0, 0)
    for j in range(S, 0, -1):
        runner.step()
        i = S - j + 1  # the state is now x_{tau_i}
        if i in _keep(S):
            note("encode", _check(f"encode ({T},{S}) x_tau_{i}", runner.x, r64["enc"][i], r32["enc"][i]))
    torch.cuda.synchronize()
    stepped = runner.x.clone()
    latent = det.encode(x0.cuda())
    assert torch.equal(latent, stepped)
    # the round trip: decode what the GPU encoded
    dec = det.chain_runner(latent.clone())
    dec.set(S, 0, 0)
    for i in range(S, 0, -1):
        dec.step()
        if i in _keep(S):
            note("round trip", _check(f"round trip ({T},{S}) after index {i}", dec.x, r64["rt"][i], r32["rt"][i]))
    back = det.decode(latent)
    assert torch.equal(back, dec.x)
    _check(f"decode(encode(x0)) ({T},{S})", back, r64["rt"][0], r32["rt"][0])
    rel = float((back.cpu() - x0).pow(2).mean().sqrt() / x0.pow(2).mean().sqrt())
    print(f"({T},{S}) round trip vs x0 itself: relative RMS {rel:.3e} (a random-weight network is no noise predictor: not held to a bound)")
    print(f"({T},{S}) largest GPU error per chain (gap, error):", {k: (f"{g:.2e}", f"{e:.2e}") for k, (g, e) in worst.items()})


# ------------------------------------------------------------------------------------------ 4. partial runs
@pytest.mark.parametrize("T,S,k", [(100, 5, 3), (1000, 50, 20)])
def test_partial_encode_and_decode(T, S, k):
    """decode(encode(x0, upto=k), start=k) against the same two half-chains of the restatement (bound as in test 3)"""
    import dmme_amd

    abar, tau = R.alpha_bar(T), R.tau(T, S)
    _, x0 = _inputs()
    refs = {}
    with torch.no_grad():
        for dtype, model in _cpu_models().items():
            mid = R.encode(model, x0, abar, tau, upto=k, dtype=dtype)[-1]
            refs[dtype] = (mid, R.decode(model, mid, abar, tau, 0.0, start=k, dtype=dtype)[0])
    net, _, _ = _tiny()
    det = dmme_amd.GeneralizedDDIM(net, T, S).cuda()
    mid = det.encode(x0.cuda(), upto=k)
    _check(f"encode upto {k} ({T},{S})", mid, refs[torch.float64][0], refs[torch.float32][0])
    _check(f"decode start {k} ({T},{S})", det.decode(mid, start=k), refs[torch.float64][1], refs[torch.float32][1])
    assert torch.equal(det.encode(x0.cuda(), upto=0), x0.cuda()) and torch.equal(det.decode(mid, start=0), mid)


# ------------------------------------------------------------------------------------------ 5. dmme_slerp
def _gpu_slerp(xa, xb, w):
    from dmme_amd import _lib

    a, b = xa.cuda().contiguous(), xb.cuda().contiguous()
    wd = torch.tensor(w, dtype=torch.float32).cuda()
    out = torch.full((len(w),) + tuple(a.shape), float("nan"), device="cuda")
    _lib.check(_lib.lib().dmme_slerp(_lib.ptr(a), _lib.ptr(b), _lib.ptr(wd), len(w), a.shape[0], a[0].numel(), _lib.ptr(out), _lib.stream_ptr()), "dmme_slerp")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [32, 64])
def test_slerp_vs_float64(B, hw):
    """dmme_slerp against the float64 restatement; bound: 4 x the gap between the restatement evaluated in float32 numpy and in
    float64 (largest over the outputs).  synth.normal latents: in >= 3072 dimensions |cos theta| stays far from 1 (asserted < 0.2),
    so acos is well conditioned.  w = 0 / w = 1 return xa / xb, and xa == xb (theta = 0: the linear form) returns xa, to that bound.

    Measured on the MI355X (gap / GPU error / bound): B=1 32x32 3.72e-7 / 2.78e-7 / 1.49e-6, B=3 32x32 3.76e-7 / 2.78e-7 / 1.51e-6,
    B=1 64x64 4.04e-7 / 2.58e-7 / 1.62e-6, B=3 64x64 6.13e-7 / 3.46e-7 / 2.45e-6; xa == xb: 2.38e-7 / 2.38e-7 / 9.54e-7 (B=1 32x32:
    gap 4.77e-7)."""
    w = [0.0, 0.25, 0.5, 0.8, 1.0]
    shape = (B, 3, hw, hw)
    xa, xb = synth.normal(60 + B, shape), synth.normal(70 + hw, shape)
    a64, b64 = xa.double().reshape(B, -1), xb.double().reshape(B, -1)
    cos = (a64 * b64).sum(1) / (a64.norm(dim=1) * b64.norm(dim=1))
    assert float(cos.abs().max()) < 0.2
    ref64 = torch.from_numpy(R.slerp(xa.numpy(), xb.numpy(), w, np.float64))
    ref32 = torch.from_numpy(R.slerp(xa.numpy(), xb.numpy(), w, np.float32))
    got = _gpu_slerp(xa, xb, w)
    assert got.shape == (len(w),) + shape
    gap, _ = _check(f"slerp B={B} {hw}x{hw}", got, ref64, ref32)
    assert _maxabs(got[0], xa) <= 4 * gap and _maxabs(got[-1], xb) <= 4 * gap
    same64 = torch.from_numpy(R.slerp(xa.numpy(), xa.numpy(), w, np.float64))
    same32 = torch.from_numpy(R.slerp(xa.numpy(), xa.numpy(), w, np.float32))
    got = _gpu_slerp(xa, xa, w)
    gap, _ = _check(f"slerp xa == xb B={B} {hw}x{hw}", got, same64, same32)
    assert _maxabs(got, xa.expand_as(got)) <= 4 * gap + _maxabs(same64, xa.double().expand_as(same64))


def test_slerp_many_weights_and_a_large_image():
    """more weights than one tile (64) holds, and batch 1 at 3 x 256 x 256 (the several-blocks-per-image reduction): same yardstick"""
    w = [float(v) for v in np.linspace(0.0, 1.0, 70)]
    xa, xb = synth.normal(81, (2, 3, 16, 16)), synth.normal(82, (2, 3, 16, 16))
    _check("slerp n=70", _gpu_slerp(xa, xb, w), torch.from_numpy(R.slerp(xa.numpy(), xb.numpy(), w, np.float64)),
           torch.from_numpy(R.slerp(xa.numpy(), xb.numpy(), w, np.float32)))
    w = [0.0, 0.3, 1.0]
    xa, xb = synth.normal(83, (1, 3, 256, 256)), synth.normal(84, (1, 3, 256, 256))
    _check("slerp 3x256x256", _gpu_slerp(xa, xb, w), torch.from_numpy(R.slerp(xa.numpy(), xb.numpy(), w, np.float64)),
           torch.from_numpy(R.slerp(xa.numpy(), xb.numpy(), w, np.float32)))


# ------------------------------------------------------------------------------------------ 6. interpolate
def test_interpolate_vs_composed_restatement():
    """shape, finiteness, the endpoints (weights 0 and 1 give decode(encode(xa)) and decode(encode(xb))) and the whole pipeline
    encode -> slerp -> decode against the restatement's, each within 4 x the restatement's float32-vs-float64 gap"""
    import dmme_amd

    T, S, w = 100, 5, [0.0, 0.3, 1.0]
    abar, tau = R.alpha_bar(T), R.tau(T, S)
    xa, xb = synth.uniform(91, SHAPE), synth.uniform(92, SHAPE)
    refs = {}
    with torch.no_grad():
        for dtype, model in _cpu_models().items():
            npdt = np.float32 if dtype == torch.float32 else np.float64
            la, lb = R.encode(model, xa, abar, tau, dtype=dtype)[-1], R.encode(model, xb, abar, tau, dtype=dtype)[-1]
            lat = torch.from_numpy(R.slerp(la.numpy(), lb.numpy(), w, npdt))
            out = R.decode(model, lat.reshape((-1,) + SHAPE[1:]), abar, tau, 0.0, dtype=dtype)[0].reshape(lat.shape)
            ends = [R.decode(model, l, abar, tau, 0.0, dtype=dtype)[0] for l in (la, lb)]
            refs[dtype] = (out, ends)
    net, _, _ = _tiny()
    det = dmme_amd.GeneralizedDDIM(net, T, S).cuda()
    got = det.interpolate(xa.cuda(), xb.cuda(), w)
    assert got.shape == (len(w),) + SHAPE and bool(torch.isfinite(got).all())
    _check("interpolate, whole pipeline", got, refs[torch.float64][0], refs[torch.float32][0])
    for j, k, x in ((0, 0, xa), (-1, 1, xb)):
        _check(f"interpolate endpoint {k} vs the restatement's round trip", got[j], refs[torch.float64][1][k], refs[torch.float32][1][k])
        gap = _maxabs(refs[torch.float32][1][k], refs[torch.float64][1][k])
        assert _maxabs(got[j], det.decode(det.encode(x.cuda()))) <= 4 * gap, k  # (a batch of n x B against a batch of B)
    with pytest.raises(ValueError):
        det.interpolate(xa.cuda(), xb[:1].cuda(), w)


# ------------------------------------------------------------------------------------------ 7. 16-bit plans
@pytest.mark.parametrize("precision,budget", [("bf16", 1.0e-2), ("fp16", 1.5e-3)])
def test_16bit_generate_against_the_fp32_run(precision, budget):
    """one 5-step eta = 0 chain on the default UNet in bf16 / fp16 against the fp32 plan from the same x_T.  The existing 16-bit
    chain tests assert finiteness and bit-reproducibility; the numeric budgets they rest on are the per-evaluation relative-RMS
    bounds of the default UNet (tests/test_gpu_unet.py: BF16_REL_RMS = 1.0e-2, tests/test_gpu_fp16.py: FP16_REL_RMS = 1.5e-3).
    A chain of S evaluations is held to S x that budget, relative to the RMS of the fp32 result: every step adds k1 eps with
    |k1| < 1 and eps of the state's own magnitude, and the gains k0 of the (100, 5) table multiply to 1.7 in all, so S budgets
    cover the S evaluations with room for what the network does to an already perturbed input.
    Measured on the MI355X: bf16 1.40e-3 (bound 5.0e-2), fp16 1.81e-4 (bound 7.5e-3)."""
    import dmme_amd

    T, S = 100, 5
    sd = O.make_state_dict(O.UNetConfig(), 21)
    outs = {}
    for prec in ("fp32", precision):
        net = dmme_amd.UNet(precision=prec)
        net.load_state_dict(sd, strict=True)
        proc = dmme_amd.GeneralizedDDIM(net.cuda().eval(), T, S).cuda()
        runs = []
        for _ in range(2):
            torch.manual_seed(5)
            runs.append(proc.generate(SHAPE).clone())
        assert bool(torch.isfinite(runs[0]).all()) and torch.equal(runs[0], runs[1])  # (what the existing 16-bit chain tests assert)
        outs[prec] = runs[0]
    rel = float((outs[precision] - outs["fp32"]).pow(2).mean().sqrt() / outs["fp32"].pow(2).mean().sqrt())
    print(f"{precision} vs fp32, 5-step chain: relative RMS {rel:.3e} (bound {S * budget:.1e})")
    assert rel <= S * budget


# ------------------------------------------------------------------------------------------ 8. the trainer's sample command
def test_trainer_sample_with_the_paper_sampler():
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "dmme_amd.trainer", "sample", "--config", os.path.join(ROOT, "configs", "ddim", "cifar10.yaml"),
           "--sampler", "ddim-paper", "--eta", "0.5", "--num-images", "4"]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=660)
    assert res.returncode == 0, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    rec = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["images"] == [4, 3, 32, 32] and rec["finite"] is True
