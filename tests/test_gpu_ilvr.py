"""-m gpu: ILVR (dmme_amd.ILVR) on the MI355X - the low-pass filter dmme_lowpass against float64 under a derived elementwise bound, the
fused form against the streaming form bit for bit, the update against its float64 expression under a derived bound, the identities that
tie the step to DDPM's update, the eager twin against the chain form (normals, loop state), the captured chains against the eager loops
and against the CPU restatement tests/ilvr_ref.py, and the refusals.

Bounds (tests/ilvr_ref.py: filter_bound, update_bound) are derived from the precision of fp32 and the lengths of the two dot products, not
measured; tests/test_ilvr_host.py shows on the CPU that a plain fp32 evaluation sits well inside them.  Against the restatement the
yardstick is the one of tests/test_gpu_repaint.py: the GPU's fp32 result may sit at 4 x the restatement's own float32-versus-float64 gap
from the float64 result.  Every comparison prints its figures."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import ilvr_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 32, 32)
CHAINS = [(100, 8, 4, 0), (1000, 20, 8, 5)]  # (T, sub_timesteps, N, range_level)


def _lib():
    from dmme_amd import _lib

    return _lib


def _filters(H, W, N):
    import dmme_amd

    return tuple(torch.from_numpy(dmme_amd.lowpass_matrix(n, N).astype(np.float32)).cuda() for n in (H, W))


def _scratch(planes, H, W):
    return torch.empty(int(_lib().lib().dmme_lowpass_scratch_bytes(planes, H, W)) // 4, dtype=torch.float32, device="cuda")


def _fused(H, W):
    return H * W <= int(_lib().lib().dmme_lowpass_lds_capacity())


def _lowpass(src, dst, Ph, Pw, scratch=None, force=0):
    L = _lib()
    planes, H, W = src.shape
    L.check(L.lib().dmme_lowpass(L.ptr(src), L.ptr(dst), planes, H, W, L.ptr(Ph), L.ptr(Pw), L.ptr(scratch), force, L.stream_ptr()), "dmme_lowpass")
    return dst


def _eager(x, out, ref, z2, row, Ph, Pw, scratch=None, planes=1, force=0):
    L = _lib()
    B, Cc, H, W = x.shape
    L.check(L.lib().dmme_ilvr_step(L.ptr(x), L.ptr(out), L.ptr(ref), L.ptr(z2), (C.c_float * 8)(*row), L.ptr(Ph), L.ptr(Pw), L.ptr(scratch), B, Cc, H, W, planes,
                                   force, L.stream_ptr()), "dmme_ilvr_step")
    return x


def _chain_update(x, out, ref, noise, Ph, Pw, tabs, scratch=None, planes=1, force=0):
    L = _lib()
    B, Cc, H, W = x.shape
    L.check(L.lib().dmme_chain_update_ilvr(L.ptr(x), L.ptr(out), L.ptr(ref), L.ptr(noise), L.ptr(Ph), L.ptr(Pw), L.ptr(scratch), L.ptr(tabs.coef), L.ptr(tabs.ttab),
                                           L.ptr(tabs.state), B, Cc, H, W, planes, force, L.stream_ptr()), "dmme_chain_update_ilvr")
    return x


def _randn2(shape, seed, off):
    """the [2, *shape] block of one step: dmme_randn of 2 * numel values at quad offset `off`"""
    L = _lib()
    z = torch.empty((2,) + tuple(shape), dtype=torch.float32, device="cuda")
    L.check(L.lib().dmme_randn(L.ptr(z), z.numel(), seed, off, L.stream_ptr()))
    return z


class _Tables:
    def __init__(self, rows, ttab):
        self.coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).cuda()
        self.ttab = torch.tensor(ttab, dtype=torch.int64).cuda()
        self.state = torch.zeros(8, dtype=torch.int64, device="cuda")

    def set(self, i, seed, off):
        L = _lib()
        L.check(L.lib().dmme_chain_set(L.ptr(self.state), i, L.ptr(self.ttab), seed, off, L.stream_ptr()))

    def words(self):
        torch.cuda.synchronize()
        return [int(v) for v in self.state.cpu()]


def _gen_offset():
    return int(torch.cuda.default_generators[torch.cuda.current_device()].get_offset())


# ------------------------------------------------------------------------------------------ 1. the filter alone
@pytest.mark.parametrize("planes,H,W,N", [(6, 8, 8, 2), (6, 12, 20, 4), (3, 32, 32, 8), (3, 64, 64, 4), (3, 256, 256, 32)])
def test_lowpass_vs_float64(planes, H, W, N):
    """dmme_lowpass on 3 randn + 0.7 against Ph x Pw^T in float64 over the same fp32-rounded tables, elementwise inside
    (H + W + 8) 2^-24 (|Ph| |x| |Pw|^T); 12 x 20 is not square, so exchanged tables would show; 256 x 256 takes the streaming form on
    its own, the others the fused one (no scratch given).  In place (dst == src) gives the bits of out of place."""
    Ph, Pw = _filters(H, W, N)
    src = (3.0 * torch.randn(planes, H, W, generator=torch.Generator().manual_seed(3)) + 0.7).cuda()
    scratch = None if _fused(H, W) else _scratch(planes, H, W)
    assert _fused(H, W) == (H <= 64)
    got = _lowpass(src, torch.empty_like(src), Ph, Pw, scratch)
    torch.cuda.synchronize()
    want = Ph.double().cpu() @ src.double().cpu() @ Pw.double().cpu().T
    bound = R.filter_bound(src, Ph, Pw)
    err = (got.double().cpu() - want).abs()
    print(f"lowpass {planes}x{H}x{W}/{N}: max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    inplace = src.clone()
    _lowpass(inplace, inplace, Ph, Pw, scratch)
    assert torch.equal(inplace, got)


# ------------------------------------------------------------------------------------------ 2. fused = streaming
@pytest.mark.parametrize("B,H,W,N", [(2, 12, 20, 4), (1, 32, 32, 8)])
def test_fused_equals_streaming(B, H, W, N):
    """force_streaming = 1 on planes the fused form holds: the same bits from dmme_lowpass (6 / 3 planes) and from dmme_chain_update_ilvr
    drawing its own normals, on an interior row, the last row and an unconditioned row; the loop state moves alike"""
    shape = (B, 3, H, W)
    planes = 3 * B
    Ph, Pw = _filters(H, W, N)
    scratch = _scratch(planes, H, W)
    src = (3.0 * torch.randn(planes, H, W, generator=torch.Generator().manual_seed(4)) + 0.7).cuda()
    a = _lowpass(src, torch.empty_like(src), Ph, Pw)
    b = _lowpass(src, torch.empty_like(src), Ph, Pw, scratch, force=1)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    rows = R.update_rows(N)
    table = [rows["interior"]] * 2 + [rows["last"], rows["unconditioned"]]  # loop indices 1 (interior), 2, 3
    tabs = _Tables(table, [0, 10, 20, 30])
    x0, e, y = (synth.normal(s, shape).cuda() for s in (1, 2, 3))
    numel = x0.numel()
    for i in (1, 2, 3):
        got = []
        for force in (0, 1):
            x = x0.clone()
            tabs.set(i, 99, 7)
            _chain_update(x, e, y, None, Ph, Pw, tabs, scratch, force=force)
            assert tabs.words()[:5] == [i - 1, [0, 10, 20, 30][i - 1], 7 + 2 * (numel // 4), 99, 0]
            got.append(x)
        assert torch.equal(got[0], got[1]) and bool(torch.isfinite(got[0]).all()) and not torch.equal(got[0], x0), i


# ------------------------------------------------------------------------------------------ 3. the update against float64
@pytest.mark.parametrize("B,H,W,N", [(2, 8, 8, 2), (2, 12, 20, 4), (1, 32, 32, 8)])
def test_update_vs_float64_expression(B, H, W, N):
    """dmme_ilvr_step and dmme_chain_update_ilvr (both streams given) against tests/ilvr_ref.py's step in float64 over the fp32 rows and
    tables, elementwise inside 2^-24 [8 A + (H + W + 16) (|Ph| A |Pw|^T)], on an interior step, the last step (c2 = ks = 0) and an
    unconditioned step (g = 0)"""
    shape = (B, 3, H, W)
    Ph, Pw = _filters(H, W, N)
    g = torch.Generator().manual_seed(11)
    x0, e, y = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    z2 = torch.randn((2,) + shape, generator=g).cuda()
    for name, row in R.update_rows(N).items():
        want = R.step(x0.cpu(), e.cpu(), y.cpu(), z2.cpu(), row, Ph.double().cpu(), Pw.double().cpu(), torch.float64)
        bound = R.update_bound(x0, e, y, z2, row, Ph, Pw)
        eager = _eager(x0.clone(), e, y, z2, row, Ph, Pw)
        tabs = _Tables([row, row], [0, 50])
        tabs.set(1, 5, 0)
        chain = _chain_update(x0.clone(), e, y, z2, Ph, Pw, tabs)
        torch.cuda.synchronize()
        err = (eager.double().cpu() - want).abs()
        print(f"update {shape}/{N} {name}: max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
        assert bool(torch.isfinite(eager).all()) and bool((err <= bound).all()), name
        assert torch.equal(eager, chain), name


# ------------------------------------------------------------------------------------------ 4. identities
def test_identities():
    """(a) g = 0: the step is dmme_ddpm_step on the same z0 and dmme_chain_update(DMME_CHAIN_DDPM) under the same seed and offset, bit for
    bit, on the full grid at an interior timestep and at t = 1.  (b) ka = 1, ks = 0 and y = that u: d = 0 exactly and x' == u.
    (c) a stream whose coefficient is 0 may hold NaN in the given block without changing the result."""
    import dmme_amd

    L = _lib()
    lib = L.lib()
    shape, N = (2, 3, 12, 20), 4
    numel = int(np.prod(shape))
    Ph, Pw = _filters(12, 20, N)
    proc = dmme_amd.ILVR(torch.nn.Identity(), 100, 100, N, 100)  # the full grid, no step conditioned
    n, rows, ttab = proc._chain_tables()
    ddpm = dmme_amd.DDPM(torch.nn.Identity(), 100)
    dn, drows, dttab = ddpm._chain_tables()
    assert n == dn == 100 and ttab == dttab and all(r[5] == 0.0 for r in rows)
    x0, e, y = (synth.normal(s, shape).cuda() for s in (1, 2, 3))
    seed, off = 21, 1000
    z2 = _randn2(shape, seed, off)
    tabs, dtabs = _Tables(rows, ttab), _Tables(drows, dttab)
    for t in (57, 1):
        a = _eager(x0.clone(), e, y, z2, rows[t], Ph, Pw)
        b = x0.clone()
        L.check(lib.dmme_ddpm_step(L.ptr(b), L.ptr(e), L.ptr(z2[0]), ddpm._c1[t], ddpm._c2[t], ddpm._sigma[t], int(t != 1), numel, L.stream_ptr()))
        tabs.set(t, seed, off)
        c = _chain_update(x0.clone(), e, y, None, Ph, Pw, tabs)
        dtabs.set(t, seed, off)
        d = x0.clone()
        L.check(lib.dmme_chain_update(L.CHAIN_DDPM, L.ptr(d), L.ptr(e), L.ptr(dtabs.coef), L.ptr(dtabs.ttab), L.ptr(dtabs.state), shape[0], numel // shape[0],
                                      L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(c, d) and torch.equal(a, c) and bool(torch.isfinite(a).all()), t
        # (b): the reference is u itself at level b with ka = 1, ks = 0
        row = list(rows[t])
        row[3:6] = [1.0, 0.0, 1.0]
        assert torch.equal(_eager(x0.clone(), e, a, z2, row, Ph, Pw), a), t
        moved = _eager(x0.clone(), e, y, z2, row, Ph, Pw)
        assert not torch.equal(moved, a) and bool(torch.isfinite(moved).all())  # (with another reference the same row does move x)
    # (c)
    nan = torch.full_like(z2, float("nan"))
    cond = dmme_amd.ILVR(torch.nn.Identity(), 100, 10, N, 0)._chain_tables()[1]
    last, interior = cond[1], cond[8]
    assert last[2] == 0.0 and last[4] == 0.0 and last[5] == 1.0
    want = _eager(x0.clone(), e, y, None, last, Ph, Pw)
    assert torch.equal(_eager(x0.clone(), e, y, nan, last, Ph, Pw), want) and bool(torch.isfinite(want).all())
    half = z2.clone()
    half[1] = float("nan")
    free = list(interior)
    free[5] = 0.0  # unconditioned: z1 is not touched
    assert torch.equal(_eager(x0.clone(), e, y, half, free, Ph, Pw), _eager(x0.clone(), e, y, z2, free, Ph, Pw))
    only_k = list(interior)
    only_k[2] = 0.0  # no reverse noise: z0 is not touched
    half = z2.clone()
    half[0] = float("nan")
    got = _eager(x0.clone(), e, y, half, only_k, Ph, Pw)
    assert torch.equal(got, _eager(x0.clone(), e, y, z2, only_k, Ph, Pw)) and bool(torch.isfinite(got).all())
    tabs = _Tables([only_k, only_k], [0, 50])
    tabs.set(1, 5, 0)
    assert torch.equal(_chain_update(x0.clone(), e, y, half, Ph, Pw, tabs), got)


# ------------------------------------------------------------------------------------------ 5. eager = chain
@pytest.mark.parametrize("shape,N", [((2, 3, 12, 20), 4), ((2, 3, 32, 32), 4)])
def test_eager_twin_equals_the_chain_form(shape, N):
    """dmme_chain_update_ilvr drawing in the kernel (row and index from device memory) against dmme_ilvr_step fed dmme_randn(2 * numel) at
    the offset the state stood at, bit for bit after every step of two whole walks of 6 levels: every step conditioned (the last one, from
    i = 1, too), and range_level = 3 (three unconditioned steps).  The loop state after every step: i - 1, t_table[i - 1], the offset moved
    by 2 n4 whatever the step drew, the seed, the ticket back at zero, the other words as they were.  Then a network output of two planes
    per image: the eps plane is the one used."""
    import dmme_amd

    Ph, Pw = _filters(shape[2], shape[3], N)
    numel = int(np.prod(shape))
    n4, seed, off0 = numel // 4, 77, (1 << 33) + 5  # (a counter kept in 32 bits would draw other normals)
    y = (0.5 * synth.normal(5, shape)).cuda()
    for r in (0, 3):
        n, rows, ttab = dmme_amd.ILVR(torch.nn.Identity(), 100, 6, N, r)._chain_tables()
        assert n == 6 and [rw[5] for rw in rows[1:]] == [1.0 if i - 1 >= r else 0.0 for i in range(1, 7)]
        tabs = _Tables(rows, ttab)
        x = synth.normal(1, shape).cuda()
        twin = x.clone()
        tabs.set(n, seed, off0)
        tabs.state[5:] = torch.tensor([41, 42, 43], device="cuda")
        for k, i in enumerate(range(n, 0, -1)):
            out = synth.normal(100 + i, shape).cuda()
            z2 = _randn2(shape, seed, off0 + 2 * n4 * k)
            _chain_update(x, out, y, None, Ph, Pw, tabs)
            _eager(twin, out, y, z2, rows[i], Ph, Pw)
            assert tabs.words() == [i - 1, ttab[i - 1], off0 + 2 * n4 * (k + 1), seed, 0, 41, 42, 43], i
            assert torch.equal(x, twin), f"chain form and eager twin differ at loop index {i} (range_level {r})"
            assert bool(torch.isfinite(x).all())
    Cc = shape[1]
    two = synth.normal(3, (shape[0], 2 * Cc) + shape[2:]).cuda()
    one = two[:, :Cc].contiguous()
    x, twin, want = (synth.normal(2, shape).cuda() for _ in range(3))
    tabs.set(n, seed, 0)
    for k, i in enumerate((n, n - 1)):
        z2 = _randn2(shape, seed, 2 * n4 * k)
        _chain_update(x, two, y, None, Ph, Pw, tabs, planes=2)
        _eager(twin, two, y, z2, rows[i], Ph, Pw, planes=2)
        _eager(want, one, y, z2, rows[i], Ph, Pw)
    torch.cuda.synchronize()
    assert torch.equal(x, want) and torch.equal(twin, want)


# ------------------------------------------------------------------------------------------ 6. chains on the tiny UNet
def _tiny(seed=11):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision="fp32")
    net.load_state_dict(O.make_state_dict(cfg, seed), strict=True)
    return net.cuda().eval()


def _cpu_models(seed=11):
    cfg = O.TINY
    sd = O.make_state_dict(cfg, seed)
    sd64 = {k: v.to(torch.float64) if v.is_floating_point() else v for k, v in sd.items()}
    return {torch.float32: lambda x, t: O.unet_forward(sd, cfg, x, t), torch.float64: lambda x, t: O.unet_forward(sd64, cfg, x, t)}


def _image(seed):
    return (0.5 * synth.normal(seed, SHAPE)).clamp(-1.0, 1.0)


def _maxabs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def test_captured_chain_equals_the_eager_loop():
    """`sample_like` (one hipGraph of UNet + two draws + the fused update + state advance, replayed) against the host loop over
    dmme_ilvr_step, bit for bit under the same seed; torch's generator moves by x_T plus 2 numel per step either way; a second chain on the
    same runner re-uses the graph; `generate` conditions nothing and equals its eager loop; `low_pass` is dmme_lowpass"""
    import dmme_amd

    net = _tiny()
    proc = dmme_amd.ILVR(net, 100, 8, 4, 2).cuda()
    numel, y = int(np.prod(SHAPE)), _image(42).cuda()
    torch.manual_seed(77)
    before = _gen_offset()
    a = proc.sample_like(y)
    assert _gen_offset() - before == numel + 2 * numel * proc.n_levels
    runner, graph = proc._runner, proc._runner.graph
    assert isinstance(runner, dmme_amd.LikeChainRunner) and runner.capture_error is None and graph is not None and runner.noise_numel == 2 * numel
    torch.manual_seed(78)
    b = proc.sample_like(y)
    assert proc._runner is runner and runner.graph is graph and not torch.equal(a, b)
    with torch.no_grad():
        for seed, got in ((77, a), (78, b)):
            torch.manual_seed(seed)
            before = _gen_offset()
            x = dmme_amd.gaussian(SHAPE, device="cuda")
            assert torch.equal(got, proc._eager_chain(x, y)) and bool(torch.isfinite(got).all())
            assert _gen_offset() - before == numel + 2 * numel * proc.n_levels
        torch.manual_seed(77)
        gen = proc.generate(SHAPE)
        torch.manual_seed(77)
        want = proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), torch.zeros(SHAPE, device="cuda"), proc._free_tables)
        assert torch.equal(gen, want) and not torch.equal(gen, a) and proc._free_runner.graph is not None
    Ph, Pw = _filters(32, 32, 4)
    assert torch.equal(proc.low_pass(y), _lowpass(y.reshape(6, 32, 32), torch.empty(6, 32, 32, device="cuda"), Ph, Pw).reshape(SHAPE))


@functools.lru_cache(maxsize=None)
def _reference(T, n, N, r, seed, off):
    """the restatement in float32 and float64 on the normals the device draws for (seed, off), copied to the host"""
    abar = R.alpha_bar(T)
    g = R.grid(abar, n)
    L = len(g) - 1
    x_T, y = synth.normal(41, SHAPE), _image(42)
    numel = int(np.prod(SHAPE))
    normals = torch.cat([_randn2(SHAPE, seed, off + 2 * (numel // 4) * k).cpu().unsqueeze(0) for k in range(L)])
    keep = {L, L - 1, 2, 1}
    with torch.no_grad():
        ref = {dtype: R.sample_like(model, x_T, y, abar, g, N, r, normals, dtype, keep) for dtype, model in _cpu_models().items()}
    return ref, g, x_T, y


@pytest.mark.parametrize("T,n,N,r", CHAINS)
def test_chains_vs_cpu_restatement(T, n, N, r):
    """the ILVR walk on the tiny UNet in fp32, stepped through the captured graph with in-kernel draws, against tests/ilvr_ref.py in float64
    on the same normals (oracle.unet.unet_forward as the network) at the first two and last two loop indices.  Bound: 4 x the
    restatement's float32-vs-float64 gap at that index.  `sample_like` from the same x_T under the same seed returns the stepped chain's bits."""
    import dmme_amd
    from dmme_amd.common.noise import philox_reserve

    net = _tiny()
    proc = dmme_amd.ILVR(net, T, n, N, r).cuda()
    numel = int(np.prod(SHAPE))
    torch.manual_seed(5)
    x_T_dev = dmme_amd.gaussian(SHAPE, device="cuda")  # (the draw `sample_like` makes first under this seed)
    L = proc.n_levels
    seed, off = philox_reserve(x_T_dev.device, 2 * numel * L)
    ref, g, x_T, y = _reference(T, n, N, r, seed, off)
    assert proc._tau_host == g and L == len(g) - 1
    runner = proc.chain_runner(x_T.cuda().clone())
    assert isinstance(runner, dmme_amd.LikeChainRunner)
    runner.ref.copy_(y)
    runner.set(L, seed, off)
    worst = (0.0, 0.0)
    for i in range(L, 0, -1):
        runner.step()
        if i in (L, L - 1, 2, 1):
            gap, err = _maxabs(ref[torch.float32][i], ref[torch.float64][i]), _maxabs(runner.x, ref[torch.float64][i])
            print(f"ILVR ({T},{n},{N},{r}) after index {i}: CPU fp32-vs-fp64 gap {gap:.3e}, GPU error {err:.3e}, bound {4 * gap:.3e} "
                  f"(|ref|max {float(ref[torch.float64][i].abs().max()):.3f})")
            assert bool(torch.isfinite(runner.x).all()) and err <= 4 * gap, i
            worst = max(worst, (gap, err), key=lambda v: v[1])
    torch.cuda.synchronize()
    assert runner.capture_error is None and runner.graph is not None
    print(f"({T},{n},{N},{r}) largest GPU error (gap, error): {worst[0]:.2e}, {worst[1]:.2e}")
    runner.x.copy_(x_T_dev)
    runner.set(L, seed, off)
    for _ in range(L):
        runner.step()
    torch.manual_seed(5)
    got = proc.sample_like(y)
    assert torch.equal(got, runner.x) and got.data_ptr() != runner.x.data_ptr()


def test_v_prediction_with_static_threshold_and_history():
    """a prediction="v" process with threshold="static": the adapter and the thresholding stage run in front of the update in the captured
    step as in the eager loop, the two chains agree bit for bit and differ from the eps process's; a HistoryRecorder with vis_length 4
    records 4 frames, and recording does not change the chain"""
    import dmme_amd

    net = _tiny()
    proc = dmme_amd.ILVR(net, 100, 8, 4, 0, prediction="v", threshold="static").cuda()
    plain = dmme_amd.ILVR(net, 100, 8, 4, 0).cuda()
    y = _image(42).cuda()
    torch.manual_seed(9)
    a = proc.sample_like(y)
    assert proc._runner.capture_error is None and proc._runner.graph is not None
    torch.manual_seed(9)
    with torch.no_grad():
        want = proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), y)
    assert torch.equal(a, want) and bool(torch.isfinite(a).all())
    torch.manual_seed(9)
    assert not torch.equal(plain.sample_like(y), a)
    ords = dmme_amd.history_ordinals(proc.chain_length(), 4)
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    torch.manual_seed(9)
    b = proc.sample_like(y, history=rec)
    assert rec.recorded == 4 == len(ords) and torch.equal(a, b)
    torch.manual_seed(9)
    rec2 = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    with torch.no_grad():
        proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), y, history=rec2)
    torch.cuda.synchronize()
    assert rec2.recorded == 4 and torch.equal(rec.canvas, rec2.canvas)


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    """the library's error, not a launch: a conditional plan, a classifier plan, chw % 4 != 0, null scratch where the streaming form would
    run, kind 11 handed to dmme_chain_step"""
    import dmme_amd

    L = _lib()
    lib = L.lib()
    net = _tiny()
    proc = dmme_amd.ILVR(net, 100, 8, 4, 0).cuda()
    x = synth.normal(1, SHAPE).cuda()
    runner = proc.chain_runner(x)
    packed = net._packed_for(runner.plan, fold=True)
    runner.set(8, 1, 0)

    def step(plan):
        return lib.dmme_ilvr_chain_step(plan.h, L.ptr(packed), L.ptr(runner.x), L.ptr(runner.out), L.ptr(plan.workspace), L.ptr(runner.ref), L.ptr(runner.Ph),
                                        L.ptr(runner.Pw), L.ptr(runner.scratch), L.ptr(runner.coef), L.ptr(runner.ttab), L.ptr(runner.state), L.stream_ptr())

    before = x.clone()
    tiny_kw = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    cnet = dmme_amd.ConditionalUNet(precision="fp32", num_classes=5, dropout=0.0, **tiny_kw).cuda().eval()
    assert step(cnet._plan_for(2, 32, 32, x.device)) == -1 and b"class-conditional plan" in lib.dmme_last_error()
    cls = dmme_amd.EncoderClassifier(precision="fp32", num_classes=5, **tiny_kw).cuda().eval()
    assert step(cls._plan_for(2, 32, 32, x.device)) == -1 and b"predicts no noise" in lib.dmme_last_error()
    assert lib.dmme_chain_step(runner.plan.h, L.ptr(packed), L.ptr(runner.x), L.ptr(runner.out), L.ptr(runner.plan.workspace), L.CHAIN_ILVR, L.ptr(runner.coef),
                               L.ptr(runner.ttab), L.ptr(runner.state), L.stream_ptr()) == -1 and b"chain_step: sampler kind 11" in lib.dmme_last_error()
    # the update's own checks
    row = (C.c_float * 8)(*proc._chain_tables()[1][8])
    z = torch.zeros(2 * 3 * 5 * 5 * 2, device="cuda")
    odd = torch.zeros(2, 3, 5, 5, device="cuda")
    assert lib.dmme_ilvr_step(L.ptr(odd), L.ptr(odd), L.ptr(odd), L.ptr(z), row, L.ptr(runner.Ph), L.ptr(runner.Pw), None, 2, 3, 5, 5, 1, 0, L.stream_ptr()) == -2
    assert b"multiple of 4" in lib.dmme_last_error()
    Ph, Pw = _filters(32, 32, 4)
    z2 = torch.zeros((2,) + SHAPE, device="cuda")
    assert lib.dmme_ilvr_step(L.ptr(x), L.ptr(runner.out), L.ptr(runner.ref), L.ptr(z2), row, L.ptr(Ph), L.ptr(Pw), None, 2, 3, 32, 32, 1, 1, L.stream_ptr()) == -1
    assert b"scratch" in lib.dmme_last_error()
    big = torch.zeros(1, 128, 128, device="cuda")
    Pb = _filters(128, 128, 4)
    assert lib.dmme_lowpass(L.ptr(big), L.ptr(big), 1, 128, 128, L.ptr(Pb[0]), L.ptr(Pb[1]), None, 0, L.stream_ptr()) == -1 and b"scratch" in lib.dmme_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before)  # nothing was launched on x
