"""-m gpu: DDNM (dmme_amd.DDNM) on the MI355X - the measurement dmme_ddnm_measure against float64 under the mean's bound, the update
against its float64 expression under a derived bound, the identities (an unmeasured cell ignores y, the last row makes the result
consistent with the measurement, unused streams are not read, the eps plane of a two-plane output), the eager twin against the chain
form (normals, loop state), the captured chains against the eager loops and against the CPU restatement tests/ddnm_ref.py, the end-to-end
consistency of restored images, and the refusals.

Bounds (tests/ddnm_ref.py: mean_bound, update_bound, consistency_bound) are derived from the precision of fp32 and the size of a cell,
not measured; tests/test_ddnm_host.py shows on the CPU that a plain fp32 evaluation sits inside them.  Against the restatement the
yardstick is the one of tests/test_gpu_repaint.py: the GPU's fp32 result may sit at 4 x the restatement's own float32-versus-float64 gap
from the float64 result.  Every comparison prints its figures."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import ddnm_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 32, 32)
CHAINS = [(100, 8, 4, False, 0.0, (1, 1), False), (1000, 12, 2, True, 0.1, (3, 2), True)]  # (T, sub_timesteps, s, gray, sigma_y, travel, masked)


def _lib():
    from dmme_amd import _lib

    return _lib


def _mshape(shape, s, gray):
    return (shape[0], 1 if gray else shape[1], shape[2] // s, shape[3] // s)


def _binary(shape, seed, p=0.7):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < p).float()


def _measure(x, mask, s, gray):
    L = _lib()
    B, Cc, H, W = x.shape
    y = torch.full(_mshape(x.shape, s, gray), float("nan"), device="cuda")
    L.check(L.lib().dmme_ddnm_measure(L.ptr(x), L.ptr(mask), L.ptr(y), B, Cc, H, W, s, int(gray), L.stream_ptr()), "dmme_ddnm_measure")
    return y


def _eager(x, out, y, m, z2, row, s, gray, planes=1):
    L = _lib()
    B, Cc, H, W = x.shape
    L.check(L.lib().dmme_ddnm_step(L.ptr(x), L.ptr(out), L.ptr(y), L.ptr(m), L.ptr(z2), (C.c_float * 8)(*row), B, Cc, H, W, s, int(gray), planes, L.stream_ptr()),
            "dmme_ddnm_step")
    return x


def _chain_update(x, out, y, m, noise, tabs, s, gray, planes=1):
    L = _lib()
    B, Cc, H, W = x.shape
    L.check(L.lib().dmme_chain_update_ddnm(L.ptr(x), L.ptr(out), L.ptr(y), L.ptr(m), L.ptr(noise), L.ptr(tabs.coef), L.ptr(tabs.ttab), L.ptr(tabs.state), B, Cc, H, W,
                                           s, int(gray), planes, L.stream_ptr()), "dmme_chain_update_ddnm")
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


# ------------------------------------------------------------------------------------------ 1. the measurement alone
@pytest.mark.parametrize("shape,s,gray", [((2, 3, 8, 8), 2, False), ((2, 3, 10, 20), 5, False), ((2, 3, 12, 20), 1, True), ((1, 3, 32, 32), 8, True),
                                          ((1, 3, 64, 256), 32, True)])
def test_measure_vs_float64(shape, s, gray):
    """dmme_ddnm_measure on 3 randn + 0.7 against M o Pool_s o Gray_g in float64, per cell inside (n + 1) 2^-24 max_cell |x|, under a random
    binary mask and with no mask; 10 x 20 at s = 5 has quads that straddle cells, 64 x 256 at s = 32 a band of 24576 values; an
    unmeasured cell gives exactly 0; the same image at another place of a larger batch gives the same bits"""
    x = (3.0 * torch.randn(shape, generator=torch.Generator().manual_seed(3)) + 0.7).cuda()
    m = _binary(_mshape(shape, s, gray), 5)
    m.view(-1)[0], m.view(-1)[-1] = 0.0, 1.0
    m = m.cuda()
    bound = R.mean_bound(x, s, gray)
    for mask in (m, None):
        got = _measure(x, mask, s, gray)
        torch.cuda.synchronize()
        want = R.A(x.double().cpu(), s, gray, None if mask is None else mask.double().cpu())
        err = (got.double().cpu() - want).abs()
        print(f"measure {shape} s {s} gray {gray} mask {mask is not None}: max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
        if mask is not None:
            assert bool((got[mask == 0] == 0).all()) and bool((mask == 0).any())
    three = torch.cat([x.flip(0), x, x])[: shape[0] + 2].contiguous()
    again = _measure(three, None, s, gray)
    assert torch.equal(again[shape[0]:shape[0] + 1], _measure(x, None, s, gray)[:1])


def test_a_band_above_the_capacity_is_refused():
    L = _lib()
    lib = L.lib()
    cap = int(lib.dmme_ddnm_band_capacity())
    assert 3 * 32 * 256 <= cap < 3 * 32 * 512
    x = torch.ones(1, 3, 32, 512, device="cuda")
    y = torch.full((1, 1, 1, 16), 7.0, device="cuda")
    assert lib.dmme_ddnm_measure(L.ptr(x), None, L.ptr(y), 1, 3, 32, 512, 32, 1, L.stream_ptr()) == -2 and str(cap).encode() in lib.dmme_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())  # nothing was launched


# ------------------------------------------------------------------------------------------ 2. the update against float64
@pytest.mark.parametrize("shape,s,gray", [((2, 3, 8, 8), 2, False), ((2, 3, 10, 20), 5, False), ((1, 3, 32, 32), 4, True), ((2, 3, 12, 20), 1, False)])
def test_update_vs_float64_expression(shape, s, gray):
    """dmme_ddnm_step and dmme_chain_update_ddnm (both streams given) against tests/ddnm_ref.py's step in float64 over the fp32 rows,
    elementwise inside `update_bound`, on an interior step, the last step, a step with a folded jump (r1 != 0) and a step with
    lambda < 1; 12 x 20 at s = 1 takes the quad form.  The two forms agree bit for bit."""
    g = torch.Generator().manual_seed(11)
    x0, e = (torch.randn(shape, generator=g).cuda() for _ in range(2))
    z2 = torch.randn((2,) + shape, generator=g).cuda()
    ms = _mshape(shape, s, gray)
    y = torch.randn(ms, generator=g).cuda()
    m = _binary(ms, 12).cuda()
    for name, row in R.update_rows().items():
        want = R.step(x0.cpu(), e.cpu(), y.cpu(), m.cpu(), z2.cpu(), row, s, gray, torch.float64)
        bound = R.update_bound(x0, e, y, m, z2, row, s, gray)
        eager = _eager(x0.clone(), e, y, m, z2, row, s, gray)
        tabs = _Tables([row, row], [0, 50])
        tabs.set(1, 5, 0)
        chain = _chain_update(x0.clone(), e, y, m, z2, tabs, s, gray)
        torch.cuda.synchronize()
        err = (eager.double().cpu() - want).abs()
        print(f"update {shape} s {s} gray {gray} {name}: max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
        assert bool(torch.isfinite(eager).all()) and bool((err <= bound).all()), name
        assert torch.equal(eager, chain), name


# ------------------------------------------------------------------------------------------ 3. identities
@pytest.mark.parametrize("shape,s,gray", [((2, 3, 10, 20), 5, False), ((2, 3, 8, 8), 2, True), ((2, 3, 12, 20), 1, False)])
def test_identities(shape, s, gray):
    """(a) m = 0 everywhere and y = NaN: the bits of lambda = 0 with a finite y.  (b) the last row at sigma_y = 0 on any x / eps:
    dmme_ddnm_measure of the result equals y on measured cells inside `consistency_bound`, and unmeasured cells keep x0 bit for bit.
    (c) NaN in a stream whose coefficient is 0 changes nothing.  (d) a two-plane output uses the eps plane."""
    rows = R.update_rows()
    g = torch.Generator().manual_seed(21)
    x, e = (torch.randn(shape, generator=g).cuda() for _ in range(2))
    z2 = torch.randn((2,) + shape, generator=g).cuda()
    ms = _mshape(shape, s, gray)
    y = torch.randn(ms, generator=g).cuda()
    m = _binary(ms, 22).cuda()
    # (a)
    for name in ("interior", "travel"):
        row = list(rows[name])
        got = _eager(x.clone(), e, torch.full_like(y, float("nan")), torch.zeros_like(m), z2, row, s, gray)
        row[5] = 0.0
        want = _eager(x.clone(), e, y, torch.ones_like(m), z2, row, s, gray)
        assert torch.equal(got, want) and bool(torch.isfinite(got).all()), name
    # (b)
    last = rows["last"]
    xh = _eager(x.clone(), e, y, m, None, last, s, gray)
    x0 = R.x0_of(x.cpu(), e.cpu(), last, torch.float32).cuda()
    back = _measure(xh, None, s, gray)
    torch.cuda.synchronize()
    bound = R.consistency_bound(x0, xh, y, s, gray)
    err = (back.double().cpu() - y.double().cpu()).abs()
    meas = (m != 0).cpu()
    print(f"consistency {shape} s {s} gray {gray}: max |A xh - y| on measured cells {float(err[meas].max()):.3e}, largest err / bound {float((err / bound)[meas].max()):.3f}")
    assert bool((err[meas] <= bound[meas]).all()) and bool(meas.any()) and bool((~meas).any())
    free = R.replicate(m, s, gray, shape[1]) == 0
    assert torch.equal(xh[free], x0[free]) and not torch.equal(xh[~free], x0[~free])
    # (c)
    nan = torch.full_like(z2, float("nan"))
    assert torch.equal(_eager(x.clone(), e, y, m, nan, last, s, gray), xh)
    half = z2.clone()
    half[1] = float("nan")
    want = _eager(x.clone(), e, y, m, z2, rows["interior"], s, gray)
    assert torch.equal(_eager(x.clone(), e, y, m, half, rows["interior"], s, gray), want) and bool(torch.isfinite(want).all())
    only_jump = list(rows["travel"])
    only_jump[2] = 0.0
    half = z2.clone()
    half[0] = float("nan")
    want = _eager(x.clone(), e, y, m, z2, only_jump, s, gray)
    assert torch.equal(_eager(x.clone(), e, y, m, half, only_jump, s, gray), want) and bool(torch.isfinite(want).all())
    tabs = _Tables([only_jump, only_jump], [0, 50])
    tabs.set(1, 5, 0)
    assert torch.equal(_chain_update(x.clone(), e, y, m, half, tabs, s, gray), want)
    # (d)
    Cc = shape[1]
    two = torch.randn((shape[0], 2 * Cc) + shape[2:], generator=g).cuda()
    one = two[:, :Cc].contiguous()
    want = _eager(x.clone(), one, y, m, z2, rows["interior"], s, gray)
    assert torch.equal(_eager(x.clone(), two, y, m, z2, rows["interior"], s, gray, planes=2), want)


# ------------------------------------------------------------------------------------------ 4. eager = chain
@pytest.mark.parametrize("shape,s,gray", [((2, 3, 10, 20), 5, False), ((2, 3, 32, 32), 4, True), ((2, 3, 12, 20), 1, False)])
def test_eager_twin_equals_the_chain_form(shape, s, gray):
    """dmme_chain_update_ddnm drawing in the kernel (row and index from device memory) against dmme_ddnm_step fed dmme_randn(2 * numel) at
    the offset the state stood at, bit for bit after every step of a walk of 6 levels with travel 2 / 2 (rows with and without a jump,
    the last row), from an offset above 2^32.  The loop state after every step: i - 1, t_table[i - 1], the offset moved by 2 n4 whatever
    the step drew, the seed, the ticket back at zero, the other words as they were."""
    import dmme_amd

    numel = int(np.prod(shape))
    n4, seed, off0 = numel // 4, 77, (1 << 33) + 5  # (a counter kept in 32 bits would draw other normals)
    ms = _mshape(shape, s, gray)
    y = (0.5 * synth.normal(5, ms)).cuda()
    m = _binary(ms, 6).cuda()
    n, rows, ttab = dmme_amd.DDNM(torch.nn.Identity(), 100, 6, travel_length=2, travel_repeat=2)._chain_tables()
    assert n == len(R.transitions(dmme_amd.repaint_levels(6, 2, 2))) > 6 and any(r[7] != 0.0 for r in rows) and rows[1][2] == 0.0
    tabs = _Tables(rows, ttab)
    x = synth.normal(1, shape).cuda()
    twin = x.clone()
    tabs.set(n, seed, off0)
    tabs.state[5:] = torch.tensor([41, 42, 43], device="cuda")
    for k, i in enumerate(range(n, 0, -1)):
        out = synth.normal(100 + i, shape).cuda()
        z2 = _randn2(shape, seed, off0 + 2 * n4 * k)
        _chain_update(x, out, y, m, None, tabs, s, gray)
        _eager(twin, out, y, m, z2, rows[i], s, gray)
        assert tabs.words() == [i - 1, ttab[i - 1], off0 + 2 * n4 * (k + 1), seed, 0, 41, 42, 43], i
        assert torch.equal(x, twin), f"chain form and eager twin differ at loop index {i}"
        assert bool(torch.isfinite(x).all())


# ------------------------------------------------------------------------------------------ 5. chains on the tiny UNet
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


@pytest.mark.parametrize("kw", [dict(), dict(prediction="v", threshold="static")])
def test_captured_chain_equals_the_eager_loop(kw):
    """`restore` (one hipGraph of UNet + two draws + the band update + state advance, replayed) against the host loop over dmme_ddnm_step,
    bit for bit under the same seed; torch's generator moves by x_T plus 2 numel per step either way; a second chain on the same runner
    re-uses the graph; `generate` measures nothing and equals its eager loop; `degrade` is dmme_ddnm_measure.  Again with a v network
    under static thresholding, and with a HistoryRecorder, which changes nothing."""
    import dmme_amd

    net = _tiny()
    proc = dmme_amd.DDNM(net, 100, 8, scale=4, travel_length=2, travel_repeat=2, **kw).cuda()
    numel, img = int(np.prod(SHAPE)), _image(42).cuda()
    y = proc.degrade(img)
    assert torch.equal(y, _measure(img, None, 4, False)) and tuple(y.shape) == (2, 3, 8, 8)
    m = _binary(tuple(y.shape), 9).cuda()
    torch.manual_seed(77)
    before = _gen_offset()
    a = proc.restore(y, m)
    assert _gen_offset() - before == numel + 2 * numel * proc.n_rows and proc.n_rows > proc.n_levels
    runner, graph = proc._runner, proc._runner.graph
    assert isinstance(runner, dmme_amd.RestoreChainRunner) and runner.capture_error is None and graph is not None and runner.noise_numel == 2 * numel
    torch.manual_seed(78)
    b = proc.restore(y, m)
    assert proc._runner is runner and runner.graph is graph and not torch.equal(a, b) and tuple(a.shape) == SHAPE
    with torch.no_grad():
        for seed, got in ((77, a), (78, b)):
            torch.manual_seed(seed)
            before = _gen_offset()
            x = dmme_amd.gaussian(SHAPE, device="cuda")
            assert torch.equal(got, proc._eager_chain(x, y, m)) and bool(torch.isfinite(got).all())
            assert _gen_offset() - before == numel + 2 * numel * proc.n_rows
        torch.manual_seed(77)
        gen = proc.generate(SHAPE)
        torch.manual_seed(77)
        zeros = torch.zeros_like(y)
        want = proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), zeros, zeros)
        assert torch.equal(gen, want) and not torch.equal(gen, a) and proc._runner is runner
    ords = dmme_amd.history_ordinals(proc.chain_length(), 4)
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    torch.manual_seed(77)
    c = proc.restore(y, m, history=rec)
    assert rec.recorded == 4 == len(ords) and torch.equal(a, c)
    torch.manual_seed(77)
    rec2 = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    with torch.no_grad():
        proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), y, m, history=rec2)
    torch.cuda.synchronize()
    assert rec2.recorded == 4 and torch.equal(rec.canvas, rec2.canvas)
    if kw:
        torch.manual_seed(77)
        assert not torch.equal(dmme_amd.DDNM(net, 100, 8, scale=4, travel_length=2, travel_repeat=2).cuda().restore(y, m), a)


@functools.lru_cache(maxsize=None)
def _reference(T, n, s, gray, sigma_y, travel, masked, seed, off):
    """the restatement in float32 and float64 on the normals the device draws for (seed, off), copied to the host"""
    import dmme_amd

    abar = R.alpha_bar(T)
    g = R.grid(abar, n)
    tab, ttab = R.rows(abar, g, dmme_amd.repaint_levels(len(g) - 1, *travel), sigma_y)
    L = len(ttab) - 1
    x_T = synth.normal(41, SHAPE)
    ms = _mshape(SHAPE, s, gray)
    m = _binary(ms, 43) if masked else torch.ones(ms)
    y = R.A(_image(42).double(), s, gray, m.double()).float() + sigma_y * synth.normal(44, ms)
    numel = int(np.prod(SHAPE))
    normals = torch.cat([_randn2(SHAPE, seed, off + 2 * (numel // 4) * k).cpu().unsqueeze(0) for k in range(L)])
    keep = {L, L - 1, 2, 1}
    with torch.no_grad():
        ref = {dtype: R.chain(model, x_T, y, m, tab, ttab, normals, s, gray, dtype, keep) for dtype, model in _cpu_models().items()}
    return ref, ttab, x_T, y, m


@pytest.mark.parametrize("T,n,s,gray,sigma_y,travel,masked", CHAINS)
def test_chains_vs_cpu_restatement(T, n, s, gray, sigma_y, travel, masked):
    """the DDNM walk on the tiny UNet in fp32, stepped through the captured graph with in-kernel draws, against tests/ddnm_ref.py in float64
    on the same normals (oracle.unet.unet_forward as the network) at the first two and last two loop indices.  Bound: 4 x the
    restatement's float32-vs-float64 gap at that index.  `restore` from the same x_T under the same seed returns the stepped chain's bits."""
    import dmme_amd
    from dmme_amd.common.noise import philox_reserve

    net = _tiny()
    proc = dmme_amd.DDNM(net, T, n, scale=s, gray=gray, sigma_y=sigma_y, travel_length=travel[0], travel_repeat=travel[1]).cuda()
    numel = int(np.prod(SHAPE))
    torch.manual_seed(5)
    x_T_dev = dmme_amd.gaussian(SHAPE, device="cuda")  # (the draw `restore` makes first under this seed)
    L = proc.n_rows
    seed, off = philox_reserve(x_T_dev.device, 2 * numel * L)
    ref, ttab, x_T, y, m = _reference(T, n, s, gray, sigma_y, travel, masked, seed, off)
    assert proc._chain_tables()[2] == ttab and L == len(ttab) - 1
    runner = proc.chain_runner(x_T.cuda().clone())
    assert isinstance(runner, dmme_amd.RestoreChainRunner)
    runner.y.copy_(y)
    runner.mask.copy_(m)
    runner.set(L, seed, off)
    worst = (0.0, 0.0)
    for i in range(L, 0, -1):
        runner.step()
        if i in (L, L - 1, 2, 1):
            gap, err = _maxabs(ref[torch.float32][i], ref[torch.float64][i]), _maxabs(runner.x, ref[torch.float64][i])
            print(f"DDNM ({T},{n},{s},{gray},{sigma_y},{travel}) after index {i}: CPU fp32-vs-fp64 gap {gap:.3e}, GPU error {err:.3e}, bound {4 * gap:.3e} "
                  f"(|ref|max {float(ref[torch.float64][i].abs().max()):.3f})")
            assert bool(torch.isfinite(runner.x).all()) and err <= 4 * gap, i
            worst = max(worst, (gap, err), key=lambda v: v[1])
    torch.cuda.synchronize()
    assert runner.capture_error is None and runner.graph is not None
    print(f"({T},{n},{s},{gray}) largest GPU error (gap, error): {worst[0]:.2e}, {worst[1]:.2e}")
    runner.x.copy_(x_T_dev)
    runner.set(L, seed, off)
    for _ in range(L):
        runner.step()
    torch.manual_seed(5)
    got = proc.restore(y.cuda(), m.cuda())
    assert torch.equal(got, runner.x) and got.data_ptr() != runner.x.data_ptr()


# ------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("s,gray,masked", [(4, False, False), (1, True, False), (2, True, True)])
def test_restored_images_reproduce_the_measurement(s, gray, masked):
    """super-resolution x 4, colourisation and masked grey x 2 at sigma_y = 0 on the tiny UNet: `degrade(restore(y))` equals y on measured
    cells inside `consistency_bound`, whose M takes the last step's x0 (from the network output the runner holds) and the result"""
    import dmme_amd
    from dmme_amd.common.noise import philox_reserve

    net = _tiny()
    proc = dmme_amd.DDNM(net, 100, 8, scale=s, gray=gray).cuda()
    ms = _mshape(SHAPE, s, gray)
    m = (_binary(ms, 31) if masked else torch.ones(ms)).cuda()
    y = proc.degrade(_image(42).cuda(), m)
    torch.manual_seed(3)
    got = proc.restore(y, m)
    assert tuple(got.shape) == SHAPE and bool(torch.isfinite(got).all())
    # the same chain stepped by hand, to look at the last step's operands
    torch.manual_seed(3)
    x_T = dmme_amd.gaussian(SHAPE, device="cuda")
    runner = proc._runner
    L = proc.n_rows
    seed, off = philox_reserve(x_T.device, 2 * x_T.numel() * L)
    runner.x.copy_(x_T)
    runner.set(L, seed, off)
    for _ in range(L - 1):
        runner.step()
    before = runner.x.clone()
    runner.step()
    torch.cuda.synchronize()
    assert torch.equal(runner.x, got)
    x0 = R.x0_of(before.cpu(), runner.out[:, :3].cpu(), proc._chain_tables()[1][1], torch.float32)
    back = proc.degrade(got)
    bound = R.consistency_bound(x0, got, y, s, gray)
    err = (back.double().cpu() - y.double().cpu()).abs()
    meas = (m != 0).cpu()
    print(f"restore s {s} gray {gray} masked {masked}: max |A x - y| on measured cells {float(err[meas].max()):.3e}, largest err / bound "
          f"{float((err / bound)[meas].max()):.3f}, |y|max {float(y.abs().max()):.3f}")
    assert bool((err[meas] <= bound[meas]).all())
    assert float((got - proc.pinv(y, m).cuda()).abs().max()) > 1e-3  # (the null-space part is the network's, not zero)


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    """the library's error, not a launch: a conditional plan, a classifier plan, kind 12 handed to dmme_chain_step, chw % 4 != 0, a scale
    that does not divide H; x unchanged afterwards"""
    import dmme_amd

    L = _lib()
    lib = L.lib()
    net = _tiny()
    proc = dmme_amd.DDNM(net, 100, 8, scale=4).cuda()
    x = synth.normal(1, SHAPE).cuda()
    runner = proc.chain_runner(x)
    packed = net._packed_for(runner.plan, fold=True)
    runner.set(8, 1, 0)

    def step(plan, s=4):
        return lib.dmme_ddnm_chain_step(plan.h, L.ptr(packed), L.ptr(runner.x), L.ptr(runner.out), L.ptr(plan.workspace), L.ptr(runner.y), L.ptr(runner.mask), s, 0,
                                        L.ptr(runner.coef), L.ptr(runner.ttab), L.ptr(runner.state), L.stream_ptr())

    before = x.clone()
    tiny_kw = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    cnet = dmme_amd.ConditionalUNet(precision="fp32", num_classes=5, dropout=0.0, **tiny_kw).cuda().eval()
    assert step(cnet._plan_for(2, 32, 32, x.device)) == -1 and b"class-conditional plan" in lib.dmme_last_error()
    cls = dmme_amd.EncoderClassifier(precision="fp32", num_classes=5, **tiny_kw).cuda().eval()
    assert step(cls._plan_for(2, 32, 32, x.device)) == -1 and b"predicts no noise" in lib.dmme_last_error()
    assert lib.dmme_chain_step(runner.plan.h, L.ptr(packed), L.ptr(runner.x), L.ptr(runner.out), L.ptr(runner.plan.workspace), L.CHAIN_DDNM, L.ptr(runner.coef),
                               L.ptr(runner.ttab), L.ptr(runner.state), L.stream_ptr()) == -1 and b"chain_step: sampler kind 12" in lib.dmme_last_error()
    # the update's own checks
    row = (C.c_float * 8)(*proc._chain_tables()[1][8])
    z = torch.zeros(2 * 2 * 3 * 5 * 5, device="cuda")
    odd = torch.zeros(2, 3, 5, 5, device="cuda")
    assert lib.dmme_ddnm_step(L.ptr(odd), L.ptr(odd), L.ptr(odd), L.ptr(odd), L.ptr(z), row, 2, 3, 5, 5, 1, 0, 1, L.stream_ptr()) == -2
    assert b"multiples of 4" in lib.dmme_last_error()
    z2 = torch.zeros((2,) + SHAPE, device="cuda")
    assert lib.dmme_ddnm_step(L.ptr(x), L.ptr(runner.out), L.ptr(runner.y), L.ptr(runner.mask), L.ptr(z2), row, 2, 3, 32, 32, 5, 0, 1, L.stream_ptr()) == -1
    assert b"does not divide" in lib.dmme_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before)  # nothing was launched on x
