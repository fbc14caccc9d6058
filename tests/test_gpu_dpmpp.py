"""-m gpu: DPM-Solver++(2M) (dmme_amd.DPMSolverPP / ClassifierFreeDPMSolver) on the MI355X - the update kinds DMME_CHAIN_DPMPP /
DMME_CHAIN_DPMPP_CFG and their eager twins bit for bit against an fp32 torch expression, the history buffer and the loop state's
"history valid" flag, the captured chains against the eager loops, and whole chains against the CPU restatement tests/dpmpp_ref.py.

Against the restatement the yardstick is tests/test_gpu_ddim_paper.py's: the restatement's own float32-versus-float64 gap on the same
inputs (oracle.unet.unet_forward as the network), computed on the CPU while the test runs; the GPU's fp32 result may sit at 4 x that
gap from the float64 result at each checked index.  Every comparison prints gap, error and bound."""

import functools

import numpy as np
import pytest
import torch

from oracle import iddpm as OI
from oracle import synth
from oracle import unet as O

from . import cond_ref as CR
from . import dpmpp_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 32, 32)
CHAINS = [(100, 5), (1000, 20)]
NAN = float("nan")


def _tiny(seed=11):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision="fp32")
    sd = O.make_state_dict(cfg, seed)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def _cpu_models(seed=11):
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


def _keep(n):
    return sorted({n, n - 1, 2, 1} & set(range(1, n + 1)))


def _gen_offset():
    return int(torch.cuda.default_generators[torch.cuda.current_device()].get_offset())


def _expr(x, e, prev, row, valid):
    """the fp32 torch expression of one update: separate kernels, so every product and sum rounds on its own; returns (x', x0)"""
    q0, q1, k0, k1, w, clip = row[:6]
    x0 = q0 * x + q1 * e
    if clip != 0.0:
        x0 = x0.clamp(-1.0, 1.0)
    d = x0 + w * (x0 - prev) if valid else x0
    return k0 * x + k1 * d, x0


def _mix(ec, eu, s):
    return eu + s * (ec - eu)


class _Tables:
    def __init__(self, rows, ttab):
        self.coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).cuda()
        self.ttab = torch.tensor(ttab, dtype=torch.int64).cuda()
        self.state = torch.zeros(8, dtype=torch.int64, device="cuda")

    def set(self, i, seed, off):
        from dmme_amd import _lib

        _lib.check(_lib.lib().dmme_chain_set(_lib.ptr(self.state), i, _lib.ptr(self.ttab), seed, off, _lib.stream_ptr()))

    def words(self):
        torch.cuda.synchronize()
        return [int(v) for v in self.state.cpu()]


# ------------------------------------------------------------------------------------------ 1. the update alone
@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (1, 3, 4, 4)])  # 576 quads in three blocks (the ticket counts); one partial block
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("clip", [False, True])
def test_chain_update_eager_twin_and_torch_expression_are_bit_equal(shape, order, clip):
    """dmme_chain_update_dpmpp (row, index and flag from device memory) against dmme_dpmpp_step (host scalars, the flag as an argument)
    and the fp32 torch expression, bit for bit after every step of a whole index run: x and the history.  The history starts as NaN
    (it must not be read while the flag is clear) and everything stays finite.  The loop state after every step: i, t, the Philox
    offset unchanged, the seed, the ticket back at zero, the flag set.  A second run placed mid-table takes a first-order first step
    whatever the table's w says."""
    import dmme_amd
    from dmme_amd import _lib

    lib = _lib.lib()
    proc = dmme_amd.DPMSolverPP(torch.nn.Identity(), 100, 5, order=order, clip_x0=clip).cuda()
    n, rows, ttab = proc._chain_tables()
    assert n == 5 and (order == 1 or rows[n - 2][4] > 0.0)
    B, chw = shape[0], int(np.prod(shape[1:]))
    tabs = _Tables(rows, ttab)
    for start in (n, n - 2):
        x = synth.normal(1, shape).cuda()
        twin, expr = x.clone(), x.clone()
        hist = torch.full(shape, NAN, device="cuda")
        hist_twin, prev = hist.clone(), None
        tabs.set(start, 77, 1234)
        assert tabs.words()[:6] == [start, ttab[start], 1234, 77, 0, 0]
        for i in range(start, 0, -1):
            out = synth.normal(100 + i, shape).cuda()
            valid = i < start
            _lib.check(lib.dmme_chain_update_dpmpp(_lib.ptr(x), _lib.ptr(out), _lib.ptr(hist), _lib.ptr(tabs.coef), _lib.ptr(tabs.ttab), _lib.ptr(tabs.state),
                                                   B, chw, 1, _lib.stream_ptr()))
            proc._dpm_update(twin, out, i, hist_twin, valid)
            expr, prev = _expr(expr, out, prev, rows[i], valid)
            assert tabs.words()[:6] == [i - 1, ttab[i - 1], 1234, 77, 0, 1], (start, i)
            assert torch.equal(x, twin) and torch.equal(hist, hist_twin), f"chain kind and eager twin differ at loop index {i} (start {start})"
            assert torch.equal(x, expr) and torch.equal(hist, prev), f"chain kind and the torch expression differ at loop index {i} (start {start})"
            assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(hist).all())
            if clip:
                assert float(hist.abs().max()) <= 1.0
        assert torch.equal(x, hist)  # the chain ends on x0
    # an IDDPM network's output: (eps, v) planes per image, the eps plane is the one used
    x = synth.normal(2, shape).cuda()
    two = synth.normal(3, (B, 2 * shape[1]) + shape[2:]).cuda()
    hist = torch.full(shape, NAN, device="cuda")
    tabs.set(n, 0, 0)
    want = x.clone()
    for i in (n, n - 1):
        _lib.check(lib.dmme_chain_update_dpmpp(_lib.ptr(x), _lib.ptr(two), _lib.ptr(hist), _lib.ptr(tabs.coef), _lib.ptr(tabs.ttab), _lib.ptr(tabs.state), B, chw, 2,
                                               _lib.stream_ptr()))
        want, prev = _expr(want, two[:, :shape[1]], None if i == n else prev, rows[i], i < n)
    torch.cuda.synchronize()
    assert torch.equal(x, want) and torch.equal(hist, prev)


# ------------------------------------------------------------------------------------------ 2. more quads than threads
def test_grid_stride_loop():
    """(11, 3, 256, 256): 540672 quads for the 524288 threads of the largest grid, so some threads take two trips; two steps (the
    second reads the history) against the torch expression, bit for bit"""
    import dmme_amd
    from dmme_amd import _lib

    lib = _lib.lib()
    shape = (11, 3, 256, 256)
    proc = dmme_amd.DPMSolverPP(torch.nn.Identity(), 100, 5).cuda()
    n, rows, ttab = proc._chain_tables()
    tabs = _Tables(rows, ttab)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g).cuda()
    hist = torch.full(shape, NAN, device="cuda")
    want, prev = x.clone(), None
    tabs.set(n, 0, 0)
    for i in (n, n - 1):
        out = torch.randn(shape, generator=g).cuda()
        _lib.check(lib.dmme_chain_update_dpmpp(_lib.ptr(x), _lib.ptr(out), _lib.ptr(hist), _lib.ptr(tabs.coef), _lib.ptr(tabs.ttab), _lib.ptr(tabs.state),
                                               shape[0], int(np.prod(shape[1:])), 1, _lib.stream_ptr()))
        want, prev = _expr(want, out, prev, rows[i], i < n)
    assert tabs.words()[:6] == [n - 2, ttab[n - 2], 0, 0, 0, 1]
    assert torch.equal(x, want) and torch.equal(hist, prev) and bool(torch.isfinite(x).all())


# ------------------------------------------------------------------------------------------ 3. the classifier-free form
@pytest.mark.parametrize("s", [2.5, 1.0])
def test_cfg_update_is_bit_equal_and_keeps_both_halves_equal(s):
    """dmme_chain_update_cfg_dpmpp at B = 2 (x and the network output hold 4 images, the history 2) against dmme_cfg_dpmpp_step and
    the torch expression on e_u + s (e_c - e_u); both halves of x equal after every step; the plain kind fed that mixed prediction
    gives the same bits (the CFG kind is the mix in front of the plain update, nothing else).

    "s = 1 equals the plain kind fed the conditional half" holds bit for bit where s = 1 runs, not in this kernel: the three rounded
    operations e_u + 1 (e_c - e_u) do not return e_c's bits in fp32 (measured here: the first step's x differs in most elements), and
    the kernel forms the mix exactly as cfg_update does.  The samplers never send s = 1 through it: at s = 1 they run a batch-B plan,
    the conditional forward and the plain kind, which test_cfg_chains[1.0] holds to the eager plain update bit for bit."""
    import dmme_amd
    from dmme_amd import _lib

    lib = _lib.lib()
    B, img = 2, (3, 16, 16)
    chw = int(np.prod(img))
    proc = dmme_amd.DPMSolverPP(torch.nn.Identity(), 100, 5).cuda()
    n, ttab = proc.n_steps, proc._tau_host
    rows = proc._make_rows(s)
    assert all(r[6] == s for r in rows)
    tabs, plain = _Tables(rows, ttab), _Tables(rows, ttab)
    x0 = synth.normal(1, (B,) + img).cuda()
    x = torch.cat([x0, x0])
    twin, expr, xp = x.clone(), x0.clone(), x0.clone()
    hist = torch.full((B,) + img, NAN, device="cuda")
    hist_twin, hist_p, prev = hist.clone(), hist.clone(), None
    tabs.set(n, 0, 0)
    plain.set(n, 0, 0)
    for i in range(n, 0, -1):
        out = synth.normal(100 + i, (2 * B,) + img).cuda()
        _lib.check(lib.dmme_chain_update_cfg_dpmpp(_lib.ptr(x), _lib.ptr(out), _lib.ptr(hist), _lib.ptr(tabs.coef), _lib.ptr(tabs.ttab), _lib.ptr(tabs.state), B, chw,
                                                   _lib.stream_ptr()))
        _lib.check(lib.dmme_cfg_dpmpp_step(_lib.ptr(twin), _lib.ptr(out), _lib.ptr(hist_twin), (_lib.C.c_float * 8)(*rows[i]), int(i < n), B, chw, _lib.stream_ptr()))
        expr, prev = _expr(expr, _mix(out[:B], out[B:], s), prev, rows[i], i < n)
        assert tabs.words()[:6] == [i - 1, ttab[i - 1], 0, 0, 0, 1]
        assert torch.equal(x[:B], x[B:]) and torch.equal(x, twin) and torch.equal(hist, hist_twin), i
        assert torch.equal(x[:B], expr) and torch.equal(hist, prev) and tuple(hist.shape) == (B,) + img, i
        mixed = _mix(out[:B], out[B:], s).contiguous()
        _lib.check(lib.dmme_chain_update_dpmpp(_lib.ptr(xp), _lib.ptr(mixed), _lib.ptr(hist_p), _lib.ptr(plain.coef), _lib.ptr(plain.ttab), _lib.ptr(plain.state), B, chw,
                                               1, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(x[:B], xp) and torch.equal(hist, hist_p), i
    assert bool(torch.isfinite(x).all())


# ------------------------------------------------------------------------------------------ 4. whole chains against the restatement
@functools.lru_cache(maxsize=None)
def _reference(T, S, kind, order):
    abar = R.alpha_bar(T)
    g = R.grid(abar, S, kind)
    x_T = synth.normal(41, SHAPE)
    with torch.no_grad():
        return {dtype: R.decode(model, x_T, abar, g, order, dtype=dtype, keep=_keep(len(g) - 1)) for dtype, model in _cpu_models().items()}, g, x_T


@pytest.mark.parametrize("T,S", CHAINS)
def test_chains_vs_cpu_restatement(T, S):
    """the 2M chain on the tiny UNet in fp32, stepped through the captured graph, against tests/dpmpp_ref.py in float64 at the loop
    indices n, n-1, 2, 1; `decode` gives the stepped chain's bits.  Bound: 4 x the restatement's float32-vs-float64 gap at that index.

    Measured on the MI355X, largest GPU error over the checked indices (gap / GPU error / bound):
      (100, 5):   2.52e-6 / 2.52e-6 / 1.01e-5 (index 2)
      (1000, 20): 2.79e-4 / 2.59e-4 / 1.12e-3 (index 1; |x| reaches 591 under the random weights)
    The largest GPU error / gap ratio over every checked index was 1.35 ((100, 5), index 4), against the 4 allowed."""
    import dmme_amd

    ref, g, x_T = _reference(T, S, "logsnr", 2)
    net, _ = _tiny()
    proc = dmme_amd.DPMSolverPP(net, T, S).cuda()
    n = proc.n_steps
    assert proc._tau_host == g
    runner = proc.chain_runner(x_T.cuda().clone())
    runner.set(n, 0, 0)
    worst = (0.0, 0.0)
    for i in range(n, 0, -1):
        runner.step()
        if i in _keep(n):
            worst = max(worst, _check(f"2M ({T},{S}) after index {i}", runner.x, ref[torch.float64][i], ref[torch.float32][i]), key=lambda v: v[1])
    torch.cuda.synchronize()
    assert runner.capture_error is None and runner.graph is not None
    assert torch.equal(proc.decode(x_T.cuda()), runner.x)
    print(f"({T},{S}) largest GPU error (gap, error): {worst[0]:.2e}, {worst[1]:.2e}")


@pytest.mark.parametrize("T,S", CHAINS)
def test_order_one_vs_generalized_ddim(T, S):
    """order = 1 on the quadratic grid (strictly increasing at both sizes, so GeneralizedDDIM walks the same grid) against
    GeneralizedDDIM(eta = 0) and against the order-1 restatement, under the bound of the order-1 restatement's gap.

    Measured on the MI355X (gap / error vs the restatement / difference from GeneralizedDDIM / bound):
      (100, 5): 1.09e-6 / 1.17e-6 / 1.91e-6 / 4.35e-6;  (1000, 20): 2.08e-4 / 2.09e-4 / 3.36e-4 / 8.34e-4"""
    import dmme_amd

    ref, g, x_T = _reference(T, S, "quadratic", 1)
    net, _ = _tiny()
    proc = dmme_amd.DPMSolverPP(net, T, S, "quadratic", order=1).cuda()
    ddim = dmme_amd.GeneralizedDDIM(net, T, S, "quadratic").cuda()
    assert proc._tau_host == g == ddim._tau_host and proc.n_steps == S
    got = proc.decode(x_T.cuda())
    gap, _ = _check(f"order 1 ({T},{S}) vs the restatement", got, ref[torch.float64][0], ref[torch.float32][0])
    err = _maxabs(got, ddim.decode(x_T.cuda()))
    print(f"order 1 ({T},{S}) vs GeneralizedDDIM(eta = 0): difference {err:.3e}, bound {4 * gap:.3e}")
    assert err <= 4 * gap


def test_iddpm_network_through_from_process():
    """an IDDPM tiny network with its cosine schedule: the eps plane of the (B, 2C, H, W) output is the one used, the chain equals the
    restatement over oracle.iddpm.unet_forward's first C channels under the same rule.  (abar_T of the cosine schedule is 1.9e-15: the
    first x0 prediction is amplified by 2.3e7, in the restatement as on the device.)

    Measured on the MI355X: gap 3.42e+1, GPU error 3.77e+1, bound 1.37e+2 on |x| up to 9.1e7."""
    import dmme_amd
    from dmme_amd.models import iddpm as iddpm_models

    T, S = 100, 5
    cfg = OI.IUNetConfig(pos_dim=4, emb_dim=8, num_groups=2, dropout=0.0, channels_per_depth=(4, 8), num_blocks=1, attention_depths=(2,))
    sd = OI.make_state_dict(cfg, 17)
    sd64 = {k: v.to(torch.float64) if v.is_floating_point() else v for k, v in sd.items()}
    net = iddpm_models.UNet(3, 4, 8, 2, 0.0, (4, 8), 1, (2,))
    net.load_state_dict(sd, strict=True)
    p = dmme_amd.IDDPM(net.cuda().eval(), T).cuda()
    proc = dmme_amd.DPMSolverPP.from_process(p, sub_timesteps=S).cuda()
    abar = p.alpha_bar.reshape(-1).double().cpu().numpy()
    g = R.grid(abar, S, "logsnr")
    assert proc._tau_host == g
    x_T = synth.normal(43, SHAPE)
    with torch.no_grad():
        r32 = R.decode(lambda x, t: OI.unet_forward(sd, cfg, x, t)[:, :3], x_T, abar, g, dtype=torch.float32)[0]
        r64 = R.decode(lambda x, t: OI.unet_forward(sd64, cfg, x, t)[:, :3], x_T, abar, g, dtype=torch.float64)[0]
    got = proc.decode(x_T.cuda())
    assert proc._runner is not None and proc._runner.out.shape[1] == 6
    _check(f"IDDPM tiny network ({T},{S})", got, r64, r32)
    with torch.no_grad():
        assert torch.equal(got, proc._eager_chain(x_T.cuda().clone(), proc.n_steps))


# ------------------------------------------------------------------------------------------ 5. captured versus eager
def test_generate_through_the_captured_step_equals_the_eager_loop():
    """`generate` (one hipGraph of UNet + update + state advance, replayed) against the eager host loop, bit for bit; two consecutive
    chains on one runner equal two fresh ones (the flag clears on `set`: the second chain must not read the first one's history);
    a chain started mid-table likewise; after load_state_dict the runner re-captures; torch's generator moves by x_T alone"""
    import dmme_amd

    net, _ = _tiny()
    proc = dmme_amd.DPMSolverPP(net, 100, 7).cuda()
    n, numel = proc.n_steps, int(np.prod(SHAPE))
    torch.manual_seed(77)
    before = _gen_offset()
    a = proc.generate(SHAPE)
    assert _gen_offset() - before == numel
    torch.manual_seed(78)
    b = proc.generate(SHAPE)
    runner, graph = proc._runner, proc._runner.graph
    assert runner.capture_error is None and graph is not None and not torch.equal(a, b)
    with torch.no_grad():
        for seed, got in ((77, a), (78, b)):
            torch.manual_seed(seed)
            x = dmme_amd.gaussian(SHAPE, device="cuda")
            assert torch.equal(got, proc._eager_chain(x, n)) and bool(torch.isfinite(got).all())
        fresh = dmme_amd.DPMSolverPP(net, 100, 7).cuda()
        torch.manual_seed(78)
        assert torch.equal(fresh.generate(SHAPE), b)
        # a chain placed mid-table after a whole one: first order first step, not the stale history
        x_mid = synth.normal(9, SHAPE).cuda()
        before = _gen_offset()
        mid = proc.decode(x_mid, start=n - 2)
        assert _gen_offset() == before and proc._runner is runner and runner.graph is graph
        assert torch.equal(mid, proc._eager_chain(x_mid.clone(), n - 2))
        # the eager surface with a history tensor walks the same chain
        torch.manual_seed(77)
        x, hist = dmme_amd.gaussian(SHAPE, device="cuda"), torch.full(SHAPE, NAN, device="cuda")
        for i in range(n, 0, -1):
            x = proc.sampling_step(x, torch.tensor([i], device="cuda"), hist, history_valid=i < n)
        assert torch.equal(x, a) and torch.equal(x, hist)
        # without history_valid the history is written, never read: a NaN history gives the first-order step
        hist = torch.full(SHAPE, NAN, device="cuda")
        first = proc.sampling_step(x_mid, torch.tensor([n - 2], device="cuda"), hist)
        assert torch.equal(first, proc.sampling_step(x_mid, torch.tensor([n - 2], device="cuda")))
        assert bool(torch.isfinite(first).all()) and bool(torch.isfinite(hist).all())
        with pytest.raises(ValueError):
            proc.sampling_step(x_mid, torch.tensor([n - 2], device="cuda"), None, history_valid=True)
        # new weights: the runner re-captures and follows them
        net.load_state_dict(O.make_state_dict(O.TINY, 12))
        torch.manual_seed(77)
        c = proc.generate(SHAPE)
        assert proc._runner is runner and runner.graph is not graph and not torch.equal(c, a)
        torch.manual_seed(77)
        assert torch.equal(c, proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), n))


# ------------------------------------------------------------------------------------------ 6. classifier-free chains
@pytest.mark.parametrize("s", [2.5, 1.0])
def test_cfg_chains(s):
    """ClassifierFreeDPMSolver.generate in the tiny conditional setting of tests/test_gpu_cond.py: the captured chain equals the eager
    loop bit for bit, and the restatement (tests/cond_ref.py's network, mixed) under the rule of test 4.

    Measured on the MI355X (gap / GPU error / bound): s = 2.5: 2.92e-6 / 3.67e-6 / 1.17e-5;  s = 1: 2.42e-6 / 2.42e-6 / 9.67e-6"""
    import dmme_amd

    K, B, T, S = 3, 3, 100, 5
    cfg = CR.TINY
    sd = CR.make_state_dict(cfg, K, 51)
    net = dmme_amd.ConditionalUNet(precision="fp32", num_classes=K, dropout=0.0, pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    shape = (B, 3, 32, 32)
    y = torch.tensor([2, 0, 1])
    proc = dmme_amd.ClassifierFreeDPMSolver(net, T, S, guidance_scale=s).cuda()
    torch.manual_seed(7)
    before = _gen_offset()
    got = proc.generate(shape, y)
    assert _gen_offset() - before == int(np.prod(shape))
    runner = proc._cfg_runner
    assert runner.capture_error is None and runner.graph is not None and runner.plan.B == (2 * B if s != 1.0 else B) and runner.hist.shape[0] == B
    torch.manual_seed(7)
    x_T = dmme_amd.gaussian(shape, device="cuda")
    with torch.no_grad():
        assert torch.equal(got, proc._eager_generate(x_T.clone(), y))
        # the labelled eager surface, history in hand
        x, hist = x_T.clone(), torch.full(shape, NAN, device="cuda")
        for i in range(proc.n_steps, 0, -1):
            x = proc.sampling_step(x, torch.tensor([i], device="cuda"), y, hist, history_valid=i < proc.n_steps)
        assert torch.equal(x, got)
    # a second chain on the same runner: the same graph, no stale history
    torch.manual_seed(7)
    assert torch.equal(proc.generate(shape, y), got) and proc._cfg_runner.graph is runner.graph
    abar = R.alpha_bar(T)
    g = R.grid(abar, S, "logsnr")
    assert proc._tau_host == g
    yu = torch.full_like(y, K)
    refs = {}
    with torch.no_grad():
        for dtype in (torch.float32, torch.float64):
            w = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
            model = lambda x, t: R.mix(CR.forward(w, cfg, x, t, y), CR.forward(w, cfg, x, t, yu), s, dtype)
            refs[dtype] = R.decode(model, x_T.cpu(), abar, g, dtype=dtype)[0]
    _check(f"classifier-free 2M chain, s = {s}", got, refs[torch.float64], refs[torch.float32])
