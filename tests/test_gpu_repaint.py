"""-m gpu: RePaint inpainting and SDEdit editing (dmme_amd.RePaint) on the MI355X - the update kind DMME_CHAIN_REPAINT and its eager twin
bit for bit against an fp32 torch expression, the three normal streams and the loop state, the identities that tie the kind to DDPM's
update and to the known image, the captured chains against the eager loops, and whole chains against the CPU restatement
tests/repaint_ref.py.

Against the restatement the yardstick is the one of tests/test_gpu_dpmpp.py: the restatement's own float32-versus-float64 gap on the same
inputs and the same normals (oracle.unet.unet_forward as the network), computed on the CPU while the test runs; the GPU's fp32 result may
sit at 4 x that gap from the float64 result at each checked index.  Every comparison prints gap, error and bound."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import iddpm as OI
from oracle import synth
from oracle import unet as O

from . import repaint_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 32, 32)
CHAINS = [(100, 8, 3, 2), (1000, 20, 5, 3)]  # 14 and 50 steps


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


def _maxabs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _check(tag, got, ref64, ref32):
    """GPU fp32 within 4 x (the restatement's float32-vs-float64 gap) of the float64 result; returns (gap, error)"""
    gap, err = _maxabs(ref32, ref64), _maxabs(got, ref64)
    print(f"{tag}: CPU fp32-vs-fp64 gap {gap:.3e}, GPU error {err:.3e}, bound {4 * gap:.3e} (|ref|max {float(ref64.abs().max()):.3f})")
    assert bool(torch.isfinite(got).all()) and err <= 4 * gap, tag
    return gap, err


def _gen_offset():
    return int(torch.cuda.default_generators[torch.cuda.current_device()].get_offset())


def _randn3(shape, seed, off):
    """the [3, *shape] block of one step: dmme_randn of 3 * numel values at quad offset `off`"""
    from dmme_amd import _lib

    z = torch.empty((3,) + tuple(shape), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().dmme_randn(_lib.ptr(z), z.numel(), seed, off, _lib.stream_ptr()))
    return z


def _expr(x, e, x0, m, z3, row):
    """the fp32 torch expression of one update: separate kernels, so every product, sum and difference rounds on its own"""
    c0, c1, c2, ka, ks, r0, r1 = row[:7]
    u = c0 * (x - c1 * e)
    if c2 != 0.0:
        u = u + c2 * z3[0]
    k = ka * x0
    if ks != 0.0:
        k = k + ks * z3[1]
    y = m * k + (1.0 - m) * u
    return r0 * y + r1 * z3[2] if r1 != 0.0 else y


def _masks(shape):
    checker = torch.zeros(shape)
    checker.view(-1)[::2] = 1.0  # every other element: each quad holds known and generated pixels
    return {"zeros": torch.zeros(shape), "ones": torch.ones(shape), "checker": checker}


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


def _chain_update(x, out, known, mask, noise, tabs, planes=1):
    from dmme_amd import _lib

    _lib.check(_lib.lib().dmme_chain_update_repaint(_lib.ptr(x), _lib.ptr(out), _lib.ptr(known), _lib.ptr(mask), _lib.ptr(noise), _lib.ptr(tabs.coef),
                                                    _lib.ptr(tabs.ttab), _lib.ptr(tabs.state), x.shape[0], x[0].numel(), planes, _lib.stream_ptr()))


def _eager_update(x, out, known, mask, z3, row, planes=1):
    from dmme_amd import _lib

    _lib.check(_lib.lib().dmme_repaint_step(_lib.ptr(x), _lib.ptr(out), _lib.ptr(known), _lib.ptr(mask), _lib.ptr(z3), (C.c_float * 8)(*row), x.shape[0],
                                            x[0].numel(), planes, _lib.stream_ptr()))


# ------------------------------------------------------------------------------------------ 1. the update alone
@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (1, 3, 4, 4)])  # 576 quads in three blocks (the ticket counts); one partial block
@pytest.mark.parametrize("mask", ["zeros", "ones", "checker"])
def test_chain_update_eager_twin_and_torch_expression_are_bit_equal(shape, mask):
    """dmme_chain_update_repaint drawing in the kernel (row and index from device memory) against dmme_repaint_step fed
    dmme_randn(3 * numel) at the offset the state stood at, and against the fp32 torch expression, bit for bit after every step of the
    whole walk n = 6, j = 2, r = 2 (10 steps: plain ones, ones with a jump, the last).  The loop state after every step: i - 1,
    t_table[i - 1], the offset moved by 3 n4 whatever the step drew, the seed, the ticket back at zero, the sixth and the reserved words
    as they were.  Then a network output of two planes per image: the eps plane is the one used."""
    import dmme_amd

    proc = dmme_amd.RePaint(torch.nn.Identity(), 100, 6, 2, 2)
    n, rows, ttab = proc._chain_tables()
    assert n == 10 and sum(1 for r in rows[1:] if r[6] != 0.0) == 2 and rows[1][2] == rows[1][4] == rows[1][6] == 0.0
    numel = int(np.prod(shape))
    n4, seed, off0 = numel // 4, 77, 1234
    tabs = _Tables(rows, ttab)
    m = _masks(shape)[mask].cuda()
    known = (0.5 * synth.normal(5, shape)).cuda()
    x = synth.normal(1, shape).cuda()
    twin, expr = x.clone(), x.clone()
    tabs.set(n, seed, off0)
    tabs.state[5:] = torch.tensor([41, 42, 43], device="cuda")  # (no paint step reads or writes these words)
    assert tabs.words() == [n, ttab[n], off0, seed, 0, 41, 42, 43]
    for k, i in enumerate(range(n, 0, -1)):
        out = synth.normal(100 + i, shape).cuda()
        z3 = _randn3(shape, seed, off0 + 3 * n4 * k)
        _chain_update(x, out, known, m, None, tabs)
        _eager_update(twin, out, known, m, z3, rows[i])
        expr = _expr(expr, out, known, m, z3, rows[i])
        assert tabs.words() == [i - 1, ttab[i - 1], off0 + 3 * n4 * (k + 1), seed, 0, 41, 42, 43], i
        assert torch.equal(x, twin), f"chain kind and eager twin differ at loop index {i}"
        assert torch.equal(x, expr), f"chain kind and the torch expression differ at loop index {i}"
        assert bool(torch.isfinite(x).all())
    if mask == "ones":
        assert torch.equal(x, known)
    if mask == "checker":
        assert torch.equal(x.view(-1)[::2], known.view(-1)[::2]) and not torch.equal(x, known)
    # (eps, v) planes per image, as an IDDPM network writes them
    Cc = shape[1]
    two = synth.normal(3, (shape[0], 2 * Cc) + shape[2:]).cuda()
    x, twin, want = (synth.normal(2, shape).cuda() for _ in range(3))
    tabs.set(n, seed, 0)
    for k, i in enumerate((n, n - 1, n - 2, n - 3)):
        z3 = _randn3(shape, seed, 3 * n4 * k)
        _chain_update(x, two, known, m, None, tabs, planes=2)
        _eager_update(twin, two, known, m, z3, rows[i], planes=2)
        want = _expr(want, two[:, :Cc], known, m, z3, rows[i])
    torch.cuda.synchronize()
    assert torch.equal(x, want) and torch.equal(twin, want)


# ------------------------------------------------------------------------------------------ 2. identities
def test_identities():
    """m = 0 and a row without a jump: the eager twin is dmme_ddpm_step on the same z0, bit for bit, on the full grid (every timestep
    with a plain row, t = 1 included).  m = 1: the result does not depend on the network output.  After the last row x' == x0 exactly.
    The chain form fed `noise` equals the chain form drawing the same values."""
    import dmme_amd
    from dmme_amd import _lib

    lib = _lib.lib()
    shape = (3, 3, 16, 16)
    numel = int(np.prod(shape))
    proc = dmme_amd.RePaint(torch.nn.Identity(), 100, 100, 3, 2)
    n, rows, ttab = proc._chain_tables()
    zeros, ones = torch.zeros(shape, device="cuda"), torch.ones(shape, device="cuda")
    known = (0.5 * synth.normal(5, shape)).cuda()
    x0, e = synth.normal(1, shape).cuda(), synth.normal(2, shape).cuda()
    z3 = _randn3(shape, 9, 0)
    seen = set()
    for i in range(n, 0, -1):
        t = ttab[i]
        if rows[i][6] != 0.0 or t in seen:
            continue
        seen.add(t)
        a, b = x0.clone(), x0.clone()
        _eager_update(a, e, known, zeros, z3, rows[i])
        _lib.check(lib.dmme_ddpm_step(_lib.ptr(b), _lib.ptr(e), _lib.ptr(z3[0]), proc._c1[t], proc._c2[t], proc._sigma[t], int(t != 1), numel, _lib.stream_ptr()))
        assert torch.equal(a, b), f"t = {t}"
    assert seen == set(range(1, 101))
    # m = 1: two different network outputs, equal bits (a row with a jump, a plain row, the last row)
    jump = next(i for i in range(n, 0, -1) if rows[i][6] != 0.0)
    for i in (jump, n, 1):
        a, b = x0.clone(), x0.clone()
        _eager_update(a, e, known, ones, z3, rows[i])
        _eager_update(b, 3.0 * e + 1.0, known, ones, z3, rows[i])
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), i
    assert torch.equal(a, known)  # the last row: ka = 1, ks = 0, r1 = 0; it needs no normals at all
    c = x0.clone()
    _eager_update(c, e, known, ones, None, rows[1])
    assert torch.equal(c, known)
    # the override
    tabs = _Tables(rows, ttab)
    m = _masks(shape)["checker"].cuda()
    for i in (jump, n):
        a, b = x0.clone(), x0.clone()
        tabs.set(i, 9, 0)
        _chain_update(a, e, known, m, None, tabs)
        tabs.set(i, 1, 5)  # another seed and offset: every normal comes from `noise`
        _chain_update(b, e, known, m, z3, tabs)
        assert torch.equal(a, b), i
        assert tabs.words()[:5] == [i - 1, ttab[i - 1], 5 + 3 * (numel // 4), 1, 0]


# ------------------------------------------------------------------------------------------ 3. more quads than threads, 64-bit counters
def test_grid_stride_loop_and_wide_counters():
    """(11, 3, 256, 256): 540672 quads for the 524288 threads of the largest grid, so some threads take two trips; the Philox offset
    starts above 2^33, so a counter kept in 32 bits would draw other normals.  Two steps, the second with a jump, against the torch
    expression with normals from dmme_randn, bit for bit."""
    import dmme_amd

    shape = (11, 3, 256, 256)
    numel = int(np.prod(shape))
    n4 = numel // 4
    proc = dmme_amd.RePaint(torch.nn.Identity(), 100, 3, 2, 2)
    n, rows, ttab = proc._chain_tables()
    assert n == 5 and rows[n][6] == 0.0 and rows[n - 1][6] != 0.0
    tabs = _Tables(rows, ttab)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g).cuda()
    known = torch.randn(shape, generator=g).cuda()
    m = (torch.rand(shape, generator=g) < 0.5).float().cuda()
    seed, off0 = 123456789012345, (1 << 33) + 5
    want = x.clone()
    tabs.set(n, seed, off0)
    for k, i in enumerate((n, n - 1)):
        out = torch.randn(shape, generator=g).cuda()
        _chain_update(x, out, known, m, None, tabs)
        want = _expr(want, out, known, m, _randn3(shape, seed, off0 + 3 * n4 * k), rows[i])
    assert tabs.words()[:5] == [n - 2, ttab[n - 2], off0 + 6 * n4, seed, 0]
    assert torch.equal(x, want) and bool(torch.isfinite(x).all())


# ------------------------------------------------------------------------------------------ 4. whole chains against the restatement
def _half_mask():
    m = torch.zeros(1, 1, SHAPE[2], SHAPE[3])
    m[..., : SHAPE[3] // 2] = 1.0
    return m


def _image(seed):
    return (0.5 * synth.normal(seed, SHAPE)).clamp(-1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _reference(T, n, j, r, seed, off):
    """the restatement in float32 and float64 on the normals the device draws for (seed, off), copied to the host"""
    abar = R.alpha_bar(T)
    g = R.grid(abar, n)
    n_rows = R.down_count(len(g) - 1, j, r)
    x_T, x0, m = synth.normal(41, SHAPE), _image(42), _half_mask().expand(SHAPE)
    numel = int(np.prod(SHAPE))
    normals = torch.cat([_randn3(SHAPE, seed, off + 3 * (numel // 4) * k).cpu().unsqueeze(0) for k in range(n_rows)])
    keep = {n_rows, n_rows - 1, 2, 1}
    with torch.no_grad():
        ref = {dtype: R.inpaint(model, x_T, x0, m, abar, g, j, r, normals, dtype, keep) for dtype, model in _cpu_models().items()}
    return ref, g, n_rows, x_T, x0


@pytest.mark.parametrize("T,n,j,r", CHAINS)
def test_chains_vs_cpu_restatement(T, n, j, r):
    """the RePaint walk on the tiny UNet in fp32 with a half-image mask, stepped through the captured graph with in-kernel draws, against
    tests/repaint_ref.py in float64 on the same normals at the first two and last two loop indices.  Bound: 4 x the restatement's
    float32-vs-float64 gap at that index.  `inpaint` under the same seed returns the stepped chain's bits; known pixels equal x0 exactly.

    Measured on the MI355X, largest GPU error over the checked indices (gap / GPU error / bound):
      (100, 8, 3, 2), 14 steps:   3.30e-6 / 4.25e-6 / 1.32e-5 (index 1)
      (1000, 20, 5, 3), 50 steps: 6.30e-4 / 6.30e-4 / 2.52e-3 (index 1; |x| reaches 931 under the random weights)
    The largest GPU error / gap ratio over every checked index was 1.29 ((100, 8, 3, 2), index 1), against the 4 allowed."""
    import dmme_amd
    from dmme_amd.common.noise import philox_reserve

    net = _tiny()
    proc = dmme_amd.RePaint(net, T, n, j, r).cuda()
    numel = int(np.prod(SHAPE))
    torch.manual_seed(5)
    x_T_dev = dmme_amd.gaussian(SHAPE, device="cuda")  # (the draw `inpaint` makes first under this seed; the chain starts from synth's x_T below)
    seed, off = philox_reserve(x_T_dev.device, 3 * numel * proc.n_rows)
    ref, g, n_rows, x_T, x0 = _reference(T, n, j, r, seed, off)
    assert proc._tau_host == g and proc.n_rows == n_rows == {8: 14, 20: 50}[n]
    m = _half_mask()
    runner = proc.chain_runner(x_T.cuda().clone())
    assert isinstance(runner, dmme_amd.PaintChainRunner) and runner.noise_numel == 3 * numel
    runner.known.copy_(x0)
    runner.mask.copy_(m.expand(SHAPE))
    runner.set(n_rows, seed, off)
    worst = (0.0, 0.0)
    for i in range(n_rows, 0, -1):
        runner.step()
        if i in (n_rows, n_rows - 1, 2, 1):
            worst = max(worst, _check(f"RePaint ({T},{n},{j},{r}) after index {i}", runner.x, ref[torch.float64][i], ref[torch.float32][i]), key=lambda v: v[1])
    torch.cuda.synchronize()
    assert runner.capture_error is None and runner.graph is not None
    print(f"({T},{n},{j},{r}) largest GPU error (gap, error): {worst[0]:.2e}, {worst[1]:.2e}")
    keep = m.expand(SHAPE).bool()
    assert torch.equal(runner.x.cpu()[keep], x0[keep])
    # `inpaint` from its own x_T under the same seed: the same offsets, so the chain stepped from that x_T gives its bits
    runner.x.copy_(x_T_dev)
    runner.set(n_rows, seed, off)
    for _ in range(n_rows):
        runner.step()
    torch.manual_seed(5)
    got = proc.inpaint(x0, m)
    assert torch.equal(got, runner.x) and got.data_ptr() != runner.x.data_ptr() and torch.equal(got.cpu()[keep], x0[keep])
    assert proc._runner.capture_error is None and proc._runner.graph is not None


# ------------------------------------------------------------------------------------------ 5. captured versus eager
def test_inpaint_through_the_captured_step_equals_the_eager_loop():
    """`inpaint` (one hipGraph of UNet + three draws + update + state advance, replayed) against the host loop over dmme_repaint_step,
    bit for bit under the same seed; a second chain on the same runner re-uses the graph; torch's generator moves by x_T plus 3 numel per
    step; after load_state_dict the runner re-captures; `generate` is `inpaint` with nothing known"""
    import dmme_amd

    net = _tiny()
    proc = dmme_amd.RePaint(net, 100, 8, 3, 2).cuda()
    numel, x0, m = int(np.prod(SHAPE)), _image(42).cuda(), _half_mask().cuda()
    full = m.expand(SHAPE).contiguous()
    torch.manual_seed(77)
    before = _gen_offset()
    a = proc.inpaint(x0, m)
    assert _gen_offset() - before == numel + 3 * numel * proc.n_rows
    runner, graph = proc._runner, proc._runner.graph
    assert runner.capture_error is None and graph is not None and isinstance(runner, dmme_amd.PaintChainRunner)
    torch.manual_seed(78)
    b = proc.inpaint(x0, m)
    assert proc._runner is runner and runner.graph is graph and not torch.equal(a, b)
    with torch.no_grad():
        for seed, got in ((77, a), (78, b)):
            torch.manual_seed(seed)
            before = _gen_offset()
            x = dmme_amd.gaussian(SHAPE, device="cuda")
            assert torch.equal(got, proc._eager_chain(x, x0, full)) and bool(torch.isfinite(got).all())
            assert _gen_offset() - before == numel + 3 * numel * proc.n_rows
        torch.manual_seed(77)
        gen = proc.generate(SHAPE)
        torch.manual_seed(77)
        zeros = torch.zeros(SHAPE, device="cuda")
        assert torch.equal(gen, proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), zeros, zeros)) and proc._runner.graph is graph
        net.load_state_dict(O.make_state_dict(O.TINY, 12))
        torch.manual_seed(77)
        c = proc.inpaint(x0, m)
        assert proc._runner is runner and runner.graph is not graph and not torch.equal(c, a)
        torch.manual_seed(77)
        assert torch.equal(c, proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), x0, full))
    keep = full.bool()
    assert torch.equal(a[keep], x0[keep]) and torch.equal(c[keep], x0[keep])


def test_iddpm_network_through_from_process():
    """an IDDPM tiny network with its cosine schedule through `from_process`: the eps plane of the (B, 2C, H, W) output is the one used;
    the inpainted result against the restatement over oracle.iddpm.unet_forward's first C channels under the rule of test 4, and the
    captured chain against the eager loop bit for bit.  (abar_T of the cosine schedule is 1.9e-15: the first reverse step multiplies by
    1 / sqrt(abar_n / abar_{n-1}), in the restatement as on the device.)

    Measured on the MI355X: gap 4.08e+1, GPU error 4.32e+1, bound 1.63e+2 on |x| up to 1.35e8."""
    import dmme_amd
    from dmme_amd.common.noise import philox_reserve
    from dmme_amd.models import iddpm as iddpm_models

    T, n, j, r = 100, 5, 2, 2
    cfg = OI.IUNetConfig(pos_dim=4, emb_dim=8, num_groups=2, dropout=0.0, channels_per_depth=(4, 8), num_blocks=1, attention_depths=(2,))
    sd = OI.make_state_dict(cfg, 17)
    sd64 = {k: v.to(torch.float64) if v.is_floating_point() else v for k, v in sd.items()}
    net = iddpm_models.UNet(3, 4, 8, 2, 0.0, (4, 8), 1, (2,))
    net.load_state_dict(sd, strict=True)
    p = dmme_amd.IDDPM(net.cuda().eval(), T).cuda()
    proc = dmme_amd.RePaint.from_process(p, sub_timesteps=n, jump_length=j, resamples=r).cuda()
    abar = p.alpha_bar.reshape(-1).double().cpu().numpy()
    g = R.grid(abar, n)
    assert proc._tau_host == g and proc.n_rows == R.down_count(n, j, r) == 9
    numel, x0, m = int(np.prod(SHAPE)), _image(42), _half_mask()
    torch.manual_seed(11)
    x_T = dmme_amd.gaussian(SHAPE, device="cuda")
    seed, off = philox_reserve(x_T.device, 3 * numel * proc.n_rows)
    normals = torch.cat([_randn3(SHAPE, seed, off + 3 * (numel // 4) * k).cpu().unsqueeze(0) for k in range(proc.n_rows)])
    with torch.no_grad():
        r32 = R.inpaint(lambda x, t: OI.unet_forward(sd, cfg, x, t)[:, :3], x_T.cpu(), x0, m.expand(SHAPE), abar, g, j, r, normals, torch.float32)[0]
        r64 = R.inpaint(lambda x, t: OI.unet_forward(sd64, cfg, x, t)[:, :3], x_T.cpu(), x0, m.expand(SHAPE), abar, g, j, r, normals, torch.float64)[0]
    torch.manual_seed(11)
    got = proc.inpaint(x0, m)
    assert proc._runner is not None and proc._runner.out.shape[1] == 6 and proc._runner.capture_error is None
    _check(f"IDDPM tiny network ({T},{n},{j},{r})", got, r64, r32)
    torch.manual_seed(11)
    with torch.no_grad():
        assert torch.equal(got, proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), x0.cuda(), m.expand(SHAPE).contiguous().cuda()))


# ------------------------------------------------------------------------------------------ 6. SDEdit
def test_sdedit():
    """`edit(x_guide, 0.5)` is dmme_q_sample to level k followed by the eager plain walk, bit for bit; with a mask the kept pixels are
    the guide's exactly; strength maps to k = 1 at the low end and k = n at 1.0; the process was built with resamples = 3 and `edit`
    still walks the resamples = 1 tables (k steps, loop index = level)"""
    import dmme_amd

    net = _tiny()
    proc = dmme_amd.RePaint(net, 100, 8, 3, 3).cuda()
    n, numel = proc.n_levels, int(np.prod(SHAPE))
    assert n == 8 and proc.n_rows == 8 + 2 * 3 * 2 and proc._plain_tables[0] == 8
    guide = _image(43).cuda()
    zeros = torch.zeros(SHAPE, device="cuda")

    def eager(seed, strength, mask):
        torch.manual_seed(seed)
        k = proc.edit_level(strength)
        z = dmme_amd.gaussian_like(guide)
        t = torch.full((SHAPE[0],), proc._tau_host[k], dtype=torch.int64, device="cuda")
        x_k = proc._noised(guide, t, z, target=False)[2]
        assert torch.equal(x_k, proc._sqrt_alpha_bar[t[0]] * guide + proc._sqrt_one_minus_alpha_bar[t[0]] * z)
        with torch.no_grad():
            return proc._eager_chain(x_k, guide, mask, proc._plain_tables, k), k

    torch.manual_seed(3)
    before = _gen_offset()
    got = proc.edit(guide, 0.5)
    moved = _gen_offset() - before
    want, k = eager(3, 0.5, zeros)
    assert k == 4 and moved == numel + 3 * numel * k  # (the guide's noise, then k steps: not the walk's 20)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and not torch.equal(got, guide)
    runner = proc._edit_runner
    assert isinstance(runner, dmme_amd.PaintChainRunner) and runner.n_steps == n and runner.capture_error is None and runner.graph is not None
    assert [int(v) for v in runner.ttab.cpu()] == proc._tau_host
    # the ends of the strength scale, on the same runner and graph
    for strength, level in ((0.01, 1), (1.0, n)):
        torch.manual_seed(4)
        got = proc.edit(guide, strength)
        want, k = eager(4, strength, zeros)
        assert k == level and torch.equal(got, want) and proc._edit_runner is runner
    # the masked variant
    m = _half_mask().cuda()
    full = m.expand(SHAPE).contiguous()
    torch.manual_seed(6)
    got = proc.edit(guide, 0.75, m)
    want, k = eager(6, 0.75, full)
    keep = full.bool()
    assert k == 6 and torch.equal(got, want) and torch.equal(got[keep], guide[keep]) and not torch.equal(got[~keep], guide[~keep])
