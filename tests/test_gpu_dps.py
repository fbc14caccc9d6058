"""-m gpu: DPS (dmme_amd.DPS) on the MI355X - the measurement dmme_dps_measure, the adjoint kernel and the update against float64 under
derived bounds (tests/dps_ref.py: measure_bound, adjoint_bound, update_bound - built from the precision of fp32 and the lengths of the dot
products, not measured; tests/test_dps_host.py shows on the CPU that a plain fp32 evaluation sits inside them), the identities (an
unmeasured cell ignores y, the eps plane of a two-plane output, zeta = 0 is dmme_ddpm_step, a norm never mixes images), the eager forms
against the chain forms (normals, loop state), the assembled step against float64 autograd of the oracle, the captured chain against the
eager loop, the guidance's effect on the residual, bf16, and the refusals.  Every comparison prints its figures."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import dps_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 32, 32)
# (image shape, preset, its arguments): 12 x 20 -> 3 x 5 has measurement widths that are no multiple of 4, 64 x 64 fills the capacity
OPS = [((2, 3, 8, 8), "identity", {}), ((2, 3, 12, 20), "average", dict(scale=4)), ((1, 3, 32, 32), "bicubic", dict(scale=4)),
       ((1, 3, 64, 64), "blur", dict(size=9, sigma=2.0))]


def _lib():
    from dmme_amd import _lib

    return _lib


def _binary(shape, seed, p=0.7):
    m = (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < p).float()
    m.view(-1)[0], m.view(-1)[-1] = 0.0, 1.0
    return m


@functools.lru_cache(maxsize=None)
def _operator(idx):
    """(shape, float64 fp32-rounded Kh, Kw on the host, their fp32 device copies) of OPS[idx], from the restatement's own builders"""
    shape, name, kw = OPS[idx]
    Kh, Kw = (R.rounded(K) for K in R.operator(name, shape[2], shape[3], **kw))
    return shape, Kh, Kw, Kh.float().cuda().contiguous(), Kw.float().cuda().contiguous()


def _measure(x, Khd, Kwd, mask):
    L = _lib()
    B, Cc, H, W = x.shape
    h, w = Khd.shape[0], Kwd.shape[0]
    y = torch.full((B, Cc, h, w), float("nan"), device="cuda")
    L.check(L.lib().dmme_dps_measure(L.ptr(x), L.ptr(Khd), L.ptr(Kwd), L.ptr(mask), L.ptr(y), B, Cc, H, W, h, w, L.stream_ptr()), "dmme_dps_measure")
    return y


def _adjoint(x, out, y, m, Khd, Kwd, row, planes=1, tabs=None):
    """(g, d_out, sumsq) of the eager form, or of the chain form at the loop state of `tabs`; outputs pre-filled with NaN"""
    L = _lib()
    B, Cc, H, W = x.shape
    h, w = Khd.shape[0], Kwd.shape[0]
    g = torch.full_like(x, float("nan"))
    d_out = torch.full_like(out, float("nan"))
    ss = torch.full((B, Cc), float("nan"), device="cuda")
    if tabs is None:
        L.check(L.lib().dmme_dps_adjoint(L.ptr(x), L.ptr(out), planes, (C.c_float * 8)(*row), L.ptr(y), L.ptr(m), L.ptr(Khd), L.ptr(Kwd), L.ptr(g), L.ptr(d_out),
                                         L.ptr(ss), B, Cc, H, W, h, w, L.stream_ptr()), "dmme_dps_adjoint")
    else:
        L.check(L.lib().dmme_chain_adjoint_dps(L.ptr(x), L.ptr(out), planes, L.ptr(tabs.coef), L.ptr(tabs.state), L.ptr(y), L.ptr(m), L.ptr(Khd), L.ptr(Kwd),
                                               L.ptr(g), L.ptr(d_out), L.ptr(ss), B, Cc, H, W, h, w, L.stream_ptr()), "dmme_chain_adjoint_dps")
    return g, d_out, ss


def _eager(x, out, g, dx, ss, z, row, planes=1):
    L = _lib()
    B, Cc, H, W = x.shape
    L.check(L.lib().dmme_dps_step(L.ptr(x), L.ptr(out), L.ptr(g), L.ptr(dx), L.ptr(ss), L.ptr(z), (C.c_float * 8)(*row), B, Cc, H, W, planes, L.stream_ptr()),
            "dmme_dps_step")
    return x


def _chain_update(x, out, g, dx, ss, noise, tabs, planes=1):
    L = _lib()
    B, Cc, H, W = x.shape
    L.check(L.lib().dmme_chain_update_dps(L.ptr(x), L.ptr(out), L.ptr(g), L.ptr(dx), L.ptr(ss), L.ptr(noise), L.ptr(tabs.coef), L.ptr(tabs.ttab), L.ptr(tabs.state),
                                          B, Cc, H, W, planes, L.stream_ptr()), "dmme_chain_update_dps")
    return x


def _randn(shape, seed, off):
    L = _lib()
    z = torch.empty(tuple(shape), dtype=torch.float32, device="cuda")
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


def _rows(zeta=1.0, T=100, n=10):
    """the package's fp32 rows of a 10-level walk over T = 100"""
    import dmme_amd

    return dmme_amd.DPS(torch.nn.Identity(), T, n, zeta=zeta)._chain_tables()


# ------------------------------------------------------------------------------------------ 1. the measurement alone
@pytest.mark.parametrize("idx", range(len(OPS)))
def test_measure_vs_float64(idx):
    """dmme_dps_measure on 3 randn + 0.7 against M o (Kh x Kw^T) in float64 on the same fp32 matrices, elementwise inside measure_bound,
    under a random binary mask and with no mask; an unmeasured cell gives exactly 0; the same image at another place of a larger batch
    gives the same bits"""
    shape, Kh, Kw, Khd, Kwd = _operator(idx)
    x = (3.0 * torch.randn(shape, generator=torch.Generator().manual_seed(3)) + 0.7).cuda()
    m = _binary((shape[0], shape[1], Kh.shape[0], Kw.shape[0]), 5).cuda()
    bound = R.measure_bound(x, Kh, Kw)
    for mask in (m, None):
        got = _measure(x, Khd, Kwd, mask)
        torch.cuda.synchronize()
        want = R.A(x.double().cpu(), Kh, Kw, None if mask is None else mask.cpu())
        err = (got.double().cpu() - want).abs()
        print(f"measure {OPS[idx][1]} {shape} mask {mask is not None}: max |err| {float(err.max()):.3e}, largest err / bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
        if mask is not None:
            assert bool((got[mask == 0] == 0).all()) and bool((mask == 0).any())
    three = torch.cat([x.flip(0), x, x])[: shape[0] + 2].contiguous()
    again = _measure(three, Khd, Kwd, None)
    assert torch.equal(again[shape[0]:shape[0] + 1], _measure(x, Khd, Kwd, None)[:1])


# ------------------------------------------------------------------------------------------ 2. the adjoint kernel
@pytest.mark.parametrize("idx", range(len(OPS)))
def test_adjoint_vs_float64(idx):
    """g and sumsq of dmme_dps_adjoint against float64 on the same fp32 operands inside adjoint_bound; d_out = B_t g exactly; a two-plane
    network output uses its eps plane and gets a zero v plane in d_out; NaN in y on unmeasured cells changes no bit; the chain form
    (row read at the loop state's index, state untouched) gives the eager form's bits; sumsq of an image does not depend on the others"""
    shape, Kh, Kw, Khd, Kwd = _operator(idx)
    B, Cc, H, W = shape
    n, rows, ttab = _rows()
    i = 6
    row = rows[i]
    x, e = synth.normal(1, shape).cuda(), synth.normal(2, shape).cuda()
    ms = (B, Cc, Kh.shape[0], Kw.shape[0])
    m = _binary(ms, 5).cuda()
    y = (0.5 * synth.normal(3, ms)).cuda()
    g, d_out, ss = _adjoint(x, e, y, m, Khd, Kwd, row)
    torch.cuda.synchronize()
    want_g, _, want_ss, _ = R.adjoint(x.cpu(), e.cpu(), y.cpu(), m.cpu(), Kh, Kw, row, torch.float64)
    bg, bss = R.adjoint_bound(x, e, y, m, Kh, Kw, row)
    eg, ess = (g.double().cpu() - want_g).abs(), (ss.double().cpu() - want_ss).abs()
    print(f"adjoint {OPS[idx][1]} {shape}: g max |err| {float(eg.max()):.3e}, largest err / bound {float((eg / bg.clamp_min(1e-300)).max()):.3f}; sumsq max |err| "
          f"{float(ess.max()):.3e}, largest err / bound {float((ess / bss.clamp_min(1e-300)).max()):.3f}")
    assert bool(torch.isfinite(g).all()) and bool((eg <= bg).all()) and bool((ess <= bss).all())
    assert torch.equal(d_out, torch.tensor(row[4], device="cuda") * g)
    # two planes: the eps plane is read, the v plane's gradient is zero
    two = torch.cat([e, torch.full_like(e, float("nan"))], dim=1).contiguous()
    g2, d2, ss2 = _adjoint(x, two, y, m, Khd, Kwd, row, planes=2)
    assert torch.equal(g2, g) and torch.equal(ss2, ss) and torch.equal(d2[:, :Cc], d_out) and bool((d2[:, Cc:] == 0).all())
    # y is not looked at where nothing is measured
    ynan = torch.where(m != 0, y, torch.full_like(y, float("nan")))
    g3, d3, ss3 = _adjoint(x, e, ynan, m, Khd, Kwd, row)
    assert torch.equal(g3, g) and torch.equal(d3, d_out) and torch.equal(ss3, ss)
    # the chain form
    tabs = _Tables(rows, ttab)
    tabs.set(i, 9, 40)
    before = tabs.words()
    g4, d4, ss4 = _adjoint(x, e, y, m, Khd, Kwd, None, tabs=tabs)
    assert tabs.words() == before and torch.equal(g4, g) and torch.equal(d4, d_out) and torch.equal(ss4, ss)
    # a norm that mixed images would move this
    if B > 1:
        x5, e5, y5 = x.clone(), e.clone(), y.clone()
        x5[1:], e5[1:], y5[1:] = 3.0 * x5[1:] + 1.0, -e5[1:], y5[1:] + 2.0
        g5, _, ss5 = _adjoint(x5, e5, y5, m, Khd, Kwd, row)
        assert torch.equal(ss5[0], ss[0]) and torch.equal(g5[0], g[0]) and not torch.equal(ss5[1], ss[1])


# ------------------------------------------------------------------------------------------ 3. the update
@pytest.mark.parametrize("which", ["interior", "last"])
def test_update_vs_float64(which):
    """dmme_dps_step from given g, dx, sumsq and z against its float64 expression inside update_bound, on an interior row and on the last
    row (c2 = 0: z is not read); an image whose sumsq is 0 stays at u"""
    n, rows, ttab = _rows(zeta=0.7)
    row = rows[7] if which == "interior" else rows[1]
    assert (row[2] != 0.0) == (which == "interior") and row[5] != 0.0
    x, e, g, dx, z = (synth.normal(10 + k, SHAPE).cuda() for k in range(5))
    ss = torch.tensor([[0.5, 1.25, 2.0], [0.0, 0.0, 0.0]], device="cuda")
    zin = z if row[2] != 0.0 else None
    got = _eager(x.clone(), e, g, dx, ss, zin, row)
    torch.cuda.synchronize()
    want = R.update(x.cpu(), e.cpu(), g.cpu(), dx.cpu(), ss.cpu(), z.cpu(), row, torch.float64)
    bound = R.update_bound(x, e, g, dx, ss, z, row)
    err = (got.double().cpu() - want).abs()
    print(f"update {which}: max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    plain = R.update(x.cpu(), e.cpu(), g.cpu(), dx.cpu(), torch.zeros(2, 3), z.cpu(), row, torch.float64)
    assert float((want[0] - plain[0]).abs().max()) > 1e-3  # (the correction is there for image 0 ...)
    free = _eager(x.clone(), e, torch.full_like(g, float("nan")), torch.full_like(dx, float("nan")), ss, zin, row)
    assert torch.equal(free[1], got[1]) and bool(torch.isfinite(free[1]).all())  # (... and image 1, whose norm is 0, reads nothing of g and dx)


def test_zeta_zero_is_the_ddpm_step():
    """zeta = 0: bit-identical to dmme_ddpm_step with the same three coefficients, with NaN in g, dx and sumsq (none of them is read)"""
    L = _lib()
    n, rows, ttab = _rows(zeta=0.0)
    x, e, z = (synth.normal(20 + k, SHAPE).cuda() for k in range(3))
    nan, nss = torch.full_like(x, float("nan")), torch.full((2, 3), float("nan"), device="cuda")
    for row in (rows[7], rows[1]):
        got = _eager(x.clone(), e, nan, nan, nss, z, row)
        want = x.clone()
        L.check(L.lib().dmme_ddpm_step(L.ptr(want), L.ptr(e), L.ptr(z), row[0], row[1], row[2], int(row[2] != 0.0), want.numel(), L.stream_ptr()), "dmme_ddpm_step")
        assert torch.equal(got, want) and bool(torch.isfinite(got).all())


def test_eager_update_equals_the_chain_form():
    """dmme_chain_update_dps (row from the table, normals drawn in the kernel at a Philox offset above 2^32) against dmme_dps_step fed
    dmme_randn's normals, bit for bit over a 6-level walk; the loop state's words after every step"""
    import dmme_amd

    shape = (2, 3, 8, 12)
    numel = int(np.prod(shape))
    n4, seed, off0 = numel // 4, 0x1234567, (1 << 32) + 12
    n, rows, ttab = dmme_amd.DPS(torch.nn.Identity(), 100, 6, zeta=0.3)._chain_tables()
    assert n == 6 and rows[1][2] == 0.0 and all(r[2] != 0.0 for r in rows[2:])
    tabs = _Tables(rows, ttab)
    x = synth.normal(1, shape).cuda()
    twin = x.clone()
    ss = torch.tensor([[0.5, 1.0, 1.5], [2.0, 0.25, 0.125]], device="cuda")
    tabs.set(n, seed, off0)
    tabs.state[5:] = torch.tensor([41, 42, 43], device="cuda")
    for k, i in enumerate(range(n, 0, -1)):
        out, g, dx = (synth.normal(100 * j + i, shape).cuda() for j in (1, 2, 3))
        z = _randn(shape, seed, off0 + n4 * k)
        _chain_update(x, out, g, dx, ss, None, tabs)
        _eager(twin, out, g, dx, ss, z if rows[i][2] != 0.0 else None, rows[i])
        assert tabs.words() == [i - 1, ttab[i - 1], off0 + n4 * (k + 1), seed, 0, 41, 42, 43], i
        assert torch.equal(x, twin), f"chain form and eager form differ at loop index {i}"
        assert bool(torch.isfinite(x).all())
    # the override: the chain form on given normals
    tabs.set(n, seed, off0)
    a = _chain_update(synth.normal(1, shape).cuda(), out, g, dx, ss, z, tabs)
    assert torch.equal(a, _eager(synth.normal(1, shape).cuda(), out, g, dx, ss, z, rows[n]))


# ------------------------------------------------------------------------------------------ 4. - 7. on the networks
def _tiny(seed=11):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision="fp32")
    net.load_state_dict(O.make_state_dict(cfg, seed), strict=True)
    return net.cuda().eval()


def _oracle64(seed=11):
    cfg = O.TINY
    sd64 = {k: v.to(torch.float64) if v.is_floating_point() else v for k, v in O.make_state_dict(cfg, seed).items()}
    return lambda x, t: O.unet_forward(sd64, cfg, x, t)


def _image(seed, shape=SHAPE):
    return (0.5 * synth.normal(seed, shape)).clamp(-1.0, 1.0)


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def test_assembled_step_vs_float64():
    """one step through the runner (keep-forward, adjoint kernel, input-only backward, update in one captured graph): the dx buffer
    against float64 autograd of the oracle for the runner's own d_out, within 2e-5 of the gradient's max (the figure of
    tests/test_gpu_chain.py::test_input_gradient_vs_oracle_autograd for the tiny fp32 network); x' against the float64 update expression
    on the runner's own out, g, dx and sumsq, relative error at most 1e-5 (the figure of test_guided_steps_match_float64)"""
    import dmme_amd

    net = _tiny()
    op = dmme_amd.SeparableOperator.bicubic(32, 32, 4)
    proc = dmme_amd.DPS(net, 100, 8, operator=op, zeta=0.8).cuda()
    n, rows, ttab = proc._chain_tables()
    x = synth.normal(1, SHAPE).cuda()
    runner = proc.chain_runner(x.clone())
    assert isinstance(runner, dmme_amd.PosteriorChainRunner)
    m = _binary((2, 3, 8, 8), 9).cuda()
    runner.y.copy_(proc.degrade(_image(42).cuda(), m))
    runner.mask.copy_(m)
    model = _oracle64()
    for i in (6, 1):
        runner.x.copy_(x)
        runner.set(i, 5, 16)
        runner.step()
        torch.cuda.synchronize()
        assert runner.capture_error is None and runner.graph is not None
        xin = x.double().cpu().requires_grad_(True)
        eps = model(xin, torch.tensor([ttab[i]]))
        (want_dx,) = torch.autograd.grad(eps, xin, runner.d_out.double().cpu())
        edx = float((runner.dx.double().cpu() - want_dx).abs().max()) / float(want_dx.abs().max())
        z = _randn(SHAPE, 5, 16)
        want = R.update(x.cpu(), runner.out.cpu(), runner.g.cpu(), runner.dx.cpu(), runner.sumsq.cpu(), z.cpu(), rows[i], torch.float64)
        ex = _rel(runner.x, want)
        print(f"assembled step at index {i}: dx max |err| / max |dx| {edx:.3e} (bound 2e-5), x' relative error {ex:.3e} (bound 1e-5), "
              f"forward max |err| {float((runner.out.double().cpu() - eps.detach()).abs().max()):.3e}")
        assert edx <= 2e-5 and ex <= 1e-5
        assert float(runner.sumsq.sum()) > 0 and float((runner.x - R.update(x.cpu(), runner.out.cpu(), runner.g.cpu(), runner.dx.cpu(), torch.zeros(2, 3), z.cpu(),
                                                                               rows[i], torch.float64).float().cuda()).abs().max()) > 1e-4


@pytest.mark.parametrize("name,masked", [("blur", False), ("bicubic", True)])
def test_captured_chain_equals_the_eager_loop(name, masked):
    """`restore` (one hipGraph of keep-forward + adjoint + input-backward + draw + update + state advance, replayed) against the host loop
    over the eager entry points, bit for bit under the same seed; 8 levels over T = 100; torch's generator moves by numel (1 + n_rows)
    either way; a second chain re-uses the graph; a HistoryRecorder changes nothing; `generate` measures nothing and equals its eager loop"""
    import dmme_amd

    net = _tiny()
    op = dmme_amd.SeparableOperator.preset(name, 32, 32, blur_size=5, blur_sigma=1.5, scale=4)
    proc = dmme_amd.DPS(net, 100, 8, operator=op, zeta=0.6, sigma_y=0.05).cuda()
    assert proc.n_rows == 8
    numel, img = int(np.prod(SHAPE)), _image(42).cuda()
    clean = proc.degrade(img, noise=False)
    assert torch.equal(clean, _measure(img, *op.device(img.device), None)) and tuple(clean.shape) == (2, 3, op.h, op.w)
    m = _binary(tuple(clean.shape), 9).cuda() if masked else None
    torch.manual_seed(3)
    y = proc.degrade(img, m)
    assert not torch.equal(y, clean) and (m is None or bool((y[m == 0] == 0).all()))
    torch.manual_seed(77)
    before = _gen_offset()
    a = proc.restore(y, m)
    assert _gen_offset() - before == numel * (1 + proc.n_rows)
    runner, graph = proc._runner, proc._runner.graph
    assert isinstance(runner, dmme_amd.PosteriorChainRunner) and runner.capture_error is None and graph is not None
    torch.manual_seed(78)
    b = proc.restore(y, m)
    assert proc._runner is runner and runner.graph is graph and runner.capture_error is None and not torch.equal(a, b) and tuple(a.shape) == SHAPE
    mm = torch.ones_like(y) if m is None else m
    with torch.no_grad():
        for seed, got in ((77, a), (78, b)):
            torch.manual_seed(seed)
            before = _gen_offset()
            x = dmme_amd.gaussian(SHAPE, device="cuda")
            assert torch.equal(got, proc._eager_chain(x, y, mm)) and bool(torch.isfinite(got).all())
            assert _gen_offset() - before == numel * (1 + proc.n_rows)
        torch.manual_seed(77)
        gen = proc.generate(SHAPE)
        torch.manual_seed(77)
        zeros = torch.zeros_like(y)
        assert torch.equal(gen, proc._eager_chain(dmme_amd.gaussian(SHAPE, device="cuda"), zeros, zeros)) and not torch.equal(gen, a) and proc._runner is runner
    ords = dmme_amd.history_ordinals(proc.chain_length(), 4)
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    torch.manual_seed(77)
    c = proc.restore(y, m, history=rec)
    assert rec.recorded == 4 == len(ords) and torch.equal(a, c)


def test_guidance_reduces_the_residual():
    """Gaussian deblurring (5 taps, sigma 1.5) of a noiseless measurement on the tiny random UNet, zeta = 4, 10 levels over T = 100, seed
    77: the float64 restatement on the CPU (tests/dps_ref.py, on the normals the device draws) ends at
    ||y - A x|| / ||y - A x(zeta = 0)|| = 0.3141 (measured: 14.68 against 46.73; the GPU chain gave the same four digits), which must be below 0.5; the GPU chain's ratio under the same seed, printed, must be
    below 1.  (A random network is no denoiser: the ratio says that the gradient step pulls towards the measurement, nothing about images.)"""
    import dmme_amd
    from dmme_amd.common.noise import philox_reserve

    net = _tiny()
    zeta, n = 4.0, 10
    op = dmme_amd.SeparableOperator.gaussian_blur(32, 32, 5, 1.5)
    Kh, Kw = (K.double() for K in op.device("cpu"))  # (the fp32 matrices the device reads)
    proc, free = (dmme_amd.DPS(net, 100, n, operator=op, zeta=z).cuda() for z in (zeta, 0.0))
    y = proc.degrade(_image(42).cuda())
    numel = int(np.prod(SHAPE))
    got = []
    for p in (proc, free):
        torch.manual_seed(77)
        got.append(p.restore(y))
    gpu = [R.residual_norm(x.cpu(), y.cpu(), None, Kh, Kw) for x in got]
    # the same chain in float64 on the CPU, on the device's normals
    torch.manual_seed(77)
    x_T = dmme_amd.gaussian(SHAPE, device="cuda")
    seed, off = philox_reserve(x_T.device, numel * n)
    normals = [_randn(SHAPE, seed, off + (numel // 4) * k).cpu() for k in range(n)]
    model, cpu = _oracle64(), []
    for p in (proc, free):
        _, rows, ttab = p._chain_tables()
        x = R.chain(model, x_T.cpu(), y.cpu(), None, Kh, Kw, rows, ttab, normals, torch.float64)[0]
        cpu.append(R.residual_norm(x, y.cpu(), None, Kh, Kw))
    print(f"guidance: float64 CPU ||y - A x|| {cpu[0]:.4f} against {cpu[1]:.4f} unguided, ratio {cpu[0] / cpu[1]:.4f} (bound 0.5); GPU {gpu[0]:.4f} against "
          f"{gpu[1]:.4f}, ratio {gpu[0] / gpu[1]:.4f} (bound 1)")
    assert cpu[0] / cpu[1] < 0.5 and gpu[0] / gpu[1] < 1.0 and all(bool(torch.isfinite(x).all()) for x in got)


def test_bf16_default_unet_smoke():
    """the default UNet in bf16 at batch 8, 4 levels: two `restore` calls under one seed are finite and bit-equal, through one graph"""
    import dmme_amd

    net = dmme_amd.UNet(precision="bf16")
    net.load_state_dict(O.make_state_dict(O.UNetConfig(), 5))
    net.cuda().eval()
    shape = (8, 3, 32, 32)
    op = dmme_amd.SeparableOperator.gaussian_blur(32, 32, 5, 1.5)
    proc = dmme_amd.DPS(net, 1000, 4, operator=op, zeta=0.5).cuda()
    y = proc.degrade(_image(42, shape).cuda())
    torch.manual_seed(1)
    a = proc.restore(y)
    runner = proc._runner
    torch.manual_seed(1)
    b = proc.restore(y)
    assert runner.capture_error is None and runner.graph is not None and proc._runner is runner
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and tuple(a.shape) == shape


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    """the library's status and message, not a launch: a conditional plan, a classifier plan, a v-prediction plan, a thresholded plan,
    kind 13 handed to dmme_chain_step, a plane above dmme_dps_capacity(), h > H, W % 4 != 0; x unchanged afterwards"""
    import dmme_amd

    L = _lib()
    lib = L.lib()
    net = _tiny()
    op = dmme_amd.SeparableOperator.average(32, 32, 4)
    proc = dmme_amd.DPS(net, 100, 8, operator=op).cuda()
    x = synth.normal(1, SHAPE).cuda()
    runner = proc.chain_runner(x)
    packed = runner._packed()
    runner.set(8, 1, 0)
    dev = x.device

    def step(plan, pk=None, pb=None, bws=None):
        pk = packed if pk is None else pk
        return lib.dmme_dps_chain_step(plan.h, L.ptr(pk), L.ptr(runner.plan.packed_bwd if pb is None else pb), L.ptr(runner.x), L.ptr(runner.out), L.ptr(plan.workspace),
                                       L.ptr(runner.plan.bws if bws is None else bws), L.ptr(runner.y), L.ptr(runner.mask), L.ptr(runner.Kh), L.ptr(runner.Kw), 8, 8,
                                       L.ptr(runner.g), L.ptr(runner.d_out), L.ptr(runner.dx), L.ptr(runner.sumsq), L.ptr(runner.coef), L.ptr(runner.ttab),
                                       L.ptr(runner.state), L.stream_ptr())

    before = x.clone()
    tiny_kw = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    cnet = dmme_amd.ConditionalUNet(precision="fp32", num_classes=5, dropout=0.0, **tiny_kw).cuda().eval()
    assert step(cnet._plan_for(2, 32, 32, dev)) == -1 and b"class-conditional" in lib.dmme_last_error()
    cls = dmme_amd.EncoderClassifier(precision="fp32", num_classes=5, **tiny_kw).cuda().eval()
    assert step(cls._plan_for(2, 32, 32, dev)) == -1 and b"unconditional DMME_ARCH_DDPM or DMME_ARCH_IDDPM" in lib.dmme_last_error()
    plan = runner.plan
    ab = torch.linspace(1.0, 0.01, 101, device="cuda").repeat_interleave(2).contiguous()
    L.check(lib.dmme_unet_plan_set_prediction(plan.h, L.PRED_V, L.ptr(ab), 100))
    assert step(plan) == -2 and b"adapter" in lib.dmme_last_error()
    L.check(lib.dmme_unet_plan_set_prediction(plan.h, L.PRED_EPS, None, 100))
    tab = torch.ones(4 * 101, device="cuda")
    L.check(lib.dmme_unet_plan_set_threshold(plan.h, L.THRESHOLD_STATIC, L.ptr(tab), 100, 0, 0.0, None))
    assert step(plan) == -2 and b"clip" in lib.dmme_last_error()
    L.check(lib.dmme_unet_plan_set_threshold(plan.h, L.THRESHOLD_NONE, None, 100, 0, 0.0, None))
    assert lib.dmme_chain_step(plan.h, L.ptr(packed), L.ptr(runner.x), L.ptr(runner.out), L.ptr(plan.workspace), L.CHAIN_DPS, L.ptr(runner.coef), L.ptr(runner.ttab),
                               L.ptr(runner.state), L.stream_ptr()) == -1 and b"chain_step: sampler kind 13" in lib.dmme_last_error()
    # the plane-wise launches' own checks
    cap = int(lib.dmme_dps_capacity())
    assert 64 * 64 <= cap < 64 * 128
    big = torch.ones(1, 1, 64, 128, device="cuda")
    K64, K128 = torch.eye(64, device="cuda"), torch.eye(128, device="cuda")
    yb = torch.full((1, 1, 64, 128), 7.0, device="cuda")
    assert lib.dmme_dps_measure(L.ptr(big), L.ptr(K64), L.ptr(K128), None, L.ptr(yb), 1, 1, 64, 128, 64, 128, L.stream_ptr()) == -2
    assert str(cap).encode() in lib.dmme_last_error()
    row = (C.c_float * 8)(*proc._chain_tables()[1][8])
    g, d_out, ss = torch.full_like(x, 7.0), torch.full_like(x, 7.0), torch.full((2, 3), 7.0, device="cuda")
    K40 = torch.ones(40, 32, device="cuda")
    y40 = torch.zeros(2, 3, 40, 8, device="cuda")
    assert lib.dmme_dps_adjoint(L.ptr(x), L.ptr(runner.out), 1, row, L.ptr(y40), None, L.ptr(K40), L.ptr(runner.Kw), L.ptr(g), L.ptr(d_out), L.ptr(ss), 2, 3, 32, 32,
                                40, 8, L.stream_ptr()) == -1 and b"h <= H" in lib.dmme_last_error()
    odd = torch.zeros(2, 2, 6, 6, device="cuda")
    K6 = torch.eye(6, device="cuda")
    assert lib.dmme_dps_adjoint(L.ptr(odd), L.ptr(odd), 1, row, L.ptr(odd), None, L.ptr(K6), L.ptr(K6), L.ptr(odd.clone()), L.ptr(odd.clone()), L.ptr(ss), 2, 2, 6, 6,
                                6, 6, L.stream_ptr()) == -2 and b"multiples of 4" in lib.dmme_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((yb == 7.0).all()) and bool((g == 7.0).all()) and bool((ss == 7.0).all())  # nothing was launched
    with pytest.raises(NotImplementedError):
        dmme_amd.DPS(net, 100, 8, prediction="v")
    with pytest.raises(NotImplementedError):
        dmme_amd.DPS(net, 100, 8, threshold="static")
