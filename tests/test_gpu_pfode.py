"""-m gpu: the probability-flow ODE (dmme_amd.ProbabilityFlow) on the MI355X - the Rademacher probe and the dequantisation bit for bit against
the restatement (tests/pfode_ref.py, on tests/philox_ref.py's words), the stage update, the probe dot with its double accumulator and the
latent's log-density against float64 under derived bounds (stage_bound, dot_bound, prior_bound: built from the precision of fp32 and the
number of rounded operations, not measured; tests/test_pfode_host.py shows on the CPU that plain fp32 sits inside the stage bound), the eager
forms against the chain forms, one assembled likelihood stage against float64 autograd of the oracle, the whole walk against the eager loop
(bit for bit) and against the free-running float64 restatement on the device's own probes, decode / encode, the round trip against
GeneralizedDDIM's, bf16, and the refusals.  Every comparison prints its figures."""

import ctypes as C

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import pfode_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 32, 32)
SHAPES = [(1, 3, 5, 7), SHAPE]  # 105 values: the element tail and an odd row; two images of 3072: quads, more than one block and part
GRID = [1, 26, 50, 75, 100]
SEED, OFF = 0x1234567, (1 << 32) + 12  # (a Philox offset above 2^32)


def _lib():
    from dmme_amd import _lib

    return _lib


class _Tables:
    def __init__(self, rows, ttab):
        self.coef = torch.tensor(np.asarray(rows), dtype=torch.float32).reshape(-1).cuda()
        self.ttab = torch.tensor(ttab, dtype=torch.int64).cuda()
        self.state = torch.zeros(8, dtype=torch.int64, device="cuda")

    def set(self, i, seed, off):
        L = _lib()
        L.check(L.lib().dmme_chain_set(L.ptr(self.state), i, L.ptr(self.ttab), seed, off, L.stream_ptr()))

    def words(self):
        torch.cuda.synchronize()
        return [int(v) for v in self.state.cpu()]


def _rows32(likelihood=True, direction="encode"):
    """the package's fp32 rows of GRID over T = 100: (n, rows as python floats, t_table)"""
    import dmme_amd

    return dmme_amd.ProbabilityFlow(torch.nn.Identity(), 100, grid=GRID)._tables["likelihood" if likelihood else direction]


def _row(row):
    return (C.c_float * 8)(*[float(v) for v in row])


def _gen_offset():
    return int(torch.cuda.default_generators[torch.cuda.current_device()].get_offset())


def _gen_seed():
    return int(torch.cuda.default_generators[torch.cuda.current_device()].initial_seed()) & 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------ 1. probe and dequantisation
@pytest.mark.parametrize("shape", SHAPES)
def test_rademacher_and_probe_bit_exact(shape):
    """dmme_rademacher writes the restatement's +-1 and nothing past numel; dmme_pf_probe the same values into the eps plane of a one- and a
    two-plane buffer with an all-zero v plane; the chain form reads (seed, offset) at the loop state and leaves the state alone"""
    L = _lib()
    lib = L.lib()
    B, chw = shape[0], int(np.prod(shape[1:]))
    numel = B * chw
    want = R.rademacher(SEED, OFF, numel)
    out = torch.full((numel + 5,), 7.0, device="cuda")
    L.check(lib.dmme_rademacher(L.ptr(out), numel, SEED, OFF, L.stream_ptr()), "dmme_rademacher")
    torch.cuda.synchronize()
    assert np.array_equal(out[:numel].cpu().numpy(), want) and bool((out[numel:] == 7.0).all())
    n, rows, ttab = _rows32()
    tabs = _Tables(rows, ttab)
    tabs.set(n, SEED, OFF)
    before = tabs.words()
    for planes in (1, 2):
        ref = R.probe(SEED, OFF, B, chw, planes)
        d = torch.full((B, planes * chw), float("nan"), device="cuda")
        L.check(lib.dmme_pf_probe(L.ptr(d), B, chw, planes, SEED, OFF, L.stream_ptr()), "dmme_pf_probe")
        d2 = torch.full_like(d, float("nan"))
        L.check(lib.dmme_chain_probe_pf(L.ptr(d2), L.ptr(tabs.state), B, chw, planes, L.stream_ptr()), "dmme_chain_probe_pf")
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), ref) and torch.equal(d, d2), planes
        assert planes == 1 or not bool(d[:, chw:].any())
    assert tabs.words() == before


@pytest.mark.parametrize("shape", SHAPES)
def test_dequantize_bit_exact(shape):
    """x += (u - 0.5) * fp32(2 / 255) with the contract's u: the restatement's bits, nothing past numel"""
    L = _lib()
    numel = int(np.prod(shape))
    x = synth.normal(3, (numel,))
    buf = torch.cat([x, torch.full((3,), 7.0)]).cuda()
    L.check(L.lib().dmme_pf_dequantize(L.ptr(buf), numel, SEED, OFF, L.stream_ptr()), "dmme_pf_dequantize")
    torch.cuda.synchronize()
    assert np.array_equal(buf[:numel].cpu().numpy(), R.dequantize(x.numpy(), SEED, OFF)) and bool((buf[numel:] == 7.0).all())


# ------------------------------------------------------------------------------------------ 2. the stage update
def _stage(x, out, planes, xs, es, row=None, tabs=None, advance=0):
    L = _lib()
    B, chw = x.shape[0], x[0].numel()
    if tabs is None:
        L.check(L.lib().dmme_pf_stage(L.ptr(x), L.ptr(out), planes, L.ptr(xs), L.ptr(es), _row(row), B, chw, L.stream_ptr()), "dmme_pf_stage")
    else:
        L.check(L.lib().dmme_chain_stage_pf(L.ptr(x), L.ptr(out), planes, L.ptr(xs), L.ptr(es), L.ptr(tabs.coef), L.ptr(tabs.ttab), L.ptr(tabs.state), advance, B, chw,
                                            L.stream_ptr()), "dmme_chain_stage_pf")


@pytest.mark.parametrize("shape", SHAPES)
def test_stage_vs_float64(shape):
    """dmme_pf_stage against float64 inside stage_bound, elementwise, for an A row, a B row, the closing Euler row and a row with all four
    terms, on a one- and a two-plane network output (whose v plane is NaN: never read).  The save rule: xs, es take (x, e) from before
    the update exactly where the row says so and are untouched otherwise; a buffer whose coefficient is 0 may hold NaN"""
    n, rows, ttab = _rows32(False, "decode")
    full = (0.7, -1.3, 0.2, 2.5, 0.0, 1.0, 0.0, 0.0)
    x, xs, e, es = (3.0 * synth.normal(10 + k, shape) for k in range(4))
    nan = torch.full(shape, float("nan"))
    for name, row in (("A", rows[n]), ("B", rows[n - 1]), ("euler", rows[1]), ("full", full)):
        reads_s, reads_e = row[1] != 0.0, row[3] != 0.0
        xs_in, es_in = (xs if reads_s else nan), (es if reads_e else nan)
        want, wxs, wes = R.stage(x, xs_in, e, es_in, np.asarray(row, dtype=np.float64))
        bound = R.stage_bound(x, xs, e, es, row)
        for planes in (1, 2):
            out = e if planes == 1 else torch.cat([e.reshape(shape[0], -1), nan.reshape(shape[0], -1)], dim=1)
            gx, gxs, ges = x.clone().cuda(), xs_in.clone().cuda(), es_in.clone().cuda()
            _stage(gx, out.contiguous().cuda(), planes, gxs, ges, row)
            torch.cuda.synchronize()
            err = (gx.double().cpu() - want).abs()
            print(f"stage {name} {shape} planes {planes}: max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
            assert bool(torch.isfinite(gx).all()) and bool((err <= bound).all())
            assert torch.equal(gxs.cpu(), wxs.float()) or (not reads_s and row[5] == 0.0 and bool(torch.isnan(gxs).all()))
            assert torch.equal(ges.cpu(), wes.float()) or (not reads_e and row[5] == 0.0 and bool(torch.isnan(ges).all()))
            if row[5] != 0.0:
                assert torch.equal(gxs.cpu(), x) and torch.equal(ges.cpu(), e)


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 8, 12)])
def test_eager_stage_equals_the_chain_form(shape):
    """dmme_chain_stage_pf (row read at the loop state's index) against dmme_pf_stage, bit for bit over the whole likelihood table; the loop
    state's words after every stage: i - 1, t_table[i - 1], the offset moved by B*chw/4 where asked (only where chw is a multiple of 4:
    refused otherwise, before any launch) and left alone where not"""
    L = _lib()
    n, rows, ttab = _rows32()
    tabs = _Tables(rows, ttab)
    numel = int(np.prod(shape))
    advance = 1 if shape[1] * shape[2] * shape[3] % 4 == 0 else 0
    x = synth.normal(1, shape).cuda()
    twin = x.clone()
    xs, es, txs, tes = (torch.full_like(x, float("nan")) for _ in range(4))
    tabs.set(n, SEED, OFF)
    tabs.state[5:] = torch.tensor([41, 42, 43], device="cuda")
    if not advance:
        assert L.lib().dmme_chain_stage_pf(L.ptr(x), L.ptr(x), 1, L.ptr(xs), L.ptr(es), L.ptr(tabs.coef), L.ptr(tabs.ttab), L.ptr(tabs.state), 1, shape[0],
                                           numel // shape[0], L.stream_ptr()) == -2 and b"multiple of 4" in L.lib().dmme_last_error()
    for k, i in enumerate(range(n, 0, -1)):
        out = synth.normal(100 + i, shape).cuda()
        _stage(x, out, 1, xs, es, tabs=tabs, advance=advance)
        _stage(twin, out, 1, txs, tes, row=rows[i])
        assert tabs.words() == [i - 1, ttab[i - 1], OFF + advance * (numel // 4) * (k + 1), SEED, 0, 41, 42, 43], i
        assert torch.equal(x, twin) and torch.equal(xs, txs) and torch.equal(es, tes), f"chain form and eager form differ at loop index {i}"
        assert bool(torch.isfinite(x).all())


# ------------------------------------------------------------------------------------------ 3. the probe dot, the accumulator, the prior
def _dot(d_out, planes, dx, acc, row=None, tabs=None):
    """(s, acc) of the eager form, or of the chain form at the loop state of `tabs`; acc is updated in place"""
    L = _lib()
    lib = L.lib()
    B, chw = dx.shape[0], dx[0].numel()
    scratch = torch.full((int(lib.dmme_pf_scratch_floats(B, chw)),), float("nan"), device="cuda")
    s = torch.full((B,), float("nan"), device="cuda")
    if tabs is None:
        L.check(lib.dmme_pf_dot(L.ptr(d_out), planes, L.ptr(dx), _row(row), B, chw, L.ptr(scratch), L.ptr(s), L.ptr(acc), L.stream_ptr()), "dmme_pf_dot")
    else:
        L.check(lib.dmme_chain_dot_pf(L.ptr(d_out), planes, L.ptr(dx), L.ptr(tabs.coef), L.ptr(tabs.state), B, chw, L.ptr(scratch), L.ptr(s), L.ptr(acc), L.stream_ptr()),
                "dmme_chain_dot_pf")
    torch.cuda.synchronize()
    return s


@pytest.mark.parametrize("shape", SHAPES)
def test_dot_and_accumulator(shape):
    """s = sum z dx per image inside dot_bound of float64, read from the eps plane of a one- and a two-plane d_out; the accumulator moves by
    (double)w * (double)s, checked against that float64 expression on the device's own s (two roundings of a double: one ulp of the larger
    term); the chain form (w read at the loop state's index, state untouched) gives the same bits; an image gives the same bits alone and
    at another place of a batch of 3"""
    n, rows, ttab = _rows32()
    i = n - 1
    w = float(np.float32(rows[i][4]))
    B, chw = shape[0], int(np.prod(shape[1:]))
    z = torch.from_numpy(R.probe(SEED, OFF, B, chw, 1)).reshape(shape)
    dx = 3.0 * synth.normal(5, shape) + 0.25
    want, bound = R.dot(z, dx), R.dot_bound(z, dx)
    acc0 = torch.tensor([123.456789012345 + b for b in range(B)], dtype=torch.float64)
    tabs = _Tables(rows, ttab)
    tabs.set(i, SEED, OFF)
    before = tabs.words()
    got = {}
    for planes in (1, 2):
        d_out = z.reshape(B, -1) if planes == 1 else torch.cat([z.reshape(B, -1), torch.full((B, chw), float("nan"))], dim=1)
        d_out = d_out.contiguous().cuda()
        acc = acc0.clone().cuda()
        s = _dot(d_out, planes, dx.cuda(), acc, row=rows[i])
        err = (s.double().cpu() - want).abs()
        print(f"dot {shape} planes {planes}: s {[round(float(v), 4) for v in s]}, max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        want_acc = acc0 + w * s.double().cpu()
        assert bool(((acc.cpu() - want_acc).abs() <= 2.0 ** -52 * (acc0.abs() + (w * s.double().cpu()).abs())).all()) and not torch.equal(acc.cpu(), acc0)
        acc2 = acc0.clone().cuda()
        s2 = _dot(d_out, planes, dx.cuda(), acc2, tabs=tabs)
        assert torch.equal(s2, s) and torch.equal(acc2, acc)
        got[planes] = s
    assert torch.equal(got[1], got[2]) and tabs.words() == before
    # the same image at another place of a batch of 3
    z3, dx3 = torch.cat([z.flip(0), z, z])[:3].contiguous(), torch.cat([dx.flip(0) * 2.0, dx, dx])[:3].contiguous()
    at = B  # image 0 of the original batch sits at index B of the larger one (B = 1: index 1; B = 2: index 2)
    s3 = _dot(z3.reshape(3, -1).cuda(), 1, dx3.cuda(), torch.zeros(3, dtype=torch.float64, device="cuda"), row=rows[i])
    assert torch.equal(s3[at:at + 1], got[1][:1])


@pytest.mark.parametrize("shape", SHAPES)
def test_prior_vs_float64(shape):
    """dmme_pf_prior = -(1/2) sum x^2 - (D/2) ln(2 pi) per image in double, inside prior_bound of float64; the same bits alone and in a batch of 3"""
    L = _lib()
    lib = L.lib()

    def prior(x):
        B, chw = x.shape[0], x[0].numel()
        scratch = torch.full((int(lib.dmme_pf_scratch_floats(B, chw)),), float("nan"), device="cuda")
        out = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
        L.check(lib.dmme_pf_prior(L.ptr(x), B, chw, L.ptr(scratch), L.ptr(out), L.stream_ptr()), "dmme_pf_prior")
        torch.cuda.synchronize()
        return out

    x = 1.3 * synth.normal(8, shape) + 0.1
    got = prior(x.cuda())
    want, bound = R.prior(x), R.prior_bound(x)
    err = (got.cpu() - want).abs()
    print(f"prior {shape}: {[round(float(v), 4) for v in got]}, max |err| {float(err.max()):.3e}, largest err / bound {float((err / bound).max()):.3f}")
    assert got.dtype == torch.float64 and bool((err <= bound + 1e-12).all())
    three = torch.cat([x.flip(0) * 2.0, x, x])[:3].contiguous()
    assert torch.equal(prior(three.cuda())[shape[0]:shape[0] + 1], got[:1])


# ------------------------------------------------------------------------------------------ 4. - 8. on the networks
def _tiny(seed=11, precision="fp32"):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision=precision)
    net.load_state_dict(O.make_state_dict(cfg, seed), strict=True)
    return net.cuda().eval()


def _oracle(seed=11, dtype=torch.float64):
    cfg = O.TINY
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in O.make_state_dict(cfg, seed).items()}
    return lambda x, t: O.unet_forward(sd, cfg, x, t)


def _image(seed=42, shape=SHAPE):
    return (0.5 * synth.normal(seed, shape)).clamp(-1.0, 1.0)


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _flow(net=None, **kw):
    import dmme_amd

    kw.setdefault("grid", GRID)
    return dmme_amd.ProbabilityFlow(_tiny() if net is None else net, 100, **kw).cuda()


def test_assembled_likelihood_stage_vs_float64():
    """one likelihood stage through the runner (keep-forward, probe, input-only backward, dot, stage update in one captured graph), at a
    stage A and at a stage B index: the probe is the restatement's; runner.dx against float64 autograd of the oracle for the runner's own
    probe, within 2e-5 of the gradient's max (the figure of tests/test_gpu_chain.py::test_input_gradient_vs_oracle_autograd for the tiny fp32
    network); s against the float64 dot of the runner's own z and dx under dot_bound; s against the oracle's z^T J z under
    D * 2e-5 * max |dx64|, which follows from the same figure; acc = w s; the capture succeeded"""
    import dmme_amd

    proc = _flow()
    n, rows, ttab = proc._tables["likelihood"]
    x = _image().cuda()
    runner = proc._flow_runner("likelihood", SHAPE, x.device, dmme_amd.LikelihoodChainRunner)
    assert isinstance(runner, dmme_amd.LikelihoodChainRunner) and runner.draws
    model = _oracle()
    B, D = SHAPE[0], int(np.prod(SHAPE[1:]))
    for i in (n, 3):
        runner.x.copy_(x)
        runner.acc.zero_()
        runner.set(i, 5, 16)
        runner.step()
        torch.cuda.synchronize()
        assert runner.capture_error is None and runner.graph is not None
        z = runner.d_out.cpu()
        assert np.array_equal(z.reshape(B, -1).numpy(), R.probe(5, 16, B, D, 1))
        xin = x.double().cpu().requires_grad_(True)
        eps = model(xin, torch.tensor([ttab[i]]))
        (dx64,) = torch.autograd.grad(eps, xin, z.double())
        edx = float((runner.dx.double().cpu() - dx64).abs().max()) / float(dx64.abs().max())
        s = runner.s.double().cpu()
        own, own_bound = R.dot(z, runner.dx.cpu()), R.dot_bound(z, runner.dx.cpu())
        want, bound = R.dot(z, dx64), D * 2e-5 * float(dx64.abs().max())
        es = (s - want).abs()
        print(f"likelihood stage at index {i} (t = {ttab[i]}): dx max |err| / max |dx| {edx:.3e} (bound 2e-5); s {[round(float(v), 4) for v in s]}, against its own "
              f"float64 dot: largest err / bound {float(((s - own).abs() / own_bound).max()):.3f}; against the oracle's z^T J z: max |err| {float(es.max()):.3e}, "
              f"bound {bound:.3e}, ratio {float(es.max()) / bound:.3e}")
        assert edx <= 2e-5
        assert bool(((s - own).abs() <= own_bound).all())
        assert bool((es <= bound).all())
        w = float(np.float32(rows[i][4]))
        assert w != 0.0 and torch.equal(runner.acc.cpu(), w * s)


def test_whole_walk_captured_eager_and_float64():
    """`log_likelihood` (one hipGraph per stage, replayed) equals the host loop over the eager entry points bit for bit under one seed; a
    second call re-uses the graph; torch's generator moves by numel * stages either way; log_p, prior and divergence against the free-running
    float64 restatement fed the device's own probes (re-created from (seed, offset) by the restatement) under
    sum_k |w_k| D 2e-5 max |dx64_k|, with no further term (the float32 restatement on the CPU sits at 2.5e-5 nats); bits/dim follows"""
    import dmme_amd

    proc = _flow()
    assert np.array_equal(proc._ab64, R.alpha_bar(100))
    n, rows, ttab = proc._tables["likelihood"]
    numel, D = int(np.prod(SHAPE)), int(np.prod(SHAPE[1:]))
    x0 = _image()
    torch.manual_seed(77)
    before = _gen_offset()
    a = proc.log_likelihood(x0.cuda())
    assert _gen_offset() - before == numel * n and n == 8
    runner = proc._pf_runner_likelihood
    graph = runner.graph
    assert isinstance(runner, dmme_amd.LikelihoodChainRunner) and runner.capture_error is None and graph is not None
    torch.manual_seed(77)
    b = proc.log_likelihood(x0.cuda())
    assert proc._pf_runner_likelihood is runner and runner.graph is graph and runner.capture_error is None
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    torch.manual_seed(78)
    c = proc.log_likelihood(x0.cuda())
    assert not torch.equal(c.divergence, a.divergence) and runner.graph is graph
    with torch.no_grad():
        torch.manual_seed(77)
        before = _gen_offset()
        latent, acc = proc._eager_likelihood(x0.clone().cuda())
        torch.cuda.synchronize()
        assert _gen_offset() - before == numel * n
    assert torch.equal(latent, a.latent) and torch.equal(acc, a.divergence) and bool(torch.isfinite(a.log_p).all())
    assert a.log_p.dtype == a.prior.dtype == a.divergence.dtype == torch.float64 and tuple(a.latent.shape) == SHAPE
    # the float64 restatement on the device's probes
    torch.manual_seed(77)
    seed, off = _gen_seed(), _gen_offset() // 4
    probes = lambda k: torch.from_numpy(R.rademacher(seed, off + k * (numel // 4), numel)).reshape(SHAPE)
    ref = R.likelihood(_oracle(), x0, proc._ab64, GRID, probes)
    bound = sum(abs(w) * D * 2e-5 * m for w, m in zip(ref["w"], ref["dxmax"]))
    errs = {k: float((getattr(a, k2).cpu() - ref[k]).abs().max()) for k, k2 in (("log_p", "log_p"), ("prior", "prior"), ("acc", "divergence"))}
    print(f"whole walk: log p {[round(float(v), 3) for v in a.log_p]} (float64 {[round(float(v), 3) for v in ref['log_p']]}), |err| log_p {errs['log_p']:.3e}, prior "
          f"{errs['prior']:.3e}, divergence {errs['acc']:.3e}; bound {bound:.3e}; ratio {max(errs.values()) / bound:.3e}; x_T relative error "
          f"{_rel(a.latent, ref['latent']):.3e}; per-stage traces between {min(float(s.min()) for s in ref['s']):.1f} and {max(float(s.max()) for s in ref['s']):.1f}")
    assert all(e <= bound for e in errs.values())
    bpd = proc.bits_per_dim(x0.cuda())
    assert bpd.dtype == torch.float64 and float((bpd.cpu() - R.bits_per_dim(ref["log_p"], D)).abs().max()) <= bound / (D * np.log(2.0))
    # dequantisation first: its span, then the walk's
    torch.manual_seed(77)
    before = _gen_offset()
    d = proc.log_likelihood(x0.cuda(), dequantize=True)
    assert _gen_offset() - before == numel * (n + 1) and bool(torch.isfinite(d.log_p).all()) and not torch.equal(d.log_p, a.log_p)


@pytest.mark.parametrize("planes", [1, 2])
def test_decode_encode_vs_float64(planes):
    """`decode` and `encode` in fp32 over the 4 steps of GRID against the float64 restatement, relative error at most 1e-5 (the figure
    tests/test_gpu_dps.py takes from test_guided_steps_match_float64); the captured chain equals the eager loop bit for bit; nothing is drawn;
    a HistoryRecorder changes nothing; final_denoise=False ends at t_min.  planes = 2: an IDDPM network, whose eps plane the walk reads"""
    import dmme_amd

    if planes == 2:
        from dmme_amd.models.iddpm import UNet as IUNet
        from oracle import iddpm as OI

        icfg = OI.TINY
        inet = IUNet(icfg.in_channels, icfg.pos_dim, icfg.emb_dim, icfg.num_groups, icfg.dropout, icfg.channels_per_depth, icfg.num_blocks, icfg.attention_depths,
                     precision="fp32", num_heads=icfg.num_heads)
        sd = OI.make_state_dict(icfg, 11)
        inet.load_state_dict(sd, strict=True)
        sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
        model = lambda x, t: OI.unet_forward(sd64, icfg, x, t)
        proc = _flow(inet.cuda().eval())
    else:
        model = _oracle()
        proc = _flow()
    x_T, x0 = synth.normal(1, SHAPE), _image()
    before = _gen_offset()
    dec = proc.decode(x_T.cuda())
    raw = proc.decode(x_T.cuda(), final_denoise=False)
    enc = proc.encode(x0.cuda())
    assert _gen_offset() == before
    for name in ("decode", "decode_raw", "encode"):
        r = getattr(proc, f"_pf_runner_{name}")
        assert isinstance(r, dmme_amd.FlowChainRunner) and r.capture_error is None and r.graph is not None and not r.draws
        assert r.out.shape[1] == planes * SHAPE[1]
    want = {"decode": R.walk(model, x_T, proc._ab64, GRID, "decode"), "raw": R.walk(model, x_T, proc._ab64, GRID, "decode", final_denoise=False),
            "encode": R.walk(model, x0, proc._ab64, GRID, "encode")}
    figs = {"decode": _rel(dec, want["decode"]), "raw": _rel(raw, want["raw"]), "encode": _rel(enc, want["encode"])}
    print(f"planes {planes}: relative error against float64: decode {figs['decode']:.3e}, decode to t_min {figs['raw']:.3e}, encode {figs['encode']:.3e} (bound 1e-5)")
    assert all(v <= 1e-5 for v in figs.values()) and not torch.equal(dec, raw)
    with torch.no_grad():
        assert torch.equal(dec, proc._eager_walk(x_T.clone().cuda(), "decode"))
        assert torch.equal(raw, proc._eager_walk(x_T.clone().cuda(), "decode_raw"))
        assert torch.equal(enc, proc._eager_walk(x0.clone().cuda(), "encode", threshold=False))
    ords = dmme_amd.history_ordinals(proc.chain_length(), 4)
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    assert torch.equal(proc.decode(x_T.cuda(), history=rec), dec) and rec.recorded == 4 == len(ords) and proc.chain_length() == 9
    torch.manual_seed(5)
    g1 = proc.generate(SHAPE)
    torch.manual_seed(5)
    assert torch.equal(g1, proc.decode(dmme_amd.gaussian(SHAPE, device="cuda"))) and bool(torch.isfinite(g1).all())


def test_round_trip_beats_generalized_ddim():
    """encode then decode back to the data: Heun's error is smaller than GeneralizedDDIM's (the Euler method on the same ODE) on the same
    8-node linear grid over T = 100 - two measured values, no constant"""
    import dmme_amd

    net = _tiny()
    x0 = _image().cuda()
    gd = dmme_amd.GeneralizedDDIM(net, 100, 8, "linear", eta=0.0).cuda()
    pf = _flow(net, grid=None, nodes=8)
    assert pf._grid[0] == 1 and pf._grid[1:] == gd._tau_host[1:] and len(pf._grid) == 9
    euler = float((gd.decode(gd.encode(x0)) - x0).abs().max())
    heun = float((pf.decode(pf.encode(x0), final_denoise=False) - x0).abs().max())
    print(f"round trip over 8 nodes: max |x - x0| Heun {heun:.3e}, GeneralizedDDIM {euler:.3e}")
    assert heun < euler


def test_bf16_default_unet_smoke():
    """the default UNet in bf16 at batch 2, 3 nodes over T = 1000: the likelihood is finite, its latent is `encode`'s, and two calls under one
    seed agree bit for bit through one graph"""
    import dmme_amd

    net = dmme_amd.UNet(precision="bf16")
    net.load_state_dict(O.make_state_dict(O.UNetConfig(), 5))
    net.cuda().eval()
    shape = (2, 3, 32, 32)
    proc = dmme_amd.ProbabilityFlow(net, 1000, nodes=3).cuda()
    x0 = _image(42, shape).cuda()
    torch.manual_seed(1)
    a = proc.log_likelihood(x0)
    runner = proc._pf_runner_likelihood
    torch.manual_seed(1)
    b = proc.log_likelihood(x0)
    assert runner.capture_error is None and runner.graph is not None and proc._pf_runner_likelihood is runner
    assert all(bool(torch.isfinite(v).all()) for v in a) and all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(a.latent, proc.encode(x0))
    bpd = proc.bits_per_dim(x0)
    print(f"bf16 default UNet: log p {[round(float(v), 2) for v in a.log_p]}, bits/dim {[round(float(v), 4) for v in bpd]}")
    assert bool(torch.isfinite(bpd).all()) and bool(torch.isfinite(proc.generate(shape)).all())


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals():
    """the library's status and message, not a launch: a conditional plan, a classifier plan, a v-prediction plan, a thresholded plan, an
    fp16r32 plan, kind 14 handed to dmme_chain_step / dmme_chain_update, three output planes; x unchanged afterwards.  The process refuses
    the same before it builds a runner."""
    import dmme_amd

    L = _lib()
    lib = L.lib()
    net = _tiny()
    proc = _flow(net)
    x = synth.normal(1, SHAPE).cuda()
    runner = proc._flow_runner("likelihood", SHAPE, x.device, dmme_amd.LikelihoodChainRunner)
    runner.x.copy_(x)
    packed = runner._packed()
    runner.set(8, 1, 0)
    state_before = runner.state.clone()
    dev = x.device

    def step(plan):
        return lib.dmme_pf_ll_chain_step(plan.h, L.ptr(packed), L.ptr(runner.plan.packed_bwd), L.ptr(runner.x), L.ptr(runner.out), L.ptr(plan.workspace),
                                         L.ptr(runner.plan.bws), L.ptr(runner.xs), L.ptr(runner.es), L.ptr(runner.d_out), L.ptr(runner.dx), L.ptr(runner.scratch),
                                         L.ptr(runner.s), L.ptr(runner.acc), L.ptr(runner.coef), L.ptr(runner.ttab), L.ptr(runner.state), L.stream_ptr())

    tiny_kw = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    cnet = dmme_amd.ConditionalUNet(precision="fp32", num_classes=5, dropout=0.0, **tiny_kw).cuda().eval()
    assert step(cnet._plan_for(2, 32, 32, dev)) == -1 and b"class-conditional" in lib.dmme_last_error()
    cls = dmme_amd.EncoderClassifier(precision="fp32", num_classes=5, **tiny_kw).cuda().eval()
    assert step(cls._plan_for(2, 32, 32, dev)) == -1 and b"unconditional DMME_ARCH_DDPM or DMME_ARCH_IDDPM" in lib.dmme_last_error()
    mixed = dmme_amd.UNet(precision="fp16r32").cuda().eval()  # (the default network: the tiny one has no fp16r32 plan)
    assert step(mixed._plan_for(2, 32, 32, dev)) == -2 and b"fp16r32" in lib.dmme_last_error()
    plan = runner.plan
    ab = torch.linspace(1.0, 0.01, 101, device="cuda").repeat_interleave(2).contiguous()
    L.check(lib.dmme_unet_plan_set_prediction(plan.h, L.PRED_V, L.ptr(ab), 100))
    assert step(plan) == -2 and b"adapter" in lib.dmme_last_error()
    L.check(lib.dmme_unet_plan_set_prediction(plan.h, L.PRED_EPS, None, 100))
    tab = torch.ones(4 * 101, device="cuda")
    L.check(lib.dmme_unet_plan_set_threshold(plan.h, L.THRESHOLD_STATIC, L.ptr(tab), 100, 0, 0.0, None))
    assert step(plan) == -2 and b"clip" in lib.dmme_last_error()
    L.check(lib.dmme_unet_plan_set_threshold(plan.h, L.THRESHOLD_NONE, None, 100, 0, 0.0, None))
    assert lib.dmme_chain_step(plan.h, L.ptr(packed), L.ptr(runner.x), L.ptr(runner.out), L.ptr(plan.workspace), L.CHAIN_PFODE, L.ptr(runner.coef), L.ptr(runner.ttab),
                               L.ptr(runner.state), L.stream_ptr()) == -1 and b"chain_step: sampler kind 14" in lib.dmme_last_error()
    assert lib.dmme_chain_update(L.CHAIN_PFODE, L.ptr(runner.x), L.ptr(runner.out), L.ptr(runner.coef), L.ptr(runner.ttab), L.ptr(runner.state), 2, 3072,
                                 L.stream_ptr()) == -1 and b"14" in lib.dmme_last_error()
    assert lib.dmme_pf_chain_step(cnet._plan_for(2, 32, 32, dev).h, L.ptr(packed), L.ptr(runner.x), L.ptr(runner.out), L.ptr(plan.workspace), L.ptr(runner.xs),
                                  L.ptr(runner.es), L.ptr(runner.coef), L.ptr(runner.ttab), L.ptr(runner.state), L.stream_ptr()) == -1
    assert b"class-conditional" in lib.dmme_last_error()
    row = _row(proc._tables["likelihood"][1][8])
    assert lib.dmme_pf_stage(L.ptr(runner.x), L.ptr(runner.out), 3, L.ptr(runner.xs), L.ptr(runner.es), row, 2, 3072, L.stream_ptr()) == -1
    assert b"3 planes" in lib.dmme_last_error()
    assert lib.dmme_pf_probe(L.ptr(runner.d_out), 2, 3072, 0, 1, 0, L.stream_ptr()) == -1
    assert lib.dmme_pf_dot(L.ptr(runner.d_out), 1, L.ptr(runner.dx), row, 0, 3072, L.ptr(runner.scratch), L.ptr(runner.s), L.ptr(runner.acc), L.stream_ptr()) == -1
    assert lib.dmme_pf_prior(None, 2, 3072, L.ptr(runner.scratch), L.ptr(runner.acc), L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert torch.equal(runner.x, x) and torch.equal(runner.state, state_before) and bool((runner.acc == 0).all())  # nothing was launched
    for kw, msg in ((dict(prediction="v"), "adapter"), (dict(threshold="static"), "clip")):
        p = _flow(net, **kw)
        for call in (p.encode, p.log_likelihood):
            with pytest.raises(NotImplementedError, match=msg):
                call(x)
        assert bool(torch.isfinite(p.decode(x)).all())  # (the sampler goes through the common front: the adapter and the clip work there)
    with pytest.raises(RuntimeError, match="train mode"):
        _flow(_tiny().train()).log_likelihood(x)
    with pytest.raises(NotImplementedError, match="fp16r32"):
        _flow(mixed).log_likelihood(x)
