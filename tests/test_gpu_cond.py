"""Class-conditional UNet and classifier-free guidance on the MI355X against the CPU restatement (tests/cond_ref.py): forward in three
precisions, every gradient, label dropout against the Philox reference, the guided update kernels bit for bit, the captured chains,
what is refused, and one training step."""

import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from dmme_amd.optim import FusedAdam
from oracle import diffusion as D
from oracle import synth
from oracle import unet as O

from . import cond_ref as R
from . import philox_ref as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TINY_KW = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
SHAPE = (3, 32, 32)
# the bounds the unconditional net is held to against the same oracle blocks
FP32_TOL = {"tiny": 2e-5, "default": 2e-4}  # tests/test_gpu_guidance.py, relative to the reference's max
BF16_REL_RMS, BF16_MAX_REL = 1.0e-2, 1.7e-2  # tests/test_gpu_unet.py: BF16_BOUNDS["default"]
FP16_MAX_ABS, FP16_REL_RMS = 2.0e-3, 1.5e-3  # tests/test_gpu_fp16.py
CHAIN_ATOL = 1e-4  # tests/test_gpu_chain.py: its tiny fp32 chain against the reference's trajectory


def _net(cfg, K, seed, precision="fp32", sd=None):
    sd = R.make_state_dict(cfg, K, seed) if sd is None else sd
    net = dmme_amd.ConditionalUNet(precision=precision, num_classes=K, dropout=0.0, **(TINY_KW if cfg == R.TINY else {}))
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval(), sd


def _inputs(B, seed, tmax=1000):
    x = synth.normal(seed, (B,) + SHAPE)
    t = torch.from_numpy(np.random.RandomState(seed).randint(1, tmax, size=B)).to(torch.int64)
    return x, t


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def default_case():
    """the default net's weights, inputs and CPU references (per-image t and one t), computed once for the three precisions"""
    K = 10
    sd = R.make_state_dict(R.DEFAULT, K, 21)
    x, t = _inputs(4, 22)
    y = torch.tensor([3, 0, K, 3])
    with torch.no_grad():
        want_per = R.forward(sd, R.DEFAULT, x, t, y)
        want_one = R.forward(sd, R.DEFAULT, x, t[:1], y)
    return K, sd, x, t, y, want_per, want_one


# ------------------------------------------------------------------ forward
def test_forward_fp32_tiny():
    K = 10
    net, sd = _net(R.TINY, K, 11)
    x, t = _inputs(4, 12)
    y = torch.tensor([3, 0, K, 3])  # the null row and a repeated label
    tol = FP32_TOL["tiny"]
    with torch.no_grad():
        for tt in (t, t[:1]):  # t_len == B and t_len == 1
            want = R.forward(sd, R.TINY, x, tt, y)
            got = net(x.to(DEV), tt.to(DEV), y.to(DEV))
            err = _rel(got, want)
            print(f"tiny fp32, t_len {tt.numel()}: rel err {err:.3e}")
            assert err <= tol
        # another label on the same (x, t) moves the output: a kernel that ignores y fails this
        a = net(x.to(DEV), t.to(DEV), y.to(DEV))
        b = net(x.to(DEV), t.to(DEV), torch.tensor([5, 0, K, 3], device=DEV))
        assert _rel(b[0], a[0]) > 10 * tol and torch.equal(a[1:], b[1:])
        # a zero label table: the UNet on the shared 305 weights
        net.label_emb.weight.zero_()
        unet = dmme_amd.UNet(dropout=0.0, **TINY_KW)
        unet.load_state_dict({k: v for k, v in sd.items() if k != R.LABEL_KEY})
        unet = unet.to(DEV).eval()
        for tt in (t, t[:1]):
            assert _rel(net(x.to(DEV), tt.to(DEV), y.to(DEV)), unet(x.to(DEV), tt.to(DEV))) <= tol
    net.check_labels()


def test_forward_fp32_default(default_case):
    K, sd, x, t, y, want_per, want_one = default_case
    net, _ = _net(R.DEFAULT, K, 0, sd=sd)
    with torch.no_grad():
        for tt, want in ((t, want_per), (t[:1], want_one)):
            err = _rel(net(x.to(DEV), tt.to(DEV), y.to(DEV)), want)
            print(f"default fp32, t_len {tt.numel()}: rel err {err:.3e}")
            assert err <= FP32_TOL["default"]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_forward_16bit_default(default_case, precision):
    K, sd, x, t, y, want_per, want_one = default_case
    net, _ = _net(R.DEFAULT, K, 0, precision, sd=sd)
    with torch.no_grad():
        for tt, want in ((t, want_per), (t[:1], want_one)):
            got = net(x.to(DEV), tt.to(DEV), y.to(DEV)).cpu()
            err = (got - want).abs()
            mx, rms, wmax = float(err.max()), float(err.pow(2).mean().sqrt() / want.pow(2).mean().sqrt()), float(want.abs().max())
            print(f"default {precision}, t_len {tt.numel()}: max|err| {mx:.3e} rel-rms {rms:.3e} (|want|max {wmax:.3f})")
            if precision == "bf16":
                assert rms <= BF16_REL_RMS and mx / wmax <= BF16_MAX_REL
            else:
                assert mx <= FP16_MAX_ABS and rms <= FP16_REL_RMS


# ------------------------------------------------------------------ gradients
def test_gradients_vs_autograd():
    K, B, T = 3, 6, 1000
    net, sd = _net(R.TINY, K, 31)
    ref = {k: v.clone().requires_grad_(k != "condition.0.embeddings") for k, v in sd.items()}
    x, t = _inputs(B, 32, T)
    y = torch.tensor([2, 0, 2, 3, 0, 2])  # row 1 is absent, row 3 is the null label
    w = synth.normal(33, (B,) + SHAPE)  # dL/d(eps) of L = sum(w * eps)
    xr = x.clone().requires_grad_(True)
    (R.forward(ref, R.TINY, xr, t, y) * w).sum().backward()

    def backward():
        xg = x.to(DEV).requires_grad_(True)
        (net(xg, t.to(DEV), y.to(DEV)) * w.to(DEV)).sum().backward()
        return xg.grad

    dx = backward()
    bad = {}
    for name, p in net.named_parameters():
        want = ref[name].grad.numpy()
        err = np.abs(p.grad.cpu().numpy() - want).max()
        if err > 2e-6 + 1e-4 * np.abs(want).max():  # tests/test_gpu_train.py: its tiny fp32 gradients
            bad[name] = (float(err), float(np.abs(want).max()))
    assert not bad, f"{len(bad)} gradients off, e.g. {list(bad.items())[:6]}"
    assert float((dx.cpu() - xr.grad).abs().max()) <= 2e-6 + 1e-4 * float(xr.grad.abs().max())
    table = net.label_emb.weight.grad
    assert float(ref[R.LABEL_KEY].grad[1].abs().max()) == 0.0 and float(table[1].abs().max()) == 0.0
    assert float(table[0].abs().max()) > 0 and float(table[3].abs().max()) > 0
    # gradients accumulate, and a class absent from the batch leaves its row alone
    first = table.clone()
    with torch.no_grad():
        table[1].fill_(7.0)
    backward()
    assert torch.equal(table[1], torch.full_like(table[1], 7.0))
    np.testing.assert_allclose(table[[0, 2, 3]].cpu().numpy(), 2 * first[[0, 2, 3]].cpu().numpy(), rtol=1e-5, atol=1e-7)
    # two identical backward passes give the same bits
    got = []
    for _ in range(2):
        net.zero_grad(set_to_none=False)
        net.flat_grad().zero_()
        backward()
        got.append(net.label_emb.weight.grad.clone())
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], first)


def test_label_gradient_past_one_chunk_of_the_batch():
    """the row sum walks the batch in chunks of 256 match flags: B = 260 puts images of every class on both sides of the boundary"""
    K, B = 3, 260
    net, sd = _net(R.TINY, K, 39)
    ref = {k: v.clone().requires_grad_(k == R.LABEL_KEY) for k, v in sd.items()}
    x, t = _inputs(B, 40)
    y = torch.from_numpy(np.random.RandomState(41).randint(0, K + 1, size=B))
    y[256:] = torch.tensor([0, 1, 2, 3])
    w = synth.normal(42, (B,) + SHAPE)
    (R.forward(ref, R.TINY, x, t, y) * w).sum().backward()
    (net(x.to(DEV), t.to(DEV), y.to(DEV)) * w.to(DEV)).sum().backward()
    want = ref[R.LABEL_KEY].grad
    err = float((net.label_emb.weight.grad.cpu() - want).abs().max())
    print(f"label table gradient at B = {B}: max|err| {err:.3e} of {float(want.abs().max()):.3e}")
    assert err <= 2e-6 + 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("t_len", ["B", "1"])
def test_input_only_backward(t_len):
    """dmme_unet_backward_input_cond: dL/dx alone, after a per-image-t forward and after a one-t forward (B time rows behind the label op
    all the same); no parameter gradient is touched.  Tolerance: the tiny fp32 gradients of tests/test_gpu_train.py."""
    K, B = 3, 5
    net, sd = _net(R.TINY, K, 36)
    x, t = _inputs(B, 37)
    t = t if t_len == "B" else t[:1]
    y = torch.tensor([2, 0, K, 1, 2])
    w = synth.normal(38, (B,) + SHAPE)
    xr = x.clone().requires_grad_(True)
    (R.forward(sd, R.TINY, xr, t, y) * w).sum().backward()
    g = net.flat_grad()
    g.fill_(3.0)
    dx = net.input_grad(x.to(DEV), t.to(DEV), y, w.to(DEV))
    err = float((dx.cpu() - xr.grad).abs().max())
    print(f"input-only backward, t_len {t.numel()}: max|err| {err:.3e} of {float(xr.grad.abs().max()):.3e}")
    assert err <= 2e-6 + 1e-4 * float(xr.grad.abs().max())
    assert bool((g == 3.0).all())
    net.check_labels()


def test_backward_needs_one_timestep_per_image():
    net, _ = _net(R.TINY, 3, 34)
    x, t = _inputs(4, 35)
    out = net(x.to(DEV), t[:1].to(DEV), torch.tensor([0, 1, 2, 3], device=DEV))
    with pytest.raises(ValueError, match="one timestep per image"):
        out.sum().backward()


# ------------------------------------------------------------------ label dropout
def _dropout(y, K, p, seed, off):
    out = torch.empty_like(y)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().dmme_label_dropout(_lib.ptr(y), y.numel(), K, p, seed, off, _lib.ptr(out), _lib.ptr(status), _lib.stream_ptr()))
    return out.cpu(), int(status.item())


@pytest.mark.parametrize("B", [7, 1024])
def test_label_dropout_vs_philox_reference(B):
    K, p, seed, off = 10, 0.3, 0x1234567890ABCDEF, 977
    y = torch.from_numpy(np.random.RandomState(B).randint(0, K, size=B)).to(DEV)
    got, status = _dropout(y, K, p, seed, off)
    u = P.uniforms(seed, off, B)
    want = np.where(u < np.float32(p), K, y.cpu().numpy())
    assert status == 0 and np.array_equal(got.numpy(), want)
    assert B < 100 or 0.2 < float((got == K).float().mean()) < 0.4
    same, _ = _dropout(y, K, 0.0, seed, off)
    none, _ = _dropout(y, K, 1.0, seed, off)
    assert torch.equal(same, y.cpu()) and bool((none == K).all())


def test_label_dropout_flags_a_label_out_of_range():
    K = 10
    y = torch.tensor([1, K + 1, 2, K, 0], device=DEV)
    got, status = _dropout(y, K, 0.0, 5, 0)
    assert status == 1 and torch.equal(got, y.cpu())  # the status word and nothing else


# ------------------------------------------------------------------ the guided update kernels
def _tables(kind, eta, s):
    net = dmme_amd.ConditionalUNet(num_classes=3, **TINY_KW)
    proc = dmme_amd.ClassifierFreeDDPM(net, 8, guidance_scale=s) if kind == "ddpm" else dmme_amd.ClassifierFreeDDIM(net, 8, 4, eta=eta, guidance_scale=s)
    return proc._chain_kind, proc._chain_tables()


@pytest.mark.parametrize("chw", [3 * 32 * 32, 48])
@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_cfg_update_bit_exact(kind, eta, chw):
    from dmme_amd.diffusion_models.ddpm import ChainTables

    B, s = 2, 2.5
    code, (n, rows, ttab) = _tables(kind, eta, s)
    x = synth.normal(41, (B, chw))
    e = synth.normal(42, (2 * B, chw))
    z = synth.normal(43, (B, chw))
    lib = _lib.lib()
    tabs = ChainTables(rows, ttab, DEV)
    ed, zd = e.to(DEV), z.to(DEV)
    for i in (n, 1):  # a step that adds noise (where the kind has any) and the last one (DDPM: t == 1 adds none)
        row = rows[i]
        mixed = R.mix(e[:B], e[B:], s)
        want = R.ddpm_update(x, mixed, z, row, ttab[i] != 1) if kind == "ddpm" else R.gddim_update(x, mixed, z, row)
        # eager form: host scalars
        xe = torch.cat([x, x]).to(DEV)
        _lib.check(lib.dmme_cfg_step(code, _lib.ptr(xe), _lib.ptr(ed), _lib.ptr(zd), row[0], row[1], row[2], row[3], int(ttab[i] != 1), B, chw,
                                     _lib.stream_ptr()))
        assert torch.equal(xe[:B].cpu(), want) and torch.equal(xe[:B], xe[B:])
        # chain form: device state, injected normals
        xc = torch.cat([x, x]).to(DEV)
        tabs.set(i, 99, 1000)
        _lib.check(lib.dmme_chain_update_cfg(code, _lib.ptr(xc), _lib.ptr(ed), _lib.ptr(zd), _lib.ptr(tabs.coef), _lib.ptr(tabs.ttab),
                                             _lib.ptr(tabs.state), B, chw, _lib.stream_ptr()))
        assert torch.equal(xc[:B].cpu(), want) and torch.equal(xc[:B], xc[B:])
        st = tabs.state.cpu().tolist()
        assert st[0] == i - 1 and st[1] == ttab[i - 1] and st[2] == 1000 + B * chw // 4  # the offset advances as for batch B
        # chain form drawing its own normals: those of dmme_randn at the same span, indexed by the first half
        adds = ttab[i] != 1 if kind == "ddpm" else row[2] != 0.0
        if adds:
            xd = torch.cat([x, x]).to(DEV)
            tabs.set(i, 99, 1000)
            _lib.check(lib.dmme_chain_update_cfg(code, _lib.ptr(xd), _lib.ptr(ed), None, _lib.ptr(tabs.coef), _lib.ptr(tabs.ttab), _lib.ptr(tabs.state),
                                                 B, chw, _lib.stream_ptr()))
            zz = torch.empty((B, chw), device=DEV)
            _lib.check(lib.dmme_randn(_lib.ptr(zz), zz.numel(), 99, 1000, _lib.stream_ptr()))
            want_d = R.ddpm_update(x, mixed, zz.cpu(), row, True) if kind == "ddpm" else R.gddim_update(x, mixed, zz.cpu(), row)
            assert torch.equal(xd[:B].cpu(), want_d) and torch.equal(xd[:B], xd[B:])


# ------------------------------------------------------------------ chains
def _process(kind, net, s):
    if kind == "ddpm":
        return dmme_amd.ClassifierFreeDDPM(net, 8, guidance_scale=s).to(DEV)
    return dmme_amd.ClassifierFreeDDIM(net, 8, 4, eta=0.5, guidance_scale=s).to(DEV)


def _eager(proc, shape, y):
    n = proc.timesteps if isinstance(proc, dmme_amd.ClassifierFreeDDPM) else proc.sub_timesteps
    x = dmme_amd.gaussian(shape, device=DEV)
    for i in range(n, 0, -1):
        x = proc.sampling_step(x, torch.tensor([i], device=DEV), y)
    return x


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_chains(kind):
    K, B, s = 3, 3, 2.5
    net, sd = _net(R.TINY, K, 51)
    shape = (B,) + SHAPE
    y = torch.tensor([2, 0, 1])
    proc = _process(kind, net, s)
    n, rows, ttab = proc._chain_tables()
    # the captured graph against the eager loop: the same bits
    torch.manual_seed(7)
    got = proc.generate(shape, y)
    runner = proc._cfg_runner
    assert runner.capture_error is None and runner.graph is not None and runner.plan.B == 2 * B
    torch.manual_seed(7)
    assert torch.equal(got, _eager(proc, shape, y))
    # against the CPU chain on the same x_T and normals (the spans the chain draws, in order)
    torch.manual_seed(7)
    xT = dmme_amd.gaussian(shape, device=DEV).cpu()
    noises = [dmme_amd.gaussian(shape, device=DEV).cpu() for _ in range(n)]
    with torch.no_grad():
        want = R.cfg_chain(sd, R.TINY, xT, y, K, s, rows, ttab, noises, kind)
    err = float((got.cpu() - want).abs().max())
    print(f"{kind} chain vs CPU: max|err| {err:.3e}")
    assert err <= CHAIN_ATOL
    # other labels, another seed: the same graph
    graph = runner.graph
    torch.manual_seed(8)
    other = proc.generate(shape, torch.tensor([1, 1, K]))
    assert proc._cfg_runner is runner and runner.graph is graph and not torch.equal(other, got)
    # s == 1: batch B, the conditional-only chain
    one = _process(kind, net, 1.0)
    torch.manual_seed(9)
    a = one.generate(shape, y)
    assert one._cfg_runner.plan.B == B and one._cfg_runner.capture_error is None
    torch.manual_seed(9)
    assert torch.equal(a, _eager(one, shape, y))
    torch.manual_seed(9)
    xT = dmme_amd.gaussian(shape, device=DEV).cpu()
    noises = [dmme_amd.gaussian(shape, device=DEV).cpu() for _ in range(n)]
    with torch.no_grad():
        want = R.cfg_chain(sd, R.TINY, xT, y, K, 1.0, rows, ttab, noises, kind)
    assert float((a.cpu() - want).abs().max()) <= CHAIN_ATOL
    # s == 0: the chain with all-null labels
    zero, null = _process(kind, net, 0.0), torch.full((B,), K)
    torch.manual_seed(10)
    b0 = zero.generate(shape, y)
    torch.manual_seed(10)
    b1 = one.generate(shape, null)
    assert float((b0 - b1).abs().max()) <= CHAIN_ATOL


# ------------------------------------------------------------------ refusals
def test_refusals():
    K = 3
    net, _ = _net(R.TINY, K, 61)
    x, t = _inputs(2, 62)
    xd, td = x.to(DEV), t.to(DEV)
    plan = net._plan_for(2, 32, 32, DEV)
    packed = net._packed_for(plan)
    out = torch.empty_like(xd)
    lib = _lib.lib()
    # UNet-style entry points on a conditional plan
    for call in (lambda: dmme_amd.UNet.forward(net, xd, td), lambda: net.graphed_forward(xd, td)):
        with pytest.raises((_lib.DmmeError, ValueError)):
            call()
    rc = lib.dmme_unet_forward(plan.h, _lib.ptr(packed), _lib.ptr(xd), _lib.ptr(td), 2, _lib.ptr(out), _lib.ptr(plan.workspace), None, _lib.stream_ptr())
    assert rc == -1 and b"dmme_unet_forward_cond" in lib.dmme_last_error()
    # labels outside [0, K] on the Python side: before any launch
    gen = plan.fwd_gen
    for bad in ([0, K + 1], [-1, 0]):
        with pytest.raises(ValueError):
            net(xd, td, torch.tensor(bad))
        with pytest.raises(ValueError):
            dmme_amd.ClassifierFreeDDPM(net, 8, guidance_scale=2.0).to(DEV).generate((2,) + SHAPE, bad)
        with pytest.raises(ValueError):
            dmme_amd.ClassifierFreeDDPM(net, 8).to(DEV).training_step(xd, bad)
    assert plan.fwd_gen == gen
    # train mode
    net.train()
    with pytest.raises(RuntimeError):
        dmme_amd.ClassifierFreeDDPM(net, 8, guidance_scale=2.0).to(DEV).generate((2,) + SHAPE, [0, 1])
    net.eval()
    # the device-side status path: label K + 1 is clamped before it indexes the table (csrc/kernels_generic.hip: label_cond_kernel),
    # its image becomes NaN, the other image is untouched
    with torch.no_grad():
        good = net(xd, td, torch.tensor([1, 1], device=DEV))
        got = net(xd, td, torch.tensor([K + 1, 1], device=DEV), check_labels=False)
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], good[1])
    with pytest.raises(ValueError):
        net.check_labels()
    net.check_labels()  # the word is cleared


# ------------------------------------------------------------------ training step
def test_training_step_with_fused_adam():
    K, B, T = 3, 4, 100
    net, sd = _net(R.TINY, K, 71)
    proc = dmme_amd.ClassifierFreeDDPM(net, T, p_uncond=0.5).to(DEV)
    opt = FusedAdam(net.parameters(), lr=1e-3, max_grad_norm=1.0, ema_decay=0.9)
    ref = {k: v.clone().requires_grad_(k != "condition.0.embeddings") for k, v in sd.items()}
    params = [v for v in ref.values() if v.requires_grad]
    ropt = torch.optim.Adam(params, lr=1e-3)
    x0, t, z = synth.uniform(72, (B,) + SHAPE), synth.randint(73, 1, T, B), synth.normal(74, (B,) + SHAPE)
    y, drop = torch.tensor([2, 0, 1, 2]), torch.tensor([False, True, False, True])
    yd = torch.where(drop, torch.full_like(y, K), y)
    _, abar = D.alpha_tables(D.linear_beta(T))
    want = D.training_loss(lambda xt, tt: R.forward(ref, R.TINY, xt, tt, yd), x0, t, z, abar)
    want.backward()
    torch.nn.utils.clip_grad_norm_(params, 1.0)
    before = {k: v.detach().clone() for k, v in ref.items()}
    ropt.step()
    loss = proc.training_step(x0.to(DEV), y.to(DEV), t=t.to(DEV), noise=z.to(DEV), drop=drop)
    loss.backward()
    opt.step()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=2e-5)  # tests/test_gpu_train.py: its tiny training loop
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), ref[k].detach().numpy(), atol=3e-5, rtol=1e-4, err_msg=k)
    ema = opt.ema_parameters(net).cpu()
    for name, shape, off, isb in net._table:
        if not isb:
            n = int(np.prod(shape))
            np.testing.assert_allclose(ema[off : off + n].numpy().reshape(shape), (0.9 * before[name] + 0.1 * ref[name].detach()).numpy(), atol=3e-5, rtol=1e-4,
                                       err_msg=name)
    assert float((net.label_emb.weight.detach().cpu() - before[R.LABEL_KEY]).abs().max()) > 0
    net.check_labels()


def test_label_dropout_inside_the_training_step():
    """without an injected mask the labels are dropped on the device from torch's generator: the step is reproducible under a seed"""
    net, _ = _net(R.TINY, 3, 81)
    proc = dmme_amd.ClassifierFreeDDPM(net, 100, p_uncond=0.5).to(DEV)
    x0 = synth.uniform(82, (8,) + SHAPE).to(DEV)
    y = torch.arange(8, device=DEV) % 3
    losses = []
    for _ in range(2):
        torch.manual_seed(5)
        losses.append(float(proc.training_step(x0, y).detach()))
    assert losses[0] == losses[1] and np.isfinite(losses[0])
