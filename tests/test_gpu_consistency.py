"""GPU: consistency distillation (csrc/consistency.hip, diffusion_models/consistency.py) - the target and loss launches against their
float32 numpy restatement bit for bit (one quad, the ragged element path, several blocks, several blocks and ragged, misaligned
pointers), the per-image sum inside the any-order bound, loss and gradient against float64 autograd of the literal Algorithm-2 loss
inside the derived bounds, bad indices, the moving average, the tiny UNet as student, teacher and target network, overfitting one batch,
the K-step sampler (captured chain against the eager loop, a step and a one-step sample against the literal update), and the trainer's
`consistency` / `sample`."""

import dataclasses
import json

import numpy as np
import pytest
import torch

from oracle import unet as O

from . import consistency_ref as R
from .test_gpu_distill import TINY_KW, TINY_YAML

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPE = (2, 3, 32, 32)
T = 1000
STEPS = (1, 4, 50)
CHW = (4, 6, 3 * 32 * 32, 3 * 32 * 32 + 2)  # one quad; the ragged element path; several blocks of quads; several blocks and ragged
COMBOS = [(pred, clip) for pred in R.PREDICTIONS for clip in (False, True)]
METRICS = (("pseudo-huber", R.PSEUDO_HUBER), ("l2", R.L2))


def _indices(B, N):
    """B = 1: the last index; B = 3: three indices that include 1 and N (as different as N allows)"""
    return [N] if B == 1 else [1, max(1, (2 * N) // 5 + 1 if N > 2 else N), N]


def _same(got, want):
    """the same bits, NaN standing for NaN"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    got, want = np.ascontiguousarray(got, dtype=np.float32).reshape(-1), np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _off(a):
    """the array on the device, starting 4 bytes into its buffer: no 16-byte accesses"""
    a = np.asarray(a, dtype=np.float32)
    buf = torch.zeros(a.size + 1, device=DEV)
    buf[1:] = _dev(a).reshape(-1)
    view = buf[1:].view(a.shape)
    assert view.data_ptr() % 16 == 4
    return view


def _huber_c(chw):
    return np.float32(R.HUBER_C * np.sqrt(float(chw)))


@pytest.fixture(scope="module")
def sched():
    """the linear T = 1000 schedule as a process holds it, and the tables of every (N, prediction); computed once and left unchanged"""
    import dmme_amd

    p = dmme_amd.DDPM(torch.nn.Identity(), T)
    ab = p.alpha_bar.reshape(-1).double().numpy()
    out = {"ab": ab, "sa": p._sqrt_alpha_bar.numpy().copy(), "sd": p._sqrt_one_minus_alpha_bar.numpy().copy()}
    for N in STEPS:
        for pred in R.PREDICTIONS:
            rows64, tt = R.tables(ab, N, pred)
            got, got_tt = dmme_amd.consistency_rows(ab, N, pred)
            assert np.array_equal(got, rows64, equal_nan=True) and np.array_equal(got_tt, tt)
            rows32 = rows64.astype(np.float32)
            out[(N, pred)] = {"rows64": rows64, "rows32": rows32, "tt": tt, "rows_dev": _dev(rows32.reshape(-1)), "tt_dev": _dev(tt.reshape(-1), torch.int64)}
    return out


_INPUTS = {}


def _inputs(B, chw):
    """(x0, z, out1, out_m, out) float32 [B][chw]: images in [-1, 1], normals, and three network outputs wide enough that the clamp bites"""
    if (B, chw) not in _INPUTS:
        rng = np.random.default_rng(1000 * B + chw)
        _INPUTS[(B, chw)] = (rng.uniform(-1, 1, (B, chw)).astype(np.float32), rng.standard_normal((B, chw)).astype(np.float32)) + tuple(
            (1.5 * rng.standard_normal((B, chw))).astype(np.float32) for _ in range(3))
    return _INPUTS[(B, chw)]


def _mid(pred, clip, z_t, out1, idx, tab, N):
    from dmme_amd import _lib

    z_m = torch.full_like(z_t, 7.0)
    rc = _lib.lib().dmme_distill_mid(_lib.PREDICTIONS[pred], int(clip), _lib.ptr(z_t), _lib.ptr(out1), _lib.ptr(tab["rows_dev"]), _lib.ptr(idx), N, z_t.shape[0],
                                     z_t[0].numel(), _lib.ptr(z_m), _lib.stream_ptr())
    assert rc == 0, _lib.lib().dmme_last_error()
    return z_m


def _cm_target(clip, z_m, out_m, idx, tab, N, f_target=None):
    from dmme_amd import _lib

    f_target = torch.full_like(z_m, 7.0) if f_target is None else f_target
    rc = _lib.lib().dmme_cm_target(int(clip), _lib.ptr(z_m), _lib.ptr(out_m), _lib.ptr(tab["rows_dev"]), _lib.ptr(idx), N, z_m.shape[0], z_m[0].numel(),
                                   _lib.ptr(f_target), _lib.stream_ptr())
    assert rc == 0, _lib.lib().dmme_last_error()
    return f_target


def _cm_loss(metric, z_t, out, f_target, idx, tab, N, c32, grad_scale=1.0, want_grad=True, d_out=None):
    """(loss float, sumsq float32 [B], d_out tensor or None)"""
    from dmme_amd import _lib

    B, chw = z_t.shape[0], z_t[0].numel()
    loss, sumsq = torch.full((1,), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    scratch = torch.full((65 * B,), 7.0, device=DEV)
    if want_grad and d_out is None:
        d_out = torch.full_like(z_t, 7.0)
    rc = _lib.lib().dmme_cm_loss(metric, _lib.ptr(z_t), _lib.ptr(out), _lib.ptr(f_target), _lib.ptr(tab["rows_dev"]), _lib.ptr(idx), N, B, chw, float(c32), _lib.ptr(loss),
                                 _lib.ptr(sumsq), _lib.ptr(d_out if want_grad else None), float(grad_scale), _lib.ptr(scratch), _lib.stream_ptr())
    assert rc == 0, _lib.lib().dmme_last_error()
    return float(loss.item()), sumsq.cpu().numpy(), (d_out if want_grad else None)


def _host_chain(sched, N, pred, clip, B, chw):
    """the float32 restatement of everything in front of the loss: idx, z_t, zh_m, f_target and the student's output"""
    x0, z, o1, o_m, out = _inputs(B, chw)
    idx = np.asarray(_indices(B, N), dtype=np.int64)
    tab = sched[(N, pred)]
    z_t = R.noise32(x0, z, idx, tab["tt"], sched["sa"], sched["sd"], N)[0]
    z_m = R.mid32(clip, z_t, o1, tab["rows32"], idx, N)
    ft = R.target32(clip, z_m, o_m, tab["rows32"], idx, N)
    return idx, tab, z_t, o1, z_m, o_m, ft, out


# ------------------------------------------------------------------------------------------ 1. the launches, bit for bit
@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("chw", CHW)
def test_target_launch_matches_the_restatement(sched, chw, B, N):
    for pred, clip in COMBOS:
        idx, tab, z_t, o1, z_m, o_m, want, _ = _host_chain(sched, N, pred, clip, B, chw)
        got = _cm_target(clip, _dev(z_m), _dev(o_m), _dev(idx, torch.int64), tab, N)
        assert _same(got, want) and np.isfinite(want).all(), (pred, clip)
        first = idx == 1  # m = 0: f(z, 0; .) = z in value
        assert np.array_equal(got.cpu().numpy()[first], z_m[first]), (pred, clip)
        if N > 1:
            assert not np.array_equal(got.cpu().numpy()[~first], z_m[~first])


def _check_loss(metric, tab, N, idx, z_t, out, ft, dev, c32, grad_scale):
    """the device's sumsq inside the any-order bound of the restatement's own squares; d_out bit for bit and the loss inside the any-order
    bound of the restatement evaluated from the device's sumsq; the same loss and sumsq without d_out"""
    B, chw = z_t.shape
    loss, sumsq, d_out = _cm_loss(metric, dev(z_t), dev(out), dev(ft), _dev(idx, torch.int64), tab, N, c32, grad_scale, d_out=dev(np.zeros_like(z_t)))
    S = R.squares32(z_t, out, ft, tab["rows32"], idx, N).astype(np.float64).sum(axis=1)
    assert np.isfinite(sumsq).all() and (np.abs(sumsq - S) <= (chw + 1) * R.EPS * S).all(), (sumsq, S)
    d32, g32 = R.finish(metric, sumsq, tab["rows32"], idx, N, chw, c32, np.float32(grad_scale))
    assert _same(d_out, R.d_out32(g32, z_t, out, ft, tab["rows32"], idx, N))
    mean = float(d32.astype(np.float64).mean())
    assert np.isfinite(loss) and abs(loss - mean) <= (B + 2) * R.EPS * mean, (loss, mean)
    loss2, sumsq2, none = _cm_loss(metric, dev(z_t), dev(out), dev(ft), _dev(idx, torch.int64), tab, N, c32, grad_scale, want_grad=False)
    assert none is None and loss2 == loss and _same(sumsq2, sumsq)
    return d_out


@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("chw", CHW)
def test_loss_launch_matches_the_restatement(sched, chw, B, N):
    for pred in R.PREDICTIONS:
        idx, tab, z_t, _, _, _, ft, out = _host_chain(sched, N, pred, True, B, chw)
        for _, metric in METRICS:
            a = _check_loss(metric, tab, N, idx, z_t, out, ft, _dev, _huber_c(chw), 1.0)
            b = _check_loss(metric, tab, N, idx, z_t, out, ft, _dev, _huber_c(chw), 3.0)
            assert not torch.equal(a, b)


def test_misaligned_pointers_take_the_element_path_with_the_same_bits(sched):
    """chw % 4 == 0 but every image pointer starts 4 bytes into its buffer: no 16-byte accesses, the same results"""
    N, B, chw = 4, 3, 8
    idx, tab, z_t, _, z_m, o_m, ft, out = _host_chain(sched, N, "v", True, B, chw)
    got = _cm_target(True, _off(z_m), _off(o_m), _dev(idx, torch.int64), tab, N, _off(np.zeros_like(ft)))
    assert _same(got, ft)
    for _, metric in METRICS:
        _check_loss(metric, tab, N, idx, z_t, out, ft, _off, _huber_c(chw), 2.0)


# ------------------------------------------------------------------------------------------ 2. loss and gradient against float64
@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("pred,clip", COMBOS)
def test_loss_and_gradient_are_algorithm_2_within_the_derived_bounds(sched, N, pred, clip):
    """the device's zh_m, f_target, S_b, loss and gradient against Algorithm 2's, literally and in float64 with torch autograd on the CPU,
    on the same float32 z_t and network outputs, inside tests/consistency_ref's bounds (the worst ratios of error to bound measured on an
    MI355X: DESIGN.md, consistency distillation)"""
    worst = {}
    for B, chw in ((3, 3 * 32 * 32 + 2), (3, 3 * 32 * 32), (3, 6), (1, 4)):
        idx, tab, z_t, o1, _, o_m, _, out = _host_chain(sched, N, pred, clip, B, chw)
        d_idx = _dev(idx, torch.int64)
        z_m = _mid(pred, clip, _dev(z_t), _dev(o1), d_idx, tab, N)
        ft = _cm_target(clip, z_m, _dev(o_m), d_idx, tab, N)
        want = R.algorithm2(pred, clip, sched["ab"], N, idx, z_t, o1, o_m)
        tb = R.target_bounds(clip, tab["rows64"], idx, z_t, o1, o_m)
        ratios = {"zh_m": float((np.abs(z_m.cpu().numpy().astype(np.float64) - want["z_m"]) / tb["z_m"]).max()),
                  "f_target": float((np.abs(ft.cpu().numpy().astype(np.float64) - want["f_target"]) / tb["f_target"]).max())}
        c32, gs = _huber_c(chw), 2.0
        for name, metric in METRICS:
            loss, sumsq, d_out = _cm_loss(metric, _dev(z_t), _dev(out), ft, d_idx, tab, N, c32, gs)
            loss64, grad64, S64, _ = R.loss64(pred, metric, sched["ab"], N, idx, z_t, out, want["f_target"], float(c32), grad_scale=gs)
            lb = R.loss_bounds(metric, tab["rows64"], idx, z_t, out, want["f_target"], tb["f_target"], float(c32), gs)
            ratios[f"S_b {name}"] = float((np.abs(sumsq - S64) / lb["sumsq"]).max())
            ratios[f"loss {name}"] = abs(loss - loss64) / lb["loss"]
            ratios[f"gradient {name}"] = float((np.abs(d_out.cpu().numpy().astype(np.float64) - grad64) / lb["grad"]).max())
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"N = {N} {pred} clip {clip}: " + ", ".join(f"{k} at {v:.3f}" for k, v in worst.items()) + " of the bound")
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------ 3. bad indices
@pytest.mark.parametrize("chw", (8, 6, 3 * 32 * 32))
def test_bad_indices_come_out_nan_and_never_read_their_rows(sched, chw):
    N, B = 4, 3
    _, z_t, _, o_m, out = _inputs(B, chw)
    tab = sched[(N, "v")]
    for bad in ([0, 5, 2], [3, -7, 1 << 40]):
        idx = np.asarray(bad, dtype=np.int64)
        ok = (idx >= 1) & (idx <= N)
        want = R.target32(True, z_t, o_m, tab["rows32"], idx, N)
        ft = _cm_target(True, _dev(z_t), _dev(o_m), _dev(idx, torch.int64), tab, N)
        assert _same(ft, want) and np.isnan(want[~ok]).all() and np.isfinite(want[ok]).all()
        clean = np.where(np.isnan(want), np.float32(0.25), want)  # (a finite target: the NaN below is the loss launch's own)
        for _, metric in METRICS:
            loss, sumsq, d_out = _cm_loss(metric, _dev(z_t), _dev(out), _dev(clean), _dev(idx, torch.int64), tab, N, _huber_c(chw))
            g = d_out.cpu().numpy()
            assert np.isnan(loss) and np.isnan(sumsq[~ok]).all() and np.isfinite(sumsq[ok]).all()
            assert np.isnan(g[~ok]).all() and np.isfinite(g[ok]).all()
            _, g32 = R.finish(metric, sumsq, tab["rows32"], idx, N, chw, _huber_c(chw), np.float32(1.0))
            assert _same(d_out, R.d_out32(g32, z_t, out, clean, tab["rows32"], idx, N))


# ------------------------------------------------------------------------------------------ 4. the moving average
@pytest.mark.parametrize("numel", (1, 5, 4096 + 3))
@pytest.mark.parametrize("decay", (0.0, 0.5, 0.95, 1.0))
def test_ema_lerp_matches_the_restatement(decay, numel):
    from dmme_amd import _lib

    rng = np.random.default_rng(numel)
    dst, src = rng.standard_normal(numel).astype(np.float32), rng.standard_normal(numel).astype(np.float32)
    want = R.ema32(dst, src, decay)
    for put in (_dev, _off):
        d, s = put(dst), put(src)
        rc = _lib.lib().dmme_ema_lerp(_lib.ptr(d), _lib.ptr(s), numel, decay, _lib.stream_ptr())
        assert rc == 0, _lib.lib().dmme_last_error()
        assert _same(d, want) and _same(s, src)
    if decay == 1.0:
        assert _same(want, dst)
    if decay == 0.0:
        assert _same(want, src)


# ------------------------------------------------------------------------------------------ 5. the tiny UNet as student, teacher and target
def _tiny(seed=11):
    import dmme_amd

    net = dmme_amd.UNet(dropout=0.0, **TINY_KW)
    net.load_state_dict(O.make_state_dict(dataclasses.replace(O.TINY, dropout=0.0), seed), strict=True)
    return net.to(DEV)


def _fixed_batch(N):
    g = torch.Generator().manual_seed(5)
    x0 = (torch.rand(SHAPE, generator=g) * 2 - 1).to(DEV)
    noise = torch.randn(SHAPE, generator=g).to(DEV)
    return x0, torch.tensor([1, N], device=DEV), noise


def _adam_step(p, opt, x0, idx, noise):
    loss = p.training_step(x0, idx, noise)
    loss.backward()
    opt.step()
    opt.zero_grad()
    p.after_step()
    return loss


def test_unet_student_is_its_own_target(sched):
    """target_decay = 0: f_target composed by hand from teacher(z_t, t), the restatement and the student's eval-mode no-grad output; an
    optimiser step moves the student and leaves the teacher's bits alone; afterwards the target's output is the moved student's eval-mode
    no-grad output bit for bit, and the student is back in train mode"""
    import dmme_amd
    from dmme_amd.optim import FusedAdam

    N, pred = 4, "v"
    student, teacher = _tiny(12).train(), _tiny()
    p = dmme_amd.ConsistencyDistillation(student, teacher, T, N, prediction=pred, clip_x0=True).to(DEV)
    assert p.target is None and not teacher.training and student.training and all(not q.requires_grad for q in teacher.parameters())
    assert {id(q) for q in p.parameters()} == {id(q) for q in student.parameters()} and all(k.startswith("model.") for k in p.state_dict())
    x0, idx, noise = _fixed_batch(N)
    tab = sched[(N, pred)]
    i = idx.cpu().numpy()
    z_t, t, f_target, _ = p.consistency_target(x0, idx, noise)
    assert student.training
    p.check_indices()
    want_zt, want_t, want_m, _ = R.noise32(x0.cpu().numpy(), noise.cpu().numpy(), i, tab["tt"], sched["sa"], sched["sd"], N)
    assert _same(z_t, want_zt) and np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(want_m, [1, 750])
    with torch.no_grad():
        out1 = teacher(z_t, t).cpu().numpy()
        z_m = R.mid32(True, want_zt, out1, tab["rows32"], i, N)
        student.eval()
        out_m = student(_dev(z_m), _dev(want_m, torch.int64)).cpu().numpy()
        student.train()
    assert _same(f_target, R.target32(True, z_m, out_m, tab["rows32"], i, N))

    before_t, before_s = teacher.flat_parameters().clone(), student.flat_parameters().clone()
    opt = FusedAdam(p.parameters(), lr=1e-3)
    loss = _adam_step(p, opt, x0, idx, noise)
    assert torch.isfinite(loss) and torch.equal(teacher.flat_parameters(), before_t) and not torch.equal(student.flat_parameters(), before_s)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(8)).to(DEV)
    tt = torch.tensor([700, 3], device=DEV)
    got = p._target_out(x, tt).clone()
    assert student.training
    student.eval()
    with torch.no_grad():
        ref = student(x, tt).clone()
    student.train()
    assert torch.equal(got, ref)
    with pytest.raises(ValueError, match="reached the device"):
        p.consistency_target(x0, torch.tensor([1, 9], device=DEV), noise)
        p.check_indices()
    p.check_indices()  # (cleared by the raise)


def test_unet_target_network_follows_the_student():
    """target_decay = 0.5: the target starts as the student; after an optimiser step and after_step() its flat buffer is the restatement's
    moving average bit for bit, its next forward differs from the previous one (the re-pack and the re-fold), and the teacher's bits and
    the target's frozen state are untouched"""
    import dmme_amd
    from dmme_amd.optim import FusedAdam

    N = 4
    student, teacher = _tiny(12).train(), _tiny()
    p = dmme_amd.ConsistencyDistillation(student, teacher, T, N, prediction="v", target_decay=0.5).to(DEV)
    target = p.target
    assert target is not student and target.flat_parameters().is_cuda and torch.equal(target.flat_parameters(), student.flat_parameters())
    assert not target.training and all(not q.requires_grad for q in target.parameters())
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(8)).to(DEV)
    tt = torch.tensor([700, 3], device=DEV)
    with torch.no_grad():
        old = target(x, tt).clone()
    x0, idx, noise = _fixed_batch(N)
    before_teacher, before_target = teacher.flat_parameters().clone(), target.flat_parameters().cpu().numpy().copy()
    opt = FusedAdam(p.parameters(), lr=1e-3)
    loss = _adam_step(p, opt, x0, idx, noise)
    assert torch.isfinite(loss) and torch.equal(teacher.flat_parameters(), before_teacher)
    want = R.ema32(before_target, student.flat_parameters().cpu().numpy(), 0.5)
    assert _same(target.flat_parameters(), want) and not np.array_equal(want, before_target)
    with torch.no_grad():
        new = target(x, tt).clone()
    assert torch.isfinite(new).all() and not torch.equal(new, old)
    assert not target.training and all(not q.requires_grad for q in target.parameters())
    # decay 1 never moves it
    q = dmme_amd.ConsistencyDistillation(_tiny(12).train(), teacher, T, N, prediction="v", target_decay=1.0).to(DEV)
    frozen = q.target.flat_parameters().clone()
    _adam_step(q, FusedAdam(q.parameters(), lr=1e-3), x0, idx, noise)
    assert torch.equal(q.target.flat_parameters(), frozen) and not torch.equal(q.model.flat_parameters(), frozen)


OVERFIT_STEPS, OVERFIT_LR = 40, 1e-3


def test_overfitting_one_batch_lowers_the_loss():
    """one fixed batch, fixed indices and noise, a target network that never moves, a few dozen Adam steps: the loss ends strictly below
    where it began (measured on an MI355X: see DESIGN.md, consistency distillation)"""
    import dmme_amd
    from dmme_amd.optim import FusedAdam

    N = 4
    student, teacher = _tiny(12).train(), _tiny()
    p = dmme_amd.ConsistencyDistillation(student, teacher, T, N, prediction="v", target_decay=1.0).to(DEV)
    x0, idx, noise = _fixed_batch(N)
    opt = FusedAdam(p.parameters(), lr=OVERFIT_LR)
    losses = [_adam_step(p, opt, x0, idx, noise).detach() for _ in range(OVERFIT_STEPS)]
    losses.append(p.training_step(x0, idx, noise).detach())
    first, last = float(losses[0]), float(losses[-1])
    print(f"overfitting: loss {first:.6g} -> {last:.6g} after {OVERFIT_STEPS} Adam steps at lr {OVERFIT_LR}: ratio {last / first:.4f}")
    assert np.isfinite(first) and np.isfinite(last) and last < first


# ------------------------------------------------------------------------------------------ 6. the sampler
def _gen_state():
    g = torch.cuda.default_generators[DEV.index]
    return int(g.initial_seed()), int(g.get_offset())


@pytest.mark.parametrize("K", (1, 2))
def test_sampler_chain_equals_the_eager_loop_and_the_literal_update(sched, K):
    """`generate` through the captured step against the eager host loop under one seed: bit-identical; one eager step with the noise
    injected, and the one-step sample, against x' = alpha_p f(x, a) + sigma_p z in float64 from the network's raw output, inside
    tests/consistency_ref.sample_step_bound"""
    import dmme_amd
    from dmme_amd.diffusion_models.ddpm import prediction_table

    N, pred = 4, "v"
    net = _tiny(12).eval()
    s = dmme_amd.ConsistencySampler(net, T, K, N, prediction=pred).to(DEV)
    torch.manual_seed(77)
    got = s.generate(SHAPE).clone()
    assert s._runner is not None and (s._runner.graph is not None or getattr(net, "_graph_disabled", False))
    torch.manual_seed(77)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    x_T = x.clone()
    with torch.no_grad():
        for i in range(K, 0, -1):
            s._ddim_update(x, s._eps(x, s.tau_tensor(i, x.device)), i)
    assert torch.equal(got, x) and bool(torch.isfinite(got).all())

    rows64, ptab, tau = R.sampler_rows(sched["ab"], K), prediction_table(sched["ab"], pred), R.grid(T, K)
    z = torch.randn(SHAPE, generator=torch.Generator().manual_seed(3)).to(DEV)
    worst = 0.0
    for i in range(K, 0, -1):
        a, b = float(ptab[tau[i], 0]), float(ptab[tau[i], 1])
        with torch.no_grad():
            out = net(x_T, s.tau_tensor(i, DEV)).clone()
            step = s.sampling_step(x_T, torch.tensor([i], device=DEV), noise=z)
        xs, outs, zs = (v.cpu().numpy().astype(np.float64) for v in (x_T, out, z))
        want = R.sample_step64(pred, sched["ab"], K, i, xs, outs, zs)
        bound = R.sample_step_bound(rows64[i], a, b, xs, outs, zs)
        worst = max(worst, float((np.abs(step.cpu().numpy().astype(np.float64) - want) / bound).max()))
        if K == 1:  # generate = alpha_0 f(x_T, T) = f(x_T, T)
            worst = max(worst, float((np.abs(got.cpu().numpy().astype(np.float64) - want) / bound).max()))
    print(f"K = {K}: the sampler's step against the literal update at {worst:.3f} of the bound")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------ 7. the trainer
def test_trainer_distills_and_samples_in_one_and_two_steps(tmp_path, capsys):
    from dmme_amd import trainer

    cfg, teacher, out, imgs = (str(tmp_path / n) for n in ("tiny.yaml", "teacher.ckpt", "student.ckpt", "imgs.npy"))
    with open(cfg, "w") as f:
        f.write(TINY_YAML)
    assert trainer.main(["fit", "--config", cfg, "--save-checkpoint", teacher]) == 0
    capsys.readouterr()
    assert trainer.main(["consistency", "--config", cfg, "--ckpt-path", teacher, "--consistency-steps", "4", "--max-steps", "3", "--target-decay", "0.95", "--clip-x0",
                         "--save-checkpoint", out]) == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [2, 3] and all(np.isfinite(l["train/loss"]) and l["images_per_s"] > 0 for l in lines)
    ck = torch.load(out, map_location="cpu", weights_only=False)
    assert ck["consistency"] == {"steps": 4, "prediction": "v", "sigma_data": 0.5, "timestep_scaling": 10.0} and ck["global_step"] == 3 and "distill" not in ck
    assert all(k.startswith("diffusion_model.model.") for k in ck["state_dict"])
    t_sd = torch.load(teacher, map_location="cpu", weights_only=False)["state_dict"]
    assert set(t_sd) == set(ck["state_dict"]) and any(not torch.equal(t_sd[k], ck["state_dict"][k]) for k in t_sd)
    for extra, K in (([], 1), (["--sample-steps", "2"], 2)):
        assert trainer.main(["sample", "--config", cfg, "--ckpt-path", out, "--num-images", "2", "--save", imgs] + extra) == 0
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["images"] == [2, 3, 32, 32] and line["finite"] is True and line["consistency"] == {"steps": 4, "sample_steps": K}
        got = np.load(imgs)
        assert got.shape == (2, 3, 32, 32) and np.isfinite(got).all()
    with pytest.raises(SystemExit, match="does not divide"):
        trainer.main(["sample", "--config", cfg, "--ckpt-path", out, "--num-images", "2", "--sample-steps", "3"])
    # an explicit sampler wins over the checkpoint's
    assert trainer.main(["sample", "--config", cfg, "--ckpt-path", out, "--num-images", "2", "--sampler", "dpm++", "--sample-steps", "2"]) == 0
    assert "consistency" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
