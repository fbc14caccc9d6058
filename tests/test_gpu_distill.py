"""GPU: progressive distillation (csrc/distill.hip, diffusion_models/distill.py) - the three launches against their float32 numpy
restatement bit for bit (one quad, the ragged element path, several blocks, misaligned pointers), the noise launch against
dmme_q_sample's bits and its status word, the target against Algorithm 2 in float64 inside the derived bound, the mid launch against
GeneralizedDDIM's step, the training step with an analytic teacher, the tiny UNet as teacher and student (target by hand, frozen
teacher, halve's re-pack and re-fold), overfitting one batch, and the trainer's `distill` / `sample`."""

import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from oracle import unet as O

from . import distill_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SHAPE = (2, 3, 32, 32)
TINY_KW = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
T = 1000
STEPS = (1, 4, 256)
CHW = (4, 6, 3 * 32 * 32)  # one quad; the ragged element path; several blocks of quads
COMBOS = [(pred, clip) for pred in R.PREDICTIONS for clip in (False, True)]


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


@pytest.fixture(scope="module")
def sched():
    """the linear T = 1000 schedule as a process holds it, and the tables of every (N, prediction); computed once and left unchanged"""
    import dmme_amd

    p = dmme_amd.DDPM(torch.nn.Identity(), T)
    ab = p.alpha_bar.reshape(-1).double().numpy()
    out = {"ab": ab, "sa": p._sqrt_alpha_bar.numpy().copy(), "sd": p._sqrt_one_minus_alpha_bar.numpy().copy()}
    out["sa_dev"], out["sd_dev"] = _dev(out["sa"]), _dev(out["sd"])
    for N in STEPS:
        for pred in R.PREDICTIONS:
            rows64, tt = R.tables(ab, N, pred)
            got, got_tt = dmme_amd.distill_rows(ab, N, pred)
            assert np.array_equal(got, rows64, equal_nan=True) and np.array_equal(got_tt, tt)
            rows32 = rows64.astype(np.float32)
            out[(N, pred)] = {"rows64": rows64, "rows32": rows32, "tt": tt, "rows_dev": _dev(rows32.reshape(-1)), "tt_dev": _dev(tt.reshape(-1), torch.int64)}
    return out


_INPUTS = {}


def _inputs(B, chw):
    """(x0, z, out1, out2) float32 [B][chw]: images in [-1, 1], normals, and two network outputs wide enough that the clamp bites"""
    if (B, chw) not in _INPUTS:
        rng = np.random.default_rng(100 * B + chw)
        _INPUTS[(B, chw)] = (rng.uniform(-1, 1, (B, chw)).astype(np.float32), rng.standard_normal((B, chw)).astype(np.float32),
                             (1.5 * rng.standard_normal((B, chw))).astype(np.float32), (1.5 * rng.standard_normal((B, chw))).astype(np.float32))
    return _INPUTS[(B, chw)]


def _noise(x0, z, idx, tab, sched, N):
    from dmme_amd import _lib

    B, chw = x0.shape[0], x0[0].numel()
    z_t = torch.full_like(x0, 7.0)
    t, m = torch.full((B,), -5, dtype=torch.int64, device=DEV), torch.full((B,), -5, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _lib.lib().dmme_distill_noise(_lib.ptr(x0), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(tab["tt_dev"]), _lib.ptr(sched["sa_dev"]), _lib.ptr(sched["sd_dev"]), N, B, chw,
                                       _lib.ptr(z_t), _lib.ptr(t), _lib.ptr(m), _lib.ptr(status), _lib.stream_ptr())
    assert rc == 0, _lib.lib().dmme_last_error()
    return z_t, t, m, int(status.item())


def _mid(pred, clip, z_t, out1, idx, tab, N, z_m=None):
    from dmme_amd import _lib

    z_m = torch.full_like(z_t, 7.0) if z_m is None else z_m
    rc = _lib.lib().dmme_distill_mid(_lib.PREDICTIONS[pred], int(clip), _lib.ptr(z_t), _lib.ptr(out1), _lib.ptr(tab["rows_dev"]), _lib.ptr(idx), N, z_t.shape[0],
                                     z_t[0].numel(), _lib.ptr(z_m), _lib.stream_ptr())
    assert rc == 0, _lib.lib().dmme_last_error()
    return z_m


def _target(pred, clip, z_t, out1, z_m, out2, idx, tab, N, target=None):
    from dmme_amd import _lib

    target = torch.full_like(z_t, 7.0) if target is None else target
    rc = _lib.lib().dmme_distill_target(_lib.PREDICTIONS[pred], int(clip), _lib.ptr(z_t), _lib.ptr(out1), _lib.ptr(z_m), _lib.ptr(out2), _lib.ptr(tab["rows_dev"]),
                                        _lib.ptr(idx), N, z_t.shape[0], z_t[0].numel(), _lib.ptr(target), _lib.stream_ptr())
    assert rc == 0, _lib.lib().dmme_last_error()
    return target


# ------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("chw", CHW)
def test_noise_launch_matches_the_restatement_and_q_sample(sched, chw, B, N):
    from dmme_amd import _lib

    x0, z, _, _ = _inputs(B, chw)
    idx = np.asarray(_indices(B, N), dtype=np.int64)
    tab = sched[(N, "eps")]
    z_t, t, m, status = _noise(_dev(x0), _dev(z), _dev(idx, torch.int64), tab, sched, N)
    want, want_t, want_m, want_status = R.noise32(x0, z, idx, tab["tt"], sched["sa"], sched["sd"], N)
    assert _same(z_t, want) and status == want_status == 0
    assert np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(m.cpu().numpy(), want_m) and np.array_equal(want_t, tab["tt"][idx, 0])
    x_t, d_x0, d_z = torch.empty(B, chw, device=DEV), _dev(x0), _dev(z)
    _lib.check(_lib.lib().dmme_q_sample(_lib.ptr(d_x0), _lib.ptr(d_z), _lib.ptr(sched["sa_dev"]), _lib.ptr(sched["sd_dev"]), _lib.ptr(t), B, chw, _lib.ptr(x_t),
                                        _lib.ptr(None), _lib.stream_ptr()), "dmme_q_sample")
    assert _same(z_t, x_t.cpu().numpy())


@pytest.mark.parametrize("chw", CHW)
def test_noise_launch_flags_a_bad_index_and_never_reads_its_row(sched, chw):
    N = 4
    x0, z, _, _ = _inputs(3, chw)
    tab = sched[(N, "eps")]
    for bad in ([0, 2, 4], [1, 5, 3], [-7, 1 << 40, 2]):
        idx = np.asarray(bad, dtype=np.int64)
        z_t, t, m, status = _noise(_dev(x0), _dev(z), _dev(idx, torch.int64), tab, sched, N)
        want, want_t, want_m, want_status = R.noise32(x0, z, idx, tab["tt"], sched["sa"], sched["sd"], N)
        assert status == want_status == 1 and _same(z_t, want)
        assert np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(m.cpu().numpy(), want_m)
        ok = (idx >= 1) & (idx <= N)
        assert np.isnan(z_t.cpu().numpy()[~ok]).all() and np.isfinite(z_t.cpu().numpy()[ok]).all() and (want_t[~ok] == 0).all()


@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("chw", CHW)
def test_mid_and_target_launches_match_the_restatement(sched, chw, B, N):
    x0, z, o1, o2 = _inputs(B, chw)
    idx = np.asarray(_indices(B, N), dtype=np.int64)
    z_t = R.noise32(x0, z, idx, sched[(N, "eps")]["tt"], sched["sa"], sched["sd"], N)[0]
    d_idx, d_zt, d_o1, d_o2 = _dev(idx, torch.int64), _dev(z_t), _dev(o1), _dev(o2)
    for pred, clip in COMBOS:
        tab = sched[(N, pred)]
        want_m = R.mid32(clip, z_t, o1, tab["rows32"], idx, N)
        z_m = _mid(pred, clip, d_zt, d_o1, d_idx, tab, N)
        assert _same(z_m, want_m), (pred, clip)
        want = R.target32(clip, z_t, o1, want_m, o2, tab["rows32"], idx, N)
        got = _target(pred, clip, d_zt, d_o1, z_m, d_o2, d_idx, tab, N)
        assert _same(got, want) and np.isfinite(want).all(), (pred, clip)


def test_bad_indices_come_out_nan_in_mid_and_target(sched):
    N, B, chw = 4, 3, 8
    _, z_t, o1, o2 = _inputs(B, chw)
    idx = np.asarray([0, 5, 2], dtype=np.int64)
    tab = sched[(N, "v")]
    z_m = _mid("v", True, _dev(z_t), _dev(o1), _dev(idx, torch.int64), tab, N)
    want_m = R.mid32(True, z_t, o1, tab["rows32"], idx, N)
    got = _target("v", True, _dev(z_t), _dev(o1), z_m, _dev(o2), _dev(idx, torch.int64), tab, N)
    assert _same(z_m, want_m) and _same(got, R.target32(True, z_t, o1, want_m, o2, tab["rows32"], idx, N))
    assert np.isnan(got.cpu().numpy()[:2]).all() and np.isfinite(got.cpu().numpy()[2]).all()


def test_misaligned_pointers_take_the_element_path_with_the_same_bits(sched):
    """chw % 4 == 0 but the images start 4 bytes into their buffers: no 16-byte accesses, the same results"""
    N, B, chw = 4, 3, 8
    x0, z, o1, o2 = _inputs(B, chw)
    idx = np.asarray(_indices(B, N), dtype=np.int64)
    tab = sched[(N, "v")]

    def off(a):
        buf = torch.zeros(a.size + 1, device=DEV)
        buf[1:] = _dev(a).reshape(-1)
        view = buf[1:].view(a.shape)
        assert view.data_ptr() % 16 == 4
        return view

    d_idx = _dev(idx, torch.int64)
    z_t, t, m, status = _noise(off(x0), off(z), d_idx, tab, sched, N)
    want_zt = R.noise32(x0, z, idx, tab["tt"], sched["sa"], sched["sd"], N)[0]
    assert _same(z_t, want_zt) and status == 0
    z_m = _mid("v", True, off(want_zt), off(o1), d_idx, tab, N, off(np.zeros_like(o1)))
    want_m = R.mid32(True, want_zt, o1, tab["rows32"], idx, N)
    assert _same(z_m, want_m)
    got = _target("v", True, off(want_zt), off(o1), off(want_m), off(o2), d_idx, tab, N, off(np.zeros_like(o1)))
    assert _same(got, R.target32(True, want_zt, o1, want_m, o2, tab["rows32"], idx, N))


# ------------------------------------------------------------------------------------------ 2. the target against Algorithm 2 in float64
@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("pred,clip", COMBOS)
def test_target_is_algorithm_2_within_the_derived_bound(sched, N, pred, clip):
    """the device's z_m and target against the paper's Algorithm 2, literally and in float64 (the quotient form), on the same float32
    z_t, out1, out2, inside tests/distill_ref.bounds (the worst ratios of error to bound measured on an MI355X: DESIGN.md, progressive distillation)"""
    worst = [0.0, 0.0]
    for B, chw in ((3, 3 * 32 * 32), (3, 6), (1, 4)):
        x0, z, o1, o2 = _inputs(B, chw)
        idx = np.asarray(_indices(B, N), dtype=np.int64)
        tab = sched[(N, pred)]
        z_t = R.noise32(x0, z, idx, tab["tt"], sched["sa"], sched["sd"], N)[0]
        d_idx = _dev(idx, torch.int64)
        z_m = _mid(pred, clip, _dev(z_t), _dev(o1), d_idx, tab, N)
        got = _target(pred, clip, _dev(z_t), _dev(o1), z_m, _dev(o2), d_idx, tab, N).cpu().numpy().astype(np.float64)
        want = R.algorithm2(pred, clip, sched["ab"], N, idx, z_t, o1, o2, "quotient")
        b = R.bounds(clip, tab["rows64"], idx, z_t, o1, o2)
        worst[0] = max(worst[0], float((np.abs(z_m.cpu().numpy().astype(np.float64) - want["z_m"]) / b["z_m"]).max()))
        worst[1] = max(worst[1], float((np.abs(got - want["target"]) / b["target"]).max()))
    print(f"N = {N} {pred} clip {clip}: z_m at {worst[0]:.3f}, target at {worst[1]:.3f} of the bound")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


# ------------------------------------------------------------------------------------------ 3. the mid launch is GeneralizedDDIM's step
class _Stub(torch.nn.Module):
    """a network whose output is a given tensor (a fresh copy: the x0 / v adapter works in place on it)"""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x, t):
        return self.out.clone()


@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("pred", R.PREDICTIONS)
def test_mid_launch_is_the_step_of_generalized_ddim(sched, N, pred):
    """every image at one index i: z_m against GeneralizedDDIM(stub, T, 2N, "linear").sampling_step from loop index 2i - two float32
    evaluations of one float64 quantity, each inside its own bound of it"""
    import dmme_amd
    from dmme_amd.diffusion_models.ddpm import prediction_table

    B, C, H, W = 2, 3, 8, 8
    x0, z, o1, _ = _inputs(B, C * H * W)
    tab = sched[(N, pred)]
    stub = _Stub(_dev(o1).view(B, C, H, W))
    g = dmme_amd.GeneralizedDDIM(stub, T, 2 * N, "linear", eta=0.0, prediction=pred).to(DEV)
    ab, tau = sched["ab"], R.grid(T, N)
    ptab = prediction_table(ab, pred)
    worst = 0.0
    for i in sorted(set(_indices(3, N))):
        idx = np.full(B, i, dtype=np.int64)
        z_t = R.noise32(x0, z, idx, tab["tt"], sched["sa"], sched["sd"], N)[0]
        z_m = _mid(pred, False, _dev(z_t), _dev(o1), _dev(idx, torch.int64), tab, N).cpu().numpy().astype(np.float64)
        step = g.sampling_step(_dev(z_t).view(B, C, H, W), torch.tensor([2 * i], device=DEV)).reshape(B, -1).cpu().numpy().astype(np.float64)
        t, m = int(tau[2 * i]), int(tau[2 * i - 1])
        assert g._tau_host[2 * i] == t and g._tau_host[2 * i - 1] == m
        k0 = np.sqrt(ab[m] / ab[t])
        k1 = np.sqrt(1 - ab[m]) - k0 * np.sqrt(1 - ab[t])
        a, b = (1.0, 0.0) if pred == "eps" else (float(ptab[t, 0]), float(ptab[t, 1]))
        exact = R.algorithm2(pred, False, ab, N, idx, z_t, o1, o1)["z_m"]
        b_mid, b_step = R.bounds(False, tab["rows64"], idx, z_t, o1, o1)["z_m"], R.gddim_bound(k0, k1, a, b, z_t, o1)
        assert (np.abs(z_m - exact) <= b_mid).all() and (np.abs(step - exact) <= b_step).all(), i
        worst = max(worst, float((np.abs(z_m - step) / (b_mid + b_step)).max()))
    print(f"N = {N} {pred}: mid launch against GeneralizedDDIM's step at {worst:.3f} of the two bounds' sum")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------ 4. the training step, analytic teacher
K3 = 0.05


class _PolyTeacher(torch.nn.Module):
    """out = c(t) (z - K3 z^3), c(t) = 0.5 + 0.4 t / T: products and differences only, each one torch op, so its float32 evaluation has a
    forward bound one can write down (tests below)"""

    def __init__(self):
        super().__init__()
        self.register_buffer("c", (0.5 + 0.4 * torch.arange(T + 1, dtype=torch.float64) / T).to(torch.float32))
        self.calls = []

    def forward(self, z, t):
        assert not torch.is_grad_enabled() and not self.training
        self.calls.append(t.detach().cpu().numpy().copy())
        c = self.c[t].reshape(-1, 1, 1, 1)
        return c * (z - K3 * (z * z * z))


def _poly64(z, t):
    c = (0.5 + 0.4 * np.asarray(t, dtype=np.float64) / T).reshape((-1,) + (1,) * (z.ndim - 1))
    return c * (z - K3 * z ** 3), c


def _poly_bound(z, t, dz):
    """|fp32 teacher(z') - teacher(z)| for |z' - z| <= dz: the Lipschitz factor |c| |1 - 3 K3 z^2| on dz, and the evaluation's roundings -
    z^2, z^3, K3 z^3 (K3 and three products: 4 x 2^-24 |K3 z^3|), the difference (2^-24), c and its product (2 x 2^-24)"""
    out, c = _poly64(z, t)
    return np.abs(c) * np.abs(1 - 3 * K3 * z * z) * dz + R.EPS * np.abs(c) * (4 * np.abs(K3 * z ** 3) + 3 * np.abs(z - K3 * z ** 3))


class _AffineStudent(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = torch.nn.Parameter(torch.tensor(0.3)), torch.nn.Parameter(torch.tensor(-0.1))
        self.last = None

    def forward(self, z, t):
        out = self.a * z + self.b
        self.last = out.detach()
        return out


@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("pred,clip", COMBOS)
def test_training_step_with_an_analytic_teacher(sched, N, pred, clip):
    """injected indices and noise, any nn.Module as teacher and student: the loss against Algorithm 2's in float64 - the teacher in
    float64 at the exact z_m, the paper's quotient, the weighted MSE - inside the bound the target's bound implies"""
    import dmme_amd

    B = 3
    shape = (B, 3, 8, 8)
    x0, z, _, _ = _inputs(B, 3 * 8 * 8)
    idx = np.asarray(_indices(B, N), dtype=np.int64)
    teacher, student = _PolyTeacher(), _AffineStudent()
    p = dmme_amd.ProgressiveDistillation(student, teacher, T, N, prediction=pred, clip_x0=clip).to(DEV)
    assert teacher.c.device.type == "cuda" and p.loss_weight == "truncated-snr"
    loss = p.training_step(_dev(x0).view(shape), _dev(idx, torch.int64), _dev(z).view(shape))
    loss.backward()
    assert student.a.grad is not None and torch.isfinite(student.a.grad) and teacher.c.grad is None
    p.check_indices()
    tab = sched[(N, pred)]
    t, m = tab["tt"][idx, 0], tab["tt"][idx, 1]
    assert len(teacher.calls) == 2 and np.array_equal(teacher.calls[0], t) and np.array_equal(teacher.calls[1], m)
    z_t = R.noise32(x0, z, idx, tab["tt"], sched["sa"], sched["sd"], N)[0].reshape(shape)
    out1 = _poly64(z_t.astype(np.float64), t)[0]
    want = R.algorithm2(pred, clip, sched["ab"], N, idx, z_t, out1, lambda zm, mm: _poly64(zm, mm)[0], "quotient")
    # the device's teacher outputs: within the polynomial's evaluation bound of the float64 ones, the second also through z_m's own bound
    d_target = R.bounds(clip, tab["rows64"], idx, z_t, out1, _poly64(want["z_m"], m)[0], _poly_bound(z_t.astype(np.float64), t, 0.0),
                        lambda zm, b_zm: _poly_bound(zm, m, b_zm))["target"]
    w = dmme_amd.diffusion_models.ddpm.loss_weight_table(sched["ab"], pred, "truncated-snr")[t]
    out = student.last.cpu().numpy().astype(np.float64)
    exact = float((w.reshape(-1, 1, 1, 1) * (out - want["target"]) ** 2).mean())
    bound = R.loss_bound(w, out, want["target"], d_target)
    err = abs(float(loss.detach()) - exact)
    print(f"N = {N} {pred} clip {clip}: loss {float(loss.detach()):.6g}, float64 {exact:.6g}, error {err:.2e} at {err / bound:.3f} of the bound")
    assert err <= bound


def test_training_step_draws_its_own_indices_and_noise():
    import dmme_amd

    teacher, student = _PolyTeacher(), _AffineStudent()
    p = dmme_amd.ProgressiveDistillation(student, teacher, T, 4, prediction="x0").to(DEV)
    torch.manual_seed(3)
    x0 = torch.rand(64, 3, 8, 8, device=DEV) * 2 - 1
    z_t, t, target, idx = p.distill_target(x0)
    p.check_indices()
    i = idx.cpu().numpy()
    assert i.min() >= 1 and i.max() <= 4 and set(i) == {1, 2, 3, 4}
    tau = R.grid(T, 4)
    assert np.array_equal(t.cpu().numpy(), tau[2 * i]) and np.array_equal(teacher.calls[1], tau[2 * i - 1])
    assert torch.isfinite(target).all() and torch.isfinite(p.training_step(x0))
    with pytest.raises(ValueError, match="reached the device"):
        p.distill_target(x0[:2], torch.tensor([1, 9], device=DEV))
        p.check_indices()
    p.check_indices()  # (cleared by the raise)


# ------------------------------------------------------------------------------------------ 5. the tiny UNet as teacher and student
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


def test_unet_teacher_and_student(sched):
    """both networks the tiny UNet: the step's target is the one composed by hand from two teacher(z, t) calls and the restatement; an
    optimiser step moves the student and leaves the teacher's bits alone; halve() makes the teacher's next output the student's
    eval-mode output bit for bit - the teacher had packed and folded the old weights, so this is the re-pack and the re-fold"""
    import dmme_amd
    from dmme_amd.optim import FusedAdam

    N, pred = 4, "v"
    student, teacher = _tiny().train(), _tiny()
    p = dmme_amd.ProgressiveDistillation(student, teacher, T, N, prediction=pred, clip_x0=True).to(DEV)
    assert not teacher.training and student.training and all(not q.requires_grad for q in teacher.parameters())
    assert {id(q) for q in p.parameters()} == {id(q) for q in student.parameters()} and all(k.startswith("model.") for k in p.state_dict())
    x0, idx, noise = _fixed_batch(N)
    tab = sched[(N, pred)]
    i = idx.cpu().numpy()
    z_t, t, target, _ = p.distill_target(x0, idx, noise)
    want_zt, want_t, want_m, _ = R.noise32(x0.cpu().numpy(), noise.cpu().numpy(), i, tab["tt"], sched["sa"], sched["sd"], N)
    assert _same(z_t, want_zt) and np.array_equal(t.cpu().numpy(), want_t)
    with torch.no_grad():
        out1 = teacher(z_t, t).cpu().numpy()
        z_m = R.mid32(True, want_zt, out1, tab["rows32"], i, N)
        out2 = teacher(_dev(z_m), _dev(want_m, torch.int64)).cpu().numpy()
    assert _same(target, R.target32(True, want_zt, out1, z_m, out2, tab["rows32"], i, N))

    before_t, before_s = teacher.flat_parameters().clone(), student.flat_parameters().clone()
    opt = FusedAdam(p.parameters(), lr=1e-3)
    loss = p.training_step(x0, idx, noise)
    loss.backward()
    opt.step()
    opt.zero_grad()
    assert torch.isfinite(loss) and torch.equal(teacher.flat_parameters(), before_t) and not torch.equal(student.flat_parameters(), before_s)

    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(8)).to(DEV)
    tt = torch.tensor([700, 3], device=DEV)
    with torch.no_grad():
        old = teacher(x, tt).clone()
    p.halve()
    assert p.steps == 2 and not teacher.training and all(not q.requires_grad for q in teacher.parameters())
    assert torch.equal(teacher.flat_parameters(), student.flat_parameters())
    student.eval()
    with torch.no_grad():
        new, ref = teacher(x, tt).clone(), student(x, tt).clone()
    assert torch.equal(new, ref) and not torch.equal(new, old)
    rows, tt2 = R.tables(sched["ab"], 2, pred)
    assert _same(p._rows, rows.astype(np.float32)) and np.array_equal(p._tt.cpu().numpy().reshape(-1, 2), tt2)
    s = p.sampler()
    img = s.generate(SHAPE)
    assert s.sub_timesteps == 2 and s.model is student and tuple(img.shape) == SHAPE and torch.isfinite(img).all()


OVERFIT_STEPS, OVERFIT_LR = 40, 1e-3


def test_overfitting_one_batch_lowers_the_loss():
    """one fixed batch, fixed indices and noise, a few dozen Adam steps: the loss ends strictly below where it began (measured on an
    MI355X: see DESIGN.md, progressive distillation)"""
    import dmme_amd
    from dmme_amd.optim import FusedAdam

    N = 4
    student, teacher = _tiny().train(), _tiny()
    p = dmme_amd.ProgressiveDistillation(student, teacher, T, N, prediction="v").to(DEV)
    x0, idx, noise = _fixed_batch(N)
    opt = FusedAdam(p.parameters(), lr=OVERFIT_LR)
    losses = []
    for _ in range(OVERFIT_STEPS):
        loss = p.training_step(x0, idx, noise)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.detach())
    losses.append(p.training_step(x0, idx, noise).detach())
    first, last = float(losses[0]), float(losses[-1])
    print(f"overfitting: loss {first:.6g} -> {last:.6g} after {OVERFIT_STEPS} Adam steps at lr {OVERFIT_LR}: ratio {last / first:.4f}")
    assert np.isfinite(first) and np.isfinite(last) and last < first


# ------------------------------------------------------------------------------------------ 6. the trainer
TINY_YAML = """seed_everything: 7
trainer:
  gradient_clip_val: 1.0
  devices: 1
  max_steps: 2
  log_every_n_steps: 2
  precision: 32
model:
  class_path: dmme.LitDDPM
  init_args:
    lr: 1e-3
    warmup: 2
    decay: 0.99
    prediction: v
    loss_weight: truncated-snr
    model:
      class_path: dmme.UNet
      init_args:
        dropout: 0.0
        pos_dim: 4
        emb_dim: 8
        num_groups: 2
        channels_per_depth: [4, 8, 16, 32]
        num_blocks: 3
data:
  class_path: dmme.CIFAR10
  init_args:
    data_dir: .
    batch_size: 2
"""


def test_trainer_distills_two_stages_and_samples_the_student(tmp_path, capsys):
    from dmme_amd import trainer

    cfg, teacher, out, imgs = (str(tmp_path / n) for n in ("tiny.yaml", "teacher.ckpt", "student.ckpt", "imgs.npy"))
    with open(cfg, "w") as f:
        f.write(TINY_YAML)
    assert trainer.main(["fit", "--config", cfg, "--save-checkpoint", teacher]) == 0  # (--loss-weight truncated-snr by the YAML key)
    capsys.readouterr()
    assert trainer.main(["distill", "--config", cfg, "--ckpt-path", teacher, "--distill-from", "4", "--distill-to", "1", "--stage-steps", "3", "--clip-x0",
                         "--save-checkpoint", out]) == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith("{")]
    assert [(l["stage"], l["step"]) for l in lines] == [(2, 2), (2, 3), (1, 2), (1, 3)]
    assert all(np.isfinite(l["train/loss"]) and l["images_per_s"] > 0 for l in lines)
    ck = torch.load(out, map_location="cpu", weights_only=False)
    assert ck["distill"] == {"steps": 1, "tau_schedule": "linear", "prediction": "v"} and ck["global_step"] == 6
    assert all(k.startswith("diffusion_model.model.") for k in ck["state_dict"])
    t_sd = torch.load(teacher, map_location="cpu", weights_only=False)["state_dict"]
    assert set(t_sd) == set(ck["state_dict"]) and any(not torch.equal(t_sd[k], ck["state_dict"][k]) for k in t_sd)
    assert trainer.main(["sample", "--config", cfg, "--ckpt-path", out, "--num-images", "2", "--save", imgs]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["images"] == [2, 3, 32, 32] and line["finite"] is True and line["distill"] == {"steps": 1, "tau_schedule": "linear"}
    got = np.load(imgs)
    assert got.shape == (2, 3, 32, 32) and np.isfinite(got).all()
    # an explicit sampler wins over the checkpoint's
    assert trainer.main(["sample", "--config", cfg, "--ckpt-path", out, "--num-images", "2", "--sampler", "dpm++", "--sample-steps", "2"]) == 0
    assert "distill" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
