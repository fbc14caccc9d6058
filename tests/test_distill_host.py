"""CPU: progressive distillation's host side - the nested grids and their refusals, the tables against their definitions and against
GeneralizedDDIM's step algebra, the convex form against the paper's quotient in float64 (and what the quotient loses in float32), the
truncated-SNR weights, the restatement's bounds on the restatement itself, the ABI, LinearDecayLR, the checkpoint entry and the
trainer's refusals.  No GPU."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from dmme_amd.diffusion_models.ddpm import loss_weight_table
from dmme_amd.equations.ddim import linear_tau

from . import distill_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
STEPS = (500, 256, 128, 64, 8, 4, 2, 1)
AB = R.alpha_bar(T)


class _Net(torch.nn.Module):
    """a network with parameters that is no UNet: `out = a x`"""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(0.5))

    def forward(self, x, t):
        return self.a * x


# ------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("N", STEPS)
def test_grids_nest_and_their_points_are_distinct(N):
    tau = dmme_amd.distill_grid(T, N)
    assert np.array_equal(tau, linear_tau(T, 2 * N).numpy()) and np.array_equal(tau, R.grid(T, N))
    assert np.array_equal(linear_tau(T, N).numpy(), tau[::2])
    assert tau[0] == 0 and tau[-1] == T and (np.diff(tau) > 0).all() and tau[1] >= 1
    g = dmme_amd.GeneralizedDDIM(torch.nn.Identity(), T, N, "linear")
    assert g._tau_host == [int(v) for v in tau[::2]]


def test_refusals_of_the_grid_and_of_halve():
    with pytest.raises(ValueError, match="do not fit"):
        dmme_amd.distill_grid(T, 501)
    with pytest.raises(ValueError, match="at least 1"):
        dmme_amd.distill_grid(T, 0)
    with pytest.raises(ValueError, match="do not fit"):
        dmme_amd.ProgressiveDistillation(_Net(), _Net(), 10, 6, prediction="x0")
    with pytest.raises(ValueError, match="prediction"):
        dmme_amd.distill_rows(AB, 4, "score")
    p = dmme_amd.ProgressiveDistillation(_Net(), _Net(), T, 3, prediction="x0")
    with pytest.raises(ValueError, match="odd"):
        p.halve()
    assert p.steps == 3
    net = _Net()
    with pytest.raises(ValueError, match="two networks"):
        dmme_amd.ProgressiveDistillation(net, net, T, 4, prediction="x0")


def test_networks_with_labels_or_two_planes_are_refused():
    tiny = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=1)
    from dmme_amd.models.iddpm import UNet as IDDPMUNet

    plain = dmme_amd.UNet(**tiny)
    for bad in (dmme_amd.ConditionalUNet(num_classes=3, **tiny), IDDPMUNet(**tiny)):
        with pytest.raises(NotImplementedError, match="out of scope"):
            dmme_amd.ProgressiveDistillation(plain, bad, T, 4, prediction="v")
        with pytest.raises(NotImplementedError, match="out of scope"):
            dmme_amd.ProgressiveDistillation(bad, plain, T, 4, prediction="v")


# ------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("pred", R.PREDICTIONS)
@pytest.mark.parametrize("N", (256, 64, 4, 1))
def test_tables(N, pred):
    rows, tt = dmme_amd.distill_rows(AB, N, pred)
    want, want_tt = R.tables(AB, N, pred)
    assert rows.shape == (N + 1, 12) and rows.dtype == np.float64 and tt.shape == (N + 1, 2) and tt.dtype == np.int64
    assert np.array_equal(rows, want, equal_nan=True) and np.array_equal(tt, want_tt)
    assert np.isnan(rows[0]).all() and np.isfinite(rows[1:]).all() and (rows[1:, 10:] == 0).all()
    tau = R.grid(T, N)
    assert np.array_equal(tt[1:, 0], tau[2::2]) and np.array_equal(tt[1:, 1], tau[1::2]) and (tt[1:, 1] >= 1).all()
    w1, w2 = rows[1:, R.W1], rows[1:, R.W2]
    assert (w1[0], w2[0]) == (0.0, 1.0)
    assert (w1[1:] > 0).all() and (w2 > 0).all() and np.abs(w1 + w2 - 1).max() <= 4e-16
    # the student's parameterisation inverts the x0 pair at t: q0 (p0 o + p1 z) + q1 z = o
    p0, p1, q0, q1 = (rows[1:, k] for k in (R.P0, R.P1, R.Q0, R.Q1))
    assert np.abs(q0 * p0 - 1).max() <= 1e-12 and np.abs(q0 * p1 + q1).max() <= 1e-9 * np.abs(q1).max()


@pytest.mark.parametrize("N", (256, 64, 4, 1))
def test_the_mid_step_is_generalized_ddims_step(N):
    """z_m = m0 x1 + m1 z_t with x1 = (z_t - sigma_t e) / alpha_t is x' = k0 z_t + k1 e of GeneralizedDDIM(T, 2N, "linear") from index 2i,
    in float64: k0 = m0 / alpha_t + m1, k1 = -m0 sigma_t / alpha_t"""
    rows, _ = dmme_amd.distill_rows(AB, N, "eps")
    tau = R.grid(T, N)
    for i in range(1, N + 1):
        a, p = AB[tau[2 * i]], AB[tau[2 * i - 1]]
        k0 = np.sqrt(p / a)
        k1 = np.sqrt(1 - p) - k0 * np.sqrt(1 - a)
        m0, m1 = rows[i, R.M0], rows[i, R.M1]
        assert abs(m0 * rows[i, R.P1] + m1 - k0) <= 1e-13 * k0 and abs(m0 * rows[i, R.P0] - k1) <= 1e-13 * max(abs(k1), 1.0), i
    g = dmme_amd.GeneralizedDDIM(torch.nn.Identity(), T, 2 * N, "linear")
    i = N
    assert g._tau_host[2 * i] == tau[2 * i] and g._rev_rows[2 * i][0] == float(np.float32(np.sqrt(AB[tau[2 * i - 1]] / AB[tau[2 * i]])))


# ------------------------------------------------------------------------------------------ the convex form and the quotient
def _inputs(N, seed):
    rng = np.random.default_rng(seed)
    idx = np.arange(1, N + 1)
    shape = (N, 6)
    return idx, rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)


@pytest.mark.parametrize("pred", R.PREDICTIONS)
@pytest.mark.parametrize("N", (256, 64, 4, 1))
def test_convex_form_is_the_papers_quotient_in_float64(N, pred):
    idx, z_t, o1, o2 = _inputs(N, 3)
    for clip in (False, True):
        a = R.algorithm2(pred, clip, AB, N, idx, z_t, o1, o2, "quotient")
        b = R.algorithm2(pred, clip, AB, N, idx, z_t, o1, o2, "convex")
        scale = np.maximum(1.0, np.abs(a["x_tilde"]))
        err = float((np.abs(a["x_tilde"] - b["x_tilde"]) / scale).max())
        print(f"N = {N} {pred} clip {clip}: convex form against the quotient in float64: {err:.2e}")
        assert err <= 1e-10


def test_the_quotient_loses_in_float32_what_the_convex_form_keeps():
    """why the device never forms z_e: on x0 estimates in [-1, 1] the float32 quotient is off by 1e-4 and more somewhere along the grid,
    the float32 convex combination by a few 2^-24"""
    N = 256
    idx, z_t, _, _ = _inputs(N, 5)
    rng = np.random.default_rng(6)
    x1, x2 = rng.uniform(-1, 1, z_t.shape), rng.uniform(-1, 1, z_t.shape)
    exact = R.algorithm2("x0", False, AB, N, idx, z_t, x1, x2, "convex")["x_tilde"]
    rows, _ = R.tables(AB, N, "x0")
    w = rows[idx].astype(np.float32)
    convex = R._axpby32(w[:, R.W1:R.W1 + 1], w[:, R.W2:R.W2 + 1], x1.astype(np.float32), x2.astype(np.float32))
    e_convex = float(np.abs(convex - exact).max())
    e_quot = float(np.abs(R.quotient32(AB, N, idx, z_t, x1, x2) - exact).max())
    print(f"float32 at T = {T}, N = {N}: quotient {e_quot:.2e}, convex form {e_convex:.2e}")
    assert e_convex <= 4 * R.EPS and e_quot >= 1e-4


@pytest.mark.parametrize("pred", R.PREDICTIONS)
@pytest.mark.parametrize("clip", (False, True))
def test_the_bounds_hold_for_the_restatement_in_fp32(pred, clip):
    """tests/distill_ref.py in float32 against Algorithm 2 in float64 must sit inside its own bounds before the device is asked to"""
    N = 256
    idx, z_t, o1, o2 = (v.astype(np.float32) if v.dtype != np.int64 else v for v in _inputs(N, 9))
    rows64, _ = R.tables(AB, N, pred)
    rows32 = rows64.astype(np.float32)
    z_m = R.mid32(clip, z_t, o1, rows32, idx, N)
    got = R.target32(clip, z_t, o1, z_m, o2, rows32, idx, N)
    want = R.algorithm2(pred, clip, AB, N, idx, z_t, o1, o2)
    b = R.bounds(clip, rows64, idx, z_t, o1, o2)
    r_mid = float((np.abs(z_m - want["z_m"]) / b["z_m"]).max())
    r_tgt = float((np.abs(got - want["target"]) / b["target"]).max())
    print(f"{pred} clip {clip}: the restatement in fp32 at {r_mid:.3f} (z_m) and {r_tgt:.3f} (target) of the bounds")
    assert r_mid <= 1.0 and r_tgt <= 1.0


# ------------------------------------------------------------------------------------------ the loss weights
@pytest.mark.parametrize("pred", R.PREDICTIONS)
def test_truncated_snr_weights(pred):
    w = loss_weight_table(AB, pred, "truncated-snr")
    snr = AB[1:] / (1 - AB[1:])
    on_x0 = np.maximum(snr, 1.0)
    want = {"eps": on_x0 / snr, "x0": on_x0, "v": on_x0 / (snr + 1)}[pred]
    assert w.shape == (T + 1,) and np.allclose(w[1:], want, rtol=1e-15, atol=0)
    assert np.isnan(w[0]) if pred == "x0" else w[0] == 1.0
    # the weight each loss implies on the x0 error is max(snr, 1): eps error = (alpha / sigma) x0 error, v error = x0 error / sigma
    factor = {"eps": snr, "x0": np.ones_like(snr), "v": 1.0 / (1 - AB[1:])}[pred]
    assert np.allclose(w[1:] * factor, on_x0, rtol=1e-12)
    p = dmme_amd.DDPM(torch.nn.Identity(), T, prediction=pred, loss_weight="truncated-snr")
    assert np.array_equal(p._loss_w.numpy(), w.astype(np.float32), equal_nan=True)
    # existing values keep their bits
    from . import pred_ref

    assert np.array_equal(loss_weight_table(AB, pred, "min-snr", 5.0), pred_ref.weight_table(AB, pred, 5.0)) and (loss_weight_table(AB, pred, "uniform") == 1.0).all()
    with pytest.raises(ValueError, match="loss_weight"):
        loss_weight_table(AB, pred, "max-snr")


# ------------------------------------------------------------------------------------------ the header, the binding, the C argument checks
def test_header_binding_and_version():
    with open(os.path.join(ROOT, "include", "dmme_hip.h")) as f:
        text = f.read()
    for sym in ("dmme_distill_noise", "dmme_distill_mid", "dmme_distill_target"):
        assert f"DMME_API int {sym}(" in text and sym in _lib.PROTOTYPES
    assert _lib.lib().dmme_version() >= 117


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p, err = C.c_void_p(16), _lib.lib().dmme_last_error
    assert lib.dmme_distill_noise(None, p, p, p, p, p, 4, 1, 4, p, p, p, p, None) == -1 and b"distill_noise" in err()
    assert lib.dmme_distill_noise(p, p, p, p, p, p, 4, 1, 4, p, p, p, None, None) == -1 and b"distill_noise" in err()
    assert lib.dmme_distill_noise(p, p, p, p, p, p, 0, 1, 4, p, p, p, p, None) == -1 and b"N = 0" in err()
    assert lib.dmme_distill_mid(3, 0, p, p, p, p, 4, 1, 4, p, None) == -1 and b"prediction 3" in err()
    assert lib.dmme_distill_mid(0, 0, p, p, None, p, 4, 1, 4, p, None) == -1 and b"distill_mid" in err()
    assert lib.dmme_distill_mid(0, 0, p, p, p, p, 4, 0, 4, p, None) == -1 and b"B = 0" in err()
    assert lib.dmme_distill_target(-1, 0, p, p, p, p, p, p, 4, 1, 4, p, None) == -1 and b"prediction -1" in err()
    assert lib.dmme_distill_target(0, 0, p, p, p, None, p, p, 4, 1, 4, p, None) == -1 and b"distill_target" in err()
    assert lib.dmme_distill_target(0, 0, p, p, p, p, p, p, 4, 1, 0, p, None) == -1 and b"chw = 0" in err()


# ------------------------------------------------------------------------------------------ the process on the host
def test_the_teacher_is_frozen_and_stays_out_of_parameters_and_state_dict():
    student, teacher = _Net(), _Net()
    teacher.train()
    p = dmme_amd.ProgressiveDistillation(student, teacher, T, 4, prediction="x0")
    assert [id(q) for q in p.parameters()] == [id(student.a)] and list(p.state_dict()) == ["model.a"]
    assert not teacher.a.requires_grad and not teacher.training and student.a.requires_grad
    p.train()
    assert not teacher.training and student.training
    assert p.teacher is teacher and p.model is student and p.loss_weight == "truncated-snr"
    p.to(torch.float64)
    assert teacher.a.dtype == torch.float64  # the teacher follows .to()
    p.to(torch.float32)
    with torch.no_grad():
        student.a.fill_(0.25)
    p.halve()
    assert p.steps == 2 and float(teacher.a) == 0.25 and not teacher.a.requires_grad and tuple(p._rows.shape) == (3 * 12,) and tuple(p._tt.shape) == (3 * 2,)
    rows, tt = R.tables(p.alpha_bar.reshape(-1).double().numpy(), 2, "x0")
    assert np.array_equal(p._rows.numpy().reshape(-1, 12), rows.astype(np.float32), equal_nan=True) and np.array_equal(p._tt.numpy().reshape(-1, 2), tt)
    s = p.sampler()
    assert isinstance(s, dmme_amd.GeneralizedDDIM) and s.model is student and (s.sub_timesteps, s.tau_schedule, s.eta, s.prediction) == (2, "linear", 0.0, "x0")
    assert p.distill_meta() == {"steps": 2, "tau_schedule": "linear", "prediction": "x0"}
    with pytest.raises(ValueError, match="outside 1..2"):
        p.distill_target(torch.zeros(2, 3, 4, 4), torch.tensor([1, 3]), torch.zeros(2, 3, 4, 4))


def test_linear_decay_lr():
    par = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([par], lr=0.5)
    sched = dmme_amd.LinearDecayLR(opt, 4)
    seen = []
    for _ in range(6):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert seen == [0.5, 0.375, 0.25, 0.125, 0.0, 0.0]
    with pytest.raises(ValueError, match="total_steps"):
        dmme_amd.LinearDecayLR(opt, 0)


def test_checkpoint_records_the_distillation_and_loads_as_an_ordinary_one(tmp_path):
    from dmme_amd.checkpoint import checkpoint_dict, load_checkpoint, save_checkpoint

    student, teacher = _Net(), _Net()
    with torch.no_grad():
        student.a.fill_(0.125)
    lit = dmme_amd.LitDistill(dmme_amd.ProgressiveDistillation(student, teacher, T, 8, prediction="v"), stage_steps=10)
    assert lit.ema_decay == 0.0 and lit.diffusion_model.model is student
    path = str(tmp_path / "student.ckpt")
    save_checkpoint(path, lit, global_step=20)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["distill"] == {"steps": 8, "tau_schedule": "linear", "prediction": "v"} and list(ck["state_dict"]) == ["diffusion_model.model.a"]
    plain = dmme_amd.LitDDPM(model=_Net(), prediction="v")
    assert "distill" not in checkpoint_dict(plain)
    got = load_checkpoint(path, plain)
    assert got["distill"]["steps"] == 8 and got["global_step"] == 20 and float(plain.diffusion_model.model.a.detach()) == 0.125


# ------------------------------------------------------------------------------------------ the trainer
CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "ddim", "vpred", "cfg")}
_OK = ["distill", "--config", CFG["vpred"], "--ckpt-path", "t.ckpt", "--save-checkpoint", "o.ckpt", "--stage-steps", "5"]


@pytest.mark.parametrize("argv,msg", [
    (["fit", "--config", CFG["ddpm"], "--distill-from", "8"], "--distill-from belongs to `distill`"),
    (["sample", "--config", CFG["ddpm"], "--stage-steps", "8", "--distill-to", "1"], "--distill-to, --stage-steps belong to `distill`"),
    (["distill", "--config", CFG["vpred"], "--ckpt-path", "t.ckpt", "--save-checkpoint", "o.ckpt", "--distill-from", "8"], "distill needs --distill-to, --stage-steps"),
    (["distill", "--config", CFG["vpred"], "--save-checkpoint", "o.ckpt", "--stage-steps", "5", "--distill-from", "8", "--distill-to", "1"], "--ckpt-path"),
    (["distill", "--config", CFG["vpred"], "--ckpt-path", "t.ckpt", "--stage-steps", "5", "--distill-from", "8", "--distill-to", "1"], "--save-checkpoint"),
    (_OK + ["--distill-from", "12", "--distill-to", "4"], "power of two"),
    (_OK + ["--distill-from", "10", "--distill-to", "4"], "power of two"),
    (_OK + ["--distill-from", "4", "--distill-to", "4"], "must exceed"),
    (_OK + ["--distill-from", "4", "--distill-to", "0"], "must exceed"),
    (_OK[:-1] + ["0", "--distill-from", "4", "--distill-to", "1"], "--stage-steps must be at least 1"),
    (_OK + ["--distill-from", "4", "--distill-to", "1", "--max-steps", "3"], "do not go with `distill`"),
    (["fit", "--config", CFG["ddpm"], "--clip-x0"], "--clip-x0 belongs to --sampler dpm++"),
    (["sample", "--config", CFG["ddim"], "--tau-schedule", "linear"], "--tau-schedule belongs to --sampler dpm++"),
    (["sample", "--config", CFG["ddim"], "--sampler", "ddim-paper", "--tau-schedule", "logsnr"], "--tau-schedule belongs to --sampler dpm++"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


def test_trainer_takes_the_new_loss_weight_and_the_papers_tau_schedule():
    """the argument checks pass (what follows them needs a GPU): --loss-weight truncated-snr reaches the process the YAML builds, and
    --tau-schedule linear goes with --sampler ddim-paper"""
    import argparse

    from dmme_amd import trainer

    conf = trainer.parse_config(CFG["vpred"])
    trainer.override_prediction(conf, prediction=None, loss_weight="truncated-snr", snr_gamma=None)
    assert conf["model_spec"]["init_args"]["loss_weight"] == "truncated-snr"
    args = argparse.Namespace(command="sample", sampler="ddim-paper", tau_schedule="linear", solver_order=None, clip_x0=False, eta=None, steps=None, sample_steps=None)
    trainer._check_solver_args(args)
    args = argparse.Namespace(command="distill", sampler="config", tau_schedule=None, solver_order=None, clip_x0=True, eta=None, steps=None, sample_steps=None)
    trainer._check_solver_args(args)
