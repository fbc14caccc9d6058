"""CPU: consistency distillation's host side - the grid, its nesting and refusals, the tables against their float64 restatement and against
progressive distillation's formulas for the shared slots, the boundary row, the sampler rows against the literal update, the restatement's
bounds on the restatement itself, the ABI, every constructor refusal, the checkpoint entry and the trainer's refusals.  No GPU."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from dmme_amd.diffusion_models.distill import _x0_pair
from dmme_amd.equations.ddim import linear_tau

from . import consistency_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
STEPS = (1, 4, 50, 100, 250)
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
def test_grid_points_are_distinct_and_sub_grids_nest(N):
    tau = dmme_amd.consistency_grid(T, N)
    assert np.array_equal(tau, linear_tau(T, N).numpy()) and np.array_equal(tau, R.grid(T, N))
    assert tau[0] == 0 and tau[-1] == T and (np.diff(tau) > 0).all()
    for K in range(1, N + 1):
        if N % K == 0:  # a K-step sampler visits only timesteps the student was trained at
            assert np.array_equal(linear_tau(T, K).numpy(), tau[:: N // K]), (N, K)


def test_refusals_of_the_grid():
    with pytest.raises(ValueError, match="at least 1"):
        dmme_amd.consistency_grid(T, 0)
    with pytest.raises(ValueError, match="does not fit"):
        dmme_amd.consistency_grid(T, T + 1)
    with pytest.raises(ValueError, match="does not fit"):
        dmme_amd.consistency_grid(10, 11)  # (more points than timesteps cannot be distinct; with N <= T the spacing is at least 1 and they are)
    for T_, N_ in ((10, 8), (3, 2), (7, 7), (1000, 999)):
        assert (np.diff(dmme_amd.consistency_grid(T_, N_)) > 0).all()
    with pytest.raises(ValueError, match="prediction"):
        dmme_amd.consistency_rows(AB, 4, "score")
    with pytest.raises(ValueError, match="positive"):
        dmme_amd.consistency_rows(AB, 4, "v", sigma_data=0.0)


def test_boundary_scalings():
    cs0, co0 = R.scalings(0)
    assert (cs0, co0) == (1.0, 0.0)
    assert abs(R.scalings(20)[0] - 6.2e-6) < 5e-8
    from dmme_amd.diffusion_models.consistency import boundary_scalings

    for t in (0, 1, 20, 250, 1000):
        cs, co = boundary_scalings(t)
        want = R.scalings(t)
        assert (cs, co) == (float(want[0]), float(want[1]))
        assert abs(co * co + cs - 1.0) <= 1e-15  # co^2 = 1 - cs


# ------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("pred", R.PREDICTIONS)
@pytest.mark.parametrize("N", STEPS)
def test_tables(N, pred):
    rows, tt = dmme_amd.consistency_rows(AB, N, pred)
    want, want_tt = R.tables(AB, N, pred)
    assert rows.shape == (N + 1, 12) and rows.dtype == np.float64 and tt.shape == (N + 1, 2) and tt.dtype == np.int64
    assert np.array_equal(rows, want, equal_nan=True) and np.array_equal(tt, want_tt)
    assert np.isnan(rows[0]).all() and np.isfinite(rows[1:]).all() and (rows[1:, 10:] == 0).all()
    tau = R.grid(T, N)
    assert np.array_equal(tt[1:, 0], tau[1:]) and np.array_equal(tt[1:, 1], np.maximum(tau[:-1], 1)) and (tt[1:, 1] >= 1).all() and tuple(tt[0]) == (0, 0)
    # the first six slots are what distill_rows' formulas give for the pair (t, m)
    al, sg = np.sqrt(AB), np.sqrt(1.0 - AB)
    for i in range(1, N + 1):
        t, m = int(tau[i]), int(tau[i - 1])
        m1 = sg[m] / sg[t]
        six = _x0_pair(pred, al[t], sg[t]) + _x0_pair(pred, al[m], sg[m]) + (al[m] - m1 * al[t], m1)
        assert tuple(rows[i, :6]) == tuple(float(v) for v in six), i
        assert tuple(rows[i, 6:10]) == tuple(float(v) for v in R.scalings(t) + R.scalings(m)), i


@pytest.mark.parametrize("pred", R.PREDICTIONS)
@pytest.mark.parametrize("N", STEPS)
def test_the_boundary_row(N, pred):
    """i = 1 stands for m = 0: zh_m = x1, f(., 0; .) is the identity, and nothing divides by sigma_0 = 0"""
    rows, tt = dmme_amd.consistency_rows(AB, N, pred)
    r = rows[1]
    assert (r[R.M0], r[R.M1]) == (1.0, 0.0) and (r[R.CSM], r[R.COM]) == (1.0, 0.0) and tt[1, 1] == 1
    assert (r[R.P0M], r[R.P1M]) == ((1.0, 0.0) if pred == "x0" else (0.0, 1.0)) and (pred == "x0" or np.signbit(r[R.P0M]))
    if N > 1:
        assert (rows[2:, R.M1] > 0).all() and (rows[2:, R.COM] > 0).all() and (rows[2:, R.CSM] < 1).all()
    # in float32 the row returns z_m in value whatever the network says
    rng = np.random.default_rng(1)
    z, o = rng.standard_normal((1, 64)).astype(np.float32), rng.standard_normal((1, 64)).astype(np.float32)
    for clip in (False, True):
        assert np.array_equal(R.target32(clip, z, o, rows.astype(np.float32), np.asarray([1]), N), z)


# ------------------------------------------------------------------------------------------ the sampler rows
@pytest.mark.parametrize("pred", R.PREDICTIONS)
@pytest.mark.parametrize("K", (1, 2, 5, 10, 25, 50))
def test_sampler_rows_are_the_literal_update(K, pred):
    """k0 x + k1 eps + k2 z against alpha_p f(x, a) + sigma_p z, f from the network's raw output, in float64: eps is what the prediction
    adapter hands the chain (eps = a out + b x)"""
    from dmme_amd.diffusion_models.ddpm import prediction_table

    N = 50
    rows = dmme_amd.consistency_sampler_rows(AB, K)
    assert rows.shape == (K + 1, 3) and np.array_equal(rows, R.sampler_rows(AB, K)) and tuple(rows[0]) == (1.0, 0.0, 0.0)
    s = dmme_amd.ConsistencySampler(torch.nn.Identity(), T, K, N, prediction=pred)
    assert isinstance(s, dmme_amd.GeneralizedDDIM) and (s.sub_timesteps, s.tau_schedule, s.eta, s.prediction, s.train_steps) == (K, "linear", 0.0, pred, N)
    assert s._rev_rows == [(float(np.float32(a)), float(np.float32(b)), float(np.float32(c)), 0.0) for a, b, c in rows]
    assert s._chain_tables()[1] == s._rev_rows and s._chain_kind == _lib.CHAIN_GDDIM and s._draws == (K > 1)
    assert rows[1, 2] == 0.0 and (rows[2:, 2] > 0).all()
    ptab = prediction_table(AB, pred)
    tau = R.grid(T, K)
    rng = np.random.default_rng(K)
    x, out, z = rng.standard_normal(32), rng.standard_normal(32), rng.standard_normal(32)
    worst = 0.0
    for i in range(1, K + 1):
        a, b = (1.0, 0.0) if pred == "eps" else (float(ptab[tau[i], 0]), float(ptab[tau[i], 1]))
        eps = a * out + b * x
        got = rows[i, 0] * x + rows[i, 1] * eps + rows[i, 2] * z
        want = R.sample_step64(pred, AB, K, i, x, out, z)
        scale = np.abs(rows[i, 0] * x) + np.abs(rows[i, 1] * eps) + 1.0
        worst = max(worst, float((np.abs(got - want) / scale).max()))
    print(f"K = {K} {pred}: sampler rows against the literal update: {worst:.2e}")
    assert worst <= 1e-12


def test_sampler_refusals():
    for K in (3, 7, 100):
        with pytest.raises(ValueError, match="does not divide"):
            dmme_amd.ConsistencySampler(torch.nn.Identity(), T, K, 50)
    with pytest.raises(ValueError, match="does not divide"):
        dmme_amd.ConsistencySampler(torch.nn.Identity(), T, 0, 50)
    s = dmme_amd.ConsistencySampler(torch.nn.Identity(), T, 2, 4)
    with pytest.raises(NotImplementedError, match="no forward direction"):
        s.encode(torch.zeros(1, 3, 4, 4))
    with pytest.raises(NotImplementedError, match="no forward direction"):
        s.interpolate(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), [0.5])
    p = dmme_amd.ConsistencyDistillation(_Net(), _Net(), T, 4, prediction="x0")
    with pytest.raises(ValueError, match="does not divide"):
        p.sampler(3)
    s = p.sampler(2, threshold="static")
    assert isinstance(s, dmme_amd.ConsistencySampler) and s.model is p.model and (s.sub_timesteps, s.train_steps, s.prediction, s.threshold) == (2, 4, "x0", "static")


# ------------------------------------------------------------------------------------------ the restatement inside its own bounds
def _inputs(N, seed, chw=48):
    rng = np.random.default_rng(seed)
    idx = np.arange(1, N + 1)
    return (idx,) + tuple(rng.standard_normal((N, chw)).astype(np.float32) for _ in range(4))


@pytest.mark.parametrize("metric", (R.PSEUDO_HUBER, R.L2))
@pytest.mark.parametrize("pred", R.PREDICTIONS)
@pytest.mark.parametrize("clip", (False, True))
def test_the_bounds_hold_for_the_restatement_in_fp32(pred, clip, metric):
    """tests/consistency_ref.py in float32 against Algorithm 2 in float64 must sit inside its own bounds before the device is asked to"""
    N = 50
    idx, z_t, o1, o_m, out = _inputs(N, 9)
    rows64, _ = R.tables(AB, N, pred)
    rows32 = rows64.astype(np.float32)
    z_m = R.mid32(clip, z_t, o1, rows32, idx, N)
    ft = R.target32(clip, z_m, o_m, rows32, idx, N)
    want = R.algorithm2(pred, clip, AB, N, idx, z_t, o1, o_m)
    b = R.target_bounds(clip, rows64, idx, z_t, o1, o_m)
    r_mid = float((np.abs(z_m - want["z_m"]) / b["z_m"]).max())
    r_ft = float((np.abs(ft - want["f_target"]) / b["f_target"]).max())
    chw = z_t[0].size
    c32, gs32 = np.float32(R.HUBER_C * np.sqrt(chw)), np.float32(3.0)
    sq = R.squares32(z_t, out, ft, rows32, idx, N)
    S32 = sq.astype(np.float64).sum(axis=1).astype(np.float32)
    d32, g32 = R.finish(metric, S32, rows32, idx, N, chw, c32, gs32)
    grad32 = R.d_out32(g32, z_t, out, ft, rows32, idx, N)
    loss32 = float(np.float32(d32.astype(np.float64).sum()) * np.float32(1.0 / N))
    loss, grad, S, _ = R.loss64(pred, metric, AB, N, idx, z_t, out, want["f_target"], float(c32), grad_scale=float(gs32))
    lb = R.loss_bounds(metric, rows64, idx, z_t, out, want["f_target"], b["f_target"], float(c32), float(gs32))
    r_S = float((np.abs(S32 - S) / lb["sumsq"]).max())
    r_loss = abs(loss32 - loss) / lb["loss"]
    r_grad = float((np.abs(grad32 - grad) / lb["grad"]).max())
    print(f"{pred} clip {clip} metric {metric}: the restatement in fp32 at {r_mid:.3f} (zh_m), {r_ft:.3f} (f_target), {r_S:.3f} (S_b), {r_loss:.3f} (loss), "
          f"{r_grad:.3f} (gradient) of the bounds")
    assert max(r_mid, r_ft, r_S, r_loss, r_grad) <= 1.0


def test_ema_restatement():
    rng = np.random.default_rng(2)
    d, s = rng.standard_normal(9).astype(np.float32), rng.standard_normal(9).astype(np.float32)
    assert np.array_equal(R.ema32(d, s, 1.0), d) and np.array_equal(R.ema32(d, s, 0.0), s)
    assert np.array_equal(R.ema32(d, s, 0.5), ((d * np.float32(0.5)) + (s * np.float32(0.5))).astype(np.float32))
    one_minus = np.float32(1.0 - float(np.float32(0.95)))
    assert np.array_equal(R.ema32(d, s, 0.95), ((d * np.float32(0.95)).astype(np.float32) + (s * one_minus).astype(np.float32)).astype(np.float32))


# ------------------------------------------------------------------------------------------ the header, the binding, the C argument checks
def test_header_binding_and_version():
    with open(os.path.join(ROOT, "include", "dmme_hip.h")) as f:
        text = f.read()
    for sym in ("dmme_cm_target", "dmme_cm_loss", "dmme_ema_lerp"):
        assert f"DMME_API int {sym}(" in text and sym in _lib.PROTOTYPES
    assert _lib.lib().dmme_version() >= 119
    assert "65 * B floats" in text and _lib.CM_METRICS == {"pseudo-huber": 0, "l2": 1}


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p, err = C.c_void_p(16), _lib.lib().dmme_last_error
    assert lib.dmme_cm_target(0, None, p, p, p, 4, 1, 4, p, None) == -1 and b"cm_target" in err()
    assert lib.dmme_cm_target(0, p, p, p, p, 0, 1, 4, p, None) == -1 and b"N = 0" in err()
    assert lib.dmme_cm_target(0, p, p, p, p, 4, 1, 0, p, None) == -1 and b"chw = 0" in err()
    assert lib.dmme_cm_loss(2, p, p, p, p, p, 4, 1, 4, 1.0, p, None, None, 1.0, p, None) == -1 and b"metric 2" in err()
    assert lib.dmme_cm_loss(0, p, p, p, p, p, 4, 1, 4, 1.0, p, None, None, 1.0, None, None) == -1 and b"cm_loss" in err()
    assert lib.dmme_cm_loss(0, p, p, p, p, p, 4, 65536, 4, 1.0, p, None, None, 1.0, p, None) == -1 and b"65535" in err()
    assert lib.dmme_cm_loss(0, p, p, p, p, p, 4, 1, 4, 0.0, p, None, None, 1.0, p, None) == -1 and b"c > 0" in err()
    assert lib.dmme_ema_lerp(None, p, 4, 0.5, None) == -1 and b"ema_lerp" in err()
    assert lib.dmme_ema_lerp(p, p, 0, 0.5, None) == -1 and b"numel = 0" in err()
    assert lib.dmme_ema_lerp(p, p, 4, 1.5, None) == -1 and b"outside [0, 1]" in err()


# ------------------------------------------------------------------------------------------ the process on the host
def test_constructor_refusals():
    mk = lambda **kw: dmme_amd.ConsistencyDistillation(_Net(), _Net(), T, 4, **kw)  # noqa: E731
    net = _Net()
    with pytest.raises(ValueError, match="two networks"):
        dmme_amd.ConsistencyDistillation(net, net, T, 4)
    with pytest.raises(ValueError, match="metric"):
        mk(metric="lpips")
    for c in (0.0, -1.0, float("nan"), True):
        with pytest.raises(ValueError, match="huber_c"):
            mk(huber_c=c)
    for d in (-0.1, 1.5, True):
        with pytest.raises(ValueError, match="target_decay"):
            mk(target_decay=d)
    with pytest.raises(ValueError, match="positive"):
        mk(sigma_data=-1.0)
    with pytest.raises(ValueError, match="positive"):
        mk(timestep_scaling=0.0)
    with pytest.raises(ValueError, match="prediction"):
        mk(prediction="score")
    with pytest.raises(ValueError, match="at least 1"):
        dmme_amd.ConsistencyDistillation(_Net(), _Net(), T, 0)
    with pytest.raises(ValueError, match="does not fit"):
        dmme_amd.ConsistencyDistillation(_Net(), _Net(), 10, 11)


def test_networks_with_labels_or_two_planes_are_refused():
    tiny = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=1)
    from dmme_amd.models.iddpm import UNet as IDDPMUNet

    plain = dmme_amd.UNet(**tiny)
    for bad in (dmme_amd.ConditionalUNet(num_classes=3, **tiny), IDDPMUNet(**tiny)):
        with pytest.raises(NotImplementedError, match="out of scope"):
            dmme_amd.ConsistencyDistillation(plain, bad, T, 4)
        with pytest.raises(NotImplementedError, match="out of scope"):
            dmme_amd.ConsistencyDistillation(bad, plain, T, 4)


def test_the_teacher_and_the_target_are_frozen_and_stay_out_of_parameters_and_state_dict():
    student, teacher = _Net(), _Net()
    teacher.train()
    p = dmme_amd.ConsistencyDistillation(student, teacher, T, 4, prediction="x0")
    assert [id(q) for q in p.parameters()] == [id(student.a)] and list(p.state_dict()) == ["model.a"]
    assert not teacher.a.requires_grad and not teacher.training and student.a.requires_grad and p.target is None
    p.train()
    assert not teacher.training and student.training and p.teacher is teacher and p.model is student
    assert (p.steps, p.metric, p.target_decay, p.sigma_data, p.timestep_scaling, p.clip_x0, p.loss_weight) == (4, "pseudo-huber", 0.0, 0.5, 10.0, False, "uniform")
    assert p.huber_constant(3072) == 0.00054 * np.sqrt(3072.0) and dmme_amd.ConsistencyDistillation(_Net(), _Net(), T, 4, huber_c=0.25).huber_constant(3072) == 0.25
    rows, tt = R.tables(p.alpha_bar.reshape(-1).double().numpy(), 4, "x0")
    assert np.array_equal(p._rows.numpy().reshape(-1, 12), rows.astype(np.float32), equal_nan=True) and np.array_equal(p._tt.numpy().reshape(-1, 2), tt)
    assert p.consistency_meta() == {"steps": 4, "prediction": "x0", "sigma_data": 0.5, "timestep_scaling": 10.0}
    with pytest.raises(ValueError, match="outside 1..4"):
        p.consistency_target(torch.zeros(2, 3, 4, 4), torch.tensor([1, 5]), torch.zeros(2, 3, 4, 4))
    p.after_step()  # (nothing to move)
    with torch.no_grad():
        student.a.fill_(0.25)
    q = dmme_amd.ConsistencyDistillation(student, teacher, T, 4, prediction="x0", target_decay=0.5)
    assert q.target is not student and q.target is not teacher and float(q.target.a) == 0.25 and not q.target.a.requires_grad and not q.target.training
    assert [id(v) for v in q.parameters()] == [id(student.a)] and list(q.state_dict()) == ["model.a"]
    q.to(torch.float64)
    assert teacher.a.dtype == torch.float64 and q.target.a.dtype == torch.float64  # both follow .to()
    q.to(torch.float32)
    with torch.no_grad():
        student.a.fill_(0.75)
    q.reset_target()
    assert float(q.target.a) == 0.75 and not q.target.a.requires_grad and float(teacher.a) == 0.5


def test_checkpoint_records_the_consistency_entry_and_loads_as_an_ordinary_one(tmp_path):
    from dmme_amd.checkpoint import checkpoint_dict, load_checkpoint, save_checkpoint

    student, teacher = _Net(), _Net()
    with torch.no_grad():
        student.a.fill_(0.125)
    lit = dmme_amd.LitConsistency(dmme_amd.ConsistencyDistillation(student, teacher, T, 50, prediction="v", target_decay=0.95))
    assert lit.ema_decay == 0.0 and lit.diffusion_model.model is student and lit.sample_steps == 1
    with pytest.raises(TypeError, match="ConsistencyDistillation"):
        dmme_amd.LitConsistency(dmme_amd.DDPM(_Net(), T))
    path = str(tmp_path / "student.ckpt")
    save_checkpoint(path, lit, global_step=20)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["consistency"] == {"steps": 50, "prediction": "v", "sigma_data": 0.5, "timestep_scaling": 10.0} and "distill" not in ck
    assert list(ck["state_dict"]) == ["diffusion_model.model.a"]  # (neither the teacher nor the target network)
    plain = dmme_amd.LitDDPM(model=_Net(), prediction="v")
    assert "consistency" not in checkpoint_dict(plain)
    got = load_checkpoint(path, plain)
    assert got["consistency"]["steps"] == 50 and got["global_step"] == 20 and float(plain.diffusion_model.model.a.detach()) == 0.125


# ------------------------------------------------------------------------------------------ the trainer
CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "vpred", "cfg")}
_OK = ["consistency", "--config", CFG["vpred"], "--ckpt-path", "t.ckpt", "--save-checkpoint", "o.ckpt", "--consistency-steps", "50", "--max-steps", "5"]


@pytest.mark.parametrize("argv,msg", [
    (["fit", "--config", CFG["ddpm"], "--consistency-steps", "8"], "--consistency-steps belongs to `consistency`"),
    (["sample", "--config", CFG["ddpm"], "--metric", "l2", "--target-decay", "0.5"], "--metric, --target-decay belong to `consistency`"),
    (["sample", "--config", CFG["vpred"], "--huber-c", "0.1"], "--huber-c belongs to `consistency`"),
    (_OK[:-4], "consistency needs --consistency-steps"),
    (_OK[:-2], "consistency needs --consistency-steps"),
    (["consistency", "--config", CFG["vpred"], "--save-checkpoint", "o.ckpt", "--consistency-steps", "50", "--max-steps", "5"], "--ckpt-path"),
    (["consistency", "--config", CFG["vpred"], "--ckpt-path", "t.ckpt", "--consistency-steps", "50", "--max-steps", "5"], "--save-checkpoint"),
    (_OK + ["--sample-steps", "2"], "do not go with `consistency`"),
    (_OK[:-3] + ["0", "--max-steps", "5"], "must be at least 1"),
    (_OK + ["--metric", "l2", "--huber-c", "0.1"], "--huber-c C > 0 belongs to the pseudo-Huber metric"),
    (_OK + ["--huber-c", "0"], "--huber-c C > 0"),
    (_OK + ["--target-decay", "1.5"], "outside [0, 1]"),
    (_OK + ["--distill-from", "4"], "--distill-from belongs to `distill`"),
    (["fit", "--config", CFG["ddpm"], "--clip-x0"], "--clip-x0 belongs to --sampler dpm++"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


def test_trainer_takes_clip_x0_with_consistency():
    import argparse

    from dmme_amd import trainer

    args = argparse.Namespace(command="consistency", sampler="config", tau_schedule=None, solver_order=None, clip_x0=True, eta=None, steps=None, sample_steps=None)
    trainer._check_solver_args(args)
