"""CPU: the host side of x0 / v prediction and min-SNR loss weights - the adapter's and the weights' tables against the numpy
restatement (tests/pred_ref.py) and hand values, the round trip target -> eps in float64, constructor validation, and the trainer's
flags and YAML keys reaching the process."""

import os

import numpy as np
import pytest
import torch

from . import pred_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _schedules():
    """(name, process) over the linear T = 1000 schedule and over a cosine one installed through `_use_alpha_bar`"""
    import dmme_amd

    out = []
    for name in ("linear", "cosine"):
        for pred in (R.X0, R.V):
            p = dmme_amd.DDPM(torch.nn.Identity(), 1000, prediction=pred, loss_weight="min-snr")
            if name == "cosine":
                p._use_alpha_bar(torch.from_numpy(R.cosine_alpha_bar(1000)).to(torch.float32))
            out.append((name, pred, p))
    return out


def test_tables_are_the_float64_formulas_rounded_once():
    """the device tables the process registers: pred_ref's float64 tables over the process's own alpha_bar, rounded to fp32 - bit for bit,
    the NaN row of x0 included - for the linear schedule and for one that replaced it after construction"""
    for name, pred, p in _schedules():
        ab = p.alpha_bar.reshape(-1).double().numpy()
        assert ab[0] == 1.0 and ab.size == 1001
        if name == "linear":
            np.testing.assert_allclose(ab, R.linear_alpha_bar(1000), rtol=2e-6)  # (the buffer is fp32: 1000 fp32 products)
        got = p._pred_ab.numpy().reshape(-1, 2)
        want = R.ab_table(ab, pred).astype(np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), (name, pred)
        assert np.isnan(got[0]).all() == (pred == R.X0) and np.isfinite(got[1:]).all()
        w = p._loss_w.numpy()
        assert np.array_equal(w, R.weight_table(ab, pred, 5.0).astype(np.float32)), (name, pred)
        assert "_pred_ab" not in p.state_dict() and "_loss_w" not in p.state_dict()


@pytest.mark.parametrize("pred", [R.X0, R.V])
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_round_trip_target_to_eps_is_the_noise(schedule, pred):
    """float64: to_eps(target_p(x0, z), x_t) == z at every t in 1..T.  Bound 1e-9 relative to max|z| b_t: the map multiplies the target's
    float64 rounding (2^-53 = 1.1e-16) by at most b_t, which leaves about five orders of magnitude of margin."""
    import dmme_amd

    p = dmme_amd.DDPM(torch.nn.Identity(), 1000, prediction=pred)
    if schedule == "cosine":
        p._use_alpha_bar(torch.from_numpy(R.cosine_alpha_bar(1000)).to(torch.float32))
    ab = p.alpha_bar.reshape(-1).double().numpy()
    T = ab.size - 1
    sa, sd = np.sqrt(ab), np.sqrt(1 - ab)
    table = R.ab_table(ab, pred)
    rng = np.random.RandomState(3)
    t = np.arange(1, T + 1)
    x0, z = rng.uniform(-1, 1, (T, 7)), rng.standard_normal((T, 7))
    x_t = R.q_sample(sa, sd, x0, z, t)
    e = R.to_eps(table, R.target(pred, sa, sd, x0, z, t), x_t, t)
    assert e.dtype == np.float64
    rel = np.abs(e - z).max(axis=1) / (np.abs(z).max() * np.abs(table[1:, 1]))
    print(f"{schedule} {pred}: worst round-trip error {rel.max():.3e} of max|z| b_t (bound 1e-9), at t = {1 + int(rel.argmax())}")
    assert rel.max() <= 1e-9


def test_weight_tables_against_hand_values():
    """min-SNR-gamma at three timesteps of a hand-made alpha_bar: snr = abar/(1-abar) = 9, 1, 1/9 with gamma = 5"""
    from dmme_amd.diffusion_models.ddpm import loss_weight_table, prediction_table

    ab = np.array([1.0, 0.9, 0.5, 0.1])
    for table in (lambda p: loss_weight_table(ab, p, "min-snr", 5.0), lambda p: R.weight_table(ab, p, 5.0)):
        np.testing.assert_allclose(table("eps"), [0.0, 5.0 / 9.0, 1.0, 1.0], rtol=1e-14)
        np.testing.assert_allclose(table("x0"), [5.0, 5.0, 1.0, 1.0 / 9.0], rtol=1e-14)
        np.testing.assert_allclose(table("v"), [0.0, 0.5, 0.5, 0.1], rtol=1e-14)
    assert np.array_equal(loss_weight_table(ab, "v", "uniform"), np.ones(4))
    # the three weights are one weight on the x0 error: w_eps snr = w_x0 = w_v (snr + 1)
    snr = ab[1:] / (1 - ab[1:])
    np.testing.assert_allclose(R.weight_table(ab, "eps")[1:] * snr, R.weight_table(ab, "x0")[1:], rtol=1e-14)
    np.testing.assert_allclose(R.weight_table(ab, "v")[1:] * (snr + 1), R.weight_table(ab, "x0")[1:], rtol=1e-14)
    # the adapter's table at the same points
    np.testing.assert_allclose(prediction_table(ab, "x0")[1:], [[-3.0, np.sqrt(10.0)], [-1.0, np.sqrt(2.0)], [-1.0 / 3.0, 1.0 / np.sqrt(0.9)]], rtol=1e-14)
    np.testing.assert_allclose(prediction_table(ab, "v"), [[1.0, 0.0], [np.sqrt(0.9), np.sqrt(0.1)], [np.sqrt(0.5), np.sqrt(0.5)], [np.sqrt(0.1), np.sqrt(0.9)]], rtol=1e-14)
    assert np.isnan(prediction_table(ab, "x0")[0]).all()


def test_constructor_validation_and_pass_through():
    import dmme_amd
    from dmme_amd import _lib

    net = torch.nn.Identity()
    for kw in (dict(prediction="velocity"), dict(prediction="EPS"), dict(loss_weight="snr"), dict(snr_gamma=0.0), dict(snr_gamma=-1.0), dict(snr_gamma=float("nan"))):
        with pytest.raises(ValueError):
            dmme_amd.DDPM(net, 10, **kw)
    with pytest.raises(TypeError):
        dmme_amd.DDPM(net, 10, 1e-4, 0.02, "v")  # keyword-only: the positional signature is the reference's
    # the default is today's process: no table, no weight, the eps code
    p = dmme_amd.DDPM(net, 10)
    assert (p.prediction, p.loss_weight, p.snr_gamma, p._pred) == ("eps", "uniform", 5.0, _lib.PRED_EPS)
    assert not hasattr(p, "_pred_ab") and not hasattr(p, "_loss_w")
    assert not hasattr(dmme_amd.DDPM(net, 10, prediction="v"), "_loss_w") and not hasattr(dmme_amd.DDPM(net, 10, loss_weight="min-snr"), "_pred_ab")
    kw = dict(prediction="v", loss_weight="min-snr", snr_gamma=3.0)
    cond = dmme_amd.ConditionalUNet(num_classes=3, pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    clf = dmme_amd.EncoderClassifier(num_classes=3, pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    procs = [dmme_amd.DDIM(net, 20, 5, **kw), dmme_amd.GeneralizedDDIM(net, 20, 5, eta=0.5, **kw), dmme_amd.DPMSolverPP(net, 20, 5, **kw), dmme_amd.RePaint(net, 20, 10, 2, 2, **kw),
             dmme_amd.ClassifierFreeDDPM(cond, 20, **kw), dmme_amd.ClassifierFreeDDIM(cond, 20, 5, **kw), dmme_amd.ClassifierFreeDPMSolver(cond, 20, 5, **kw),
             dmme_amd.ClassifierGuidedDDPM(net, clf, 20, **kw), dmme_amd.ClassifierGuidedDDIM(net, clf, 20, 5, **kw)]
    for q in procs:
        assert (q.prediction, q.loss_weight, q.snr_gamma, q._pred) == ("v", "min-snr", 3.0, _lib.PRED_V), type(q).__name__
        ab = q.alpha_bar.reshape(-1).double().numpy()
        assert np.array_equal(q._pred_ab.numpy().reshape(-1, 2), R.ab_table(ab, "v").astype(np.float32)), type(q).__name__
        assert np.array_equal(q._loss_w.numpy(), R.weight_table(ab, "v", 3.0).astype(np.float32)), type(q).__name__
    # a sampler built over another process takes its schedule AND its prediction
    base = dmme_amd.DDPM(net, 20, prediction="x0")
    base._use_alpha_bar(torch.from_numpy(R.cosine_alpha_bar(20)).to(torch.float32))
    for q in (dmme_amd.DPMSolverPP.from_process(base, sub_timesteps=5), dmme_amd.RePaint.from_process(base, sub_timesteps=10, jump_length=2, resamples=2)):
        assert q.prediction == "x0" and torch.equal(q.alpha_bar, base.alpha_bar)
        assert np.array_equal(q._pred_ab.numpy(), base._pred_ab.numpy(), equal_nan=True)


def test_iddpm_refuses_other_predictions():
    import dmme_amd

    net = torch.nn.Identity()
    assert dmme_amd.IDDPM(net, 10, prediction="eps", loss_weight="uniform").prediction == "eps"
    for kw in (dict(prediction="v"), dict(prediction="x0"), dict(loss_weight="min-snr")):
        with pytest.raises(ValueError, match="IDDPM"):
            dmme_amd.IDDPM(net, 10, **kw)


def test_trainer_flags_and_yaml_reach_the_process():
    from dmme_amd import trainer

    # the new YAML
    conf = trainer.parse_config(os.path.join(ROOT, "configs", "vpred", "cifar10.yaml"))
    dm = trainer.build_module(conf).diffusion_model
    assert (type(dm).__name__, dm.prediction, dm.loss_weight, dm.snr_gamma, dm.timesteps) == ("DDPM", "v", "min-snr", 5.0, 1000)
    # ... is the DDPM config but for those keys
    base = trainer.parse_config(os.path.join(ROOT, "configs", "ddpm", "cifar10.yaml"))
    args = dict(conf["model_spec"]["init_args"])
    assert [args.pop(k) for k in ("prediction", "loss_weight", "snr_gamma")] == ["v", "min-snr", 5.0]
    assert args == base["model_spec"]["init_args"] and all(conf[k] == base[k] for k in ("batch_size", "max_steps", "precision", "gradient_clip_val"))
    # the flags override a YAML that says nothing ...
    for name, cls in (("ddpm", "DDPM"), ("ddim", "DDIM"), ("cfg", "ClassifierFreeDDPM")):
        conf = trainer.parse_config(os.path.join(ROOT, "configs", name, "cifar10.yaml"))
        trainer.override_prediction(conf, prediction="v", loss_weight="min-snr", snr_gamma=None)
        dm = trainer.build_module(conf).diffusion_model
        assert (type(dm).__name__, dm.prediction, dm.loss_weight, dm.snr_gamma) == (cls, "v", "min-snr", 5.0)
    # ... and one that says something else
    conf = trainer.parse_config(os.path.join(ROOT, "configs", "vpred", "cifar10.yaml"))
    trainer.override_prediction(conf, prediction="eps", loss_weight=None, snr_gamma=2.0)
    dm = trainer.build_module(conf).diffusion_model
    assert (dm.prediction, dm.loss_weight, dm.snr_gamma) == ("eps", "min-snr", 2.0)
    # Improved DDPM takes none of them
    conf = trainer.parse_config(os.path.join(ROOT, "configs", "iddpm", "cifar10.yaml"))
    with pytest.raises(SystemExit, match="--prediction"):
        trainer.override_prediction(conf, prediction="v", loss_weight=None, snr_gamma=None)
    trainer.override_prediction(conf, prediction=None, loss_weight=None, snr_gamma=None)  # nothing given: nothing touched
    assert trainer.build_module(conf).diffusion_model.prediction == "eps"


@pytest.mark.parametrize("name", ["ddpm", "ddim", "iddpm", "cfg"])
def test_existing_configs_still_build_eps_processes(name):
    """the YAML files that say nothing about the prediction build what they built: eps, uniform weights, no table"""
    from dmme_amd import trainer

    dm = trainer.build_module(trainer.parse_config(os.path.join(ROOT, "configs", name, "cifar10.yaml"))).diffusion_model
    assert dm.prediction == "eps" and dm.loss_weight == "uniform" and not hasattr(dm, "_pred_ab") and not hasattr(dm, "_loss_w")


@pytest.mark.skipif(not os.path.isdir("/root/reference/configs"), reason="reference checkout absent (GPU box)")
@pytest.mark.parametrize("rel", ["ddpm/cifar10", "ddim/cifar10", "iddpm/cifar10", "ddpm/lsun_church"])
def test_reference_yaml_files_still_build_eps_processes(rel):
    """build container only (as tests/test_host_logic.py reads them): the reference's own files, in place"""
    from dmme_amd import trainer

    dm = trainer.build_module(trainer.parse_config(f"/root/reference/configs/{rel}.yaml")).diffusion_model
    assert dm.prediction == "eps" and dm.loss_weight == "uniform"
