"""Host-only checks of DPM-Solver++(2M) (dmme_amd.DPMSolverPP): the order and convergence of the float64 restatement
(tests/dpmpp_ref.py) under an exact noise predictor, the grid and the rows the package builds against the restatement's, clipping,
the argument checks of the new C entry points and of the trainer's new flags (no GPU touched).

End-gain error |x_0 / x_T - exact|, exact predictor of N(0, 0.5^2 I) data, T = 1000, linear beta, float64 (test_order_and_convergence
prints this table):
    grid          S  steps   first order (= DDIM, eta = 0)   2M
    quadratic    10     10   7.68e-02                        2.45e-02
    quadratic    20     20   4.01e-02                        1.12e-02
    quadratic    40     40   2.05e-02                        2.34e-03
    logsnr       10     10   1.18e-01                        1.59e-02
    logsnr       20     20   5.97e-02                        7.28e-03
    logsnr       40     39   3.02e-02                        1.83e-03"""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib

from . import ddim_ref as DR
from . import dpmpp_ref as R

T = 1000


def test_order_one_is_ddim_at_eta_zero():
    """order = 1 in the data-prediction form against ddim_ref.reverse_rows(eta = 0) on the same grid, step by step on the same input
    (float64, gaussian_predictor): 1e-12 relative"""
    abar = R.alpha_bar(T)
    model = R.gaussian_predictor(abar)
    worst = 0.0
    for kind, S in (("quadratic", 20), ("logsnr", 20), ("linear", 10)):
        g = R.grid(abar, S, kind)
        tab, ddim = R.rows(abar, g, order=1), DR.reverse_rows(abar, g, 0.0)
        assert np.all(tab[:, R.W] == 0.0)
        x = torch.from_numpy(np.random.RandomState(3).standard_normal(64))
        for i in range(len(g) - 1, 0, -1):
            eps = model(x, torch.tensor([g[i]]))
            a, _ = R.step(x, eps, None, tab[i], False)
            b = DR.step(x, eps, None, ddim[i])
            worst = max(worst, float(((a - b).abs() / b.abs()).max()))
            x = b
    print(f"order 1 vs DDIM (eta = 0), largest relative gap over every step: {worst:.2e}")
    assert worst <= 1e-12


def test_order_and_convergence():
    """2M at most half the first-order error on the same grid, for {quadratic, logsnr} x S in {10, 20, 40}; 2M at S = 40 at most a
    third of 2M at S = 20 (the linear tau grid misses the first condition at S = 10 and is left out)"""
    abar = R.alpha_bar(T)
    print(f"{'grid':<10} {'S':>3} {'steps':>5}   first order   2M")
    err = {}
    for kind in ("quadratic", "logsnr"):
        for S in (10, 20, 40):
            g = R.grid(abar, S, kind)
            e1, e2 = R.end_gain_error(abar, g, 1), R.end_gain_error(abar, g, 2)
            ddim = R.ddim_gain_error(abar, g)
            print(f"{kind:<10} {S:>3} {len(g) - 1:>5}   {e1:.2e}      {e2:.2e}")
            assert abs(e1 - ddim) <= 1e-12 and e2 <= 0.5 * e1, (kind, S, e1, e2)
            err[kind, S] = e2
        assert err[kind, 40] <= err[kind, 20] / 3, (kind, err)


@pytest.mark.parametrize("kind", ["linear", "quadratic", "logsnr"])
@pytest.mark.parametrize("S", [1, 5, 20, 80])
def test_grid(kind, S):
    abar = R.alpha_bar(T)
    proc = dmme_amd.DPMSolverPP(torch.nn.Identity(), T, S, kind)
    g = proc._tau_host
    assert g == R.grid(abar, S, kind) and g[0] == 0 and g[-1] == T and all(b > a for a, b in zip(g, g[1:]))
    assert proc.n_steps == len(g) - 1 <= S and [int(v) for v in proc.tau] == g
    if S == 80:
        assert proc.n_steps == {"linear": 80, "quadratic": 78, "logsnr": 76}[kind]


@pytest.mark.parametrize("T_,S,kind", [(1000, 20, "logsnr"), (1000, 80, "quadratic"), (100, 5, "linear")])
@pytest.mark.parametrize("order", [1, 2])
def test_rows(T_, S, kind, order):
    abar = R.alpha_bar(T_)
    proc = dmme_amd.DPMSolverPP(torch.nn.Identity(), T_, S, kind, order=order, clip_x0=(order == 1))
    assert np.array_equal(proc.alpha_bar.reshape(-1).double().numpy(), abar)
    n, rows, ttab = proc._chain_tables()
    want = R.rows(abar, ttab, order, order == 1).astype(np.float32).astype(np.float64)
    assert n == proc.n_steps == len(rows) - 1 and np.array_equal(np.array(rows), want)  # fp32 values held exactly in python floats
    assert tuple(rows[1][2:5]) == (0.0, 1.0, 0.0) and rows[n][4] == 0.0
    assert all(r[5] == float(order == 1) and r[6] == 1.0 and r[7] == 0.0 for r in rows)
    if order == 1:
        assert all(r[4] == 0.0 for r in rows)
    elif n > 2:
        assert all(rows[i][4] > 0.0 for i in range(2, n))


def test_from_process_takes_the_schedule():
    p = dmme_amd.IDDPM(torch.nn.Identity(), 100)
    s = dmme_amd.DPMSolverPP.from_process(p, sub_timesteps=5)
    assert torch.equal(s.alpha_bar, p.alpha_bar) and s.timesteps == 100 and s.model is p.model
    ab = p.alpha_bar.reshape(-1).double().numpy()
    assert s._tau_host == R.grid(ab, 5, "logsnr")
    assert np.array_equal(np.array(s._chain_tables()[1]), R.rows(ab, s._tau_host).astype(np.float32).astype(np.float64))
    assert torch.allclose(s._sqrt_alpha_bar, p._sqrt_alpha_bar) and not torch.equal(s.alpha_bar, dmme_amd.DDPM(torch.nn.Identity(), 100).alpha_bar)


def test_python_surface_and_constructor_errors():
    assert "DPMSolverPP" in dmme_amd.__all__ and issubclass(dmme_amd.DPMSolverPP, dmme_amd.DDIM)
    assert issubclass(dmme_amd.ClassifierFreeDPMSolver, dmme_amd.DPMSolverPP)
    proc = dmme_amd.DPMSolverPP(torch.nn.Identity(), 100, 5)
    assert proc._chain_kind == _lib.CHAIN_DPMPP == 8 and _lib.CHAIN_DPMPP_CFG == 9 and proc.order == 2 and proc.tau_schedule == "logsnr"
    for kw in (dict(order=3), dict(order=0), dict(tau_schedule="cosine"), dict(sub_timesteps=0), dict(sub_timesteps=101),
               dict(alpha_bar=torch.linspace(1, 0.1, 50)), dict(alpha_bar=torch.ones(101))):
        with pytest.raises(ValueError):
            dmme_amd.DPMSolverPP(torch.nn.Identity(), 100, **{"sub_timesteps": 5, **kw})
    for bad in (0, proc.n_steps + 1):
        with pytest.raises(ValueError):
            proc.sampling_step(torch.zeros(1, 3, 8, 8), torch.tensor([bad]))
    with pytest.raises(ValueError):
        proc.decode(torch.zeros(1, 3, 8, 8), start=proc.n_steps + 1)
    with pytest.raises(TypeError):
        dmme_amd.ClassifierFreeDPMSolver(torch.nn.Identity(), 100, 5)


def test_clip_keeps_every_x0_inside_the_unit_box():
    """a restated chain on inputs scaled x3: with clip every x0 prediction lies in [-1, 1]; without it they do not"""
    abar = R.alpha_bar(100)
    g = R.grid(abar, 5, "logsnr")
    model = R.gaussian_predictor(abar)
    x = 3.0 * torch.from_numpy(np.random.RandomState(5).standard_normal(4096))
    for dtype in (torch.float64, torch.float32):
        clipped, free = [], []
        out = R.decode(model, x, abar, g, clip=True, dtype=dtype, x0s=clipped)[0]
        R.decode(model, x, abar, g, clip=False, dtype=dtype, x0s=free)
        assert len(clipped) == 5 and all(float(v.abs().max()) <= 1.0 for v in clipped) and float(out.abs().max()) <= 1.0
        assert max(float(v.abs().max()) for v in free) > 1.0


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    assert lib.dmme_version() >= 111
    p, row = C.c_void_p(16), (C.c_float * 8)()
    assert lib.dmme_dpmpp_step(p, p, None, row, 0, 1, 4, 1, None) == -1 and b"dpmpp_step" in lib.dmme_last_error()
    assert lib.dmme_dpmpp_step(p, p, p, row, 0, 1, 4, 3, None) == -1 and b"planes" in lib.dmme_last_error()
    assert lib.dmme_dpmpp_step(p, p, p, row, 0, 1, 6, 1, None) == -2 and b"multiple of 4" in lib.dmme_last_error()
    assert lib.dmme_chain_update_dpmpp(p, p, p, None, p, p, 1, 4, 1, None) == -1 and b"chain_update_dpmpp" in lib.dmme_last_error()
    assert lib.dmme_cfg_dpmpp_step(p, p, p, None, 0, 1, 4, None) == -1 and b"cfg_dpmpp_step" in lib.dmme_last_error()
    assert lib.dmme_chain_update_cfg_dpmpp(p, p, p, p, p, None, 1, 4, None) == -1 and b"chain_update_cfg_dpmpp" in lib.dmme_last_error()
    assert lib.dmme_dpmpp_chain_step(None, p, p, p, p, p, p, p, p, None) == -1 and b"dpmpp_chain_step" in lib.dmme_last_error()
    assert lib.dmme_cfg_dpmpp_chain_step(None, p, p, p, p, p, None, p, p, p, p, None) == -1 and b"cfg_dpmpp_chain_step" in lib.dmme_last_error()
    # the 4-wide kinds' entry points keep refusing the new kinds, with the messages they had
    assert lib.dmme_chain_update(8, p, p, p, p, p, 1, 4, None) == -1 and b"unknown sampler kind 8" in lib.dmme_last_error()
    assert lib.dmme_chain_update_cfg(9, p, p, None, p, p, p, 1, 4, None) == -1 and b"kind 9 is not a classifier-free kind (6, 7)" in lib.dmme_last_error()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "ddim", "iddpm", "cfg")}


@pytest.mark.parametrize("argv,msg", [
    (["fit", "--config", CFG["ddpm"], "--sampler", "dpm++"], "belongs to `sample`"),
    (["sample", "--config", CFG["ddim"], "--sampler", "dpm++", "--eta", "0.5"], "--eta"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "dpm++", "--steps", "3"], "--steps"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "dpm++", "--sample-steps", "0"], "--sample-steps"),
    (["sample", "--config", CFG["ddim"], "--solver-order", "1"], "--solver-order belongs to --sampler dpm++"),
    (["sample", "--config", CFG["ddim"], "--sampler", "ddim-paper", "--tau-schedule", "logsnr", "--clip-x0"], "--tau-schedule, --clip-x0 belong to"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


@pytest.mark.parametrize("argv,flag", [
    (["sample", "--config", CFG["ddpm"], "--sampler", "dpm++", "--solver-order", "3"], "--solver-order"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "dpm++", "--tau-schedule", "cosine"], "--tau-schedule"),
])
def test_trainer_parser_rejects_unknown_values(argv, flag, capsys):
    """the parser knows `--sampler dpm++` and names the new flag whose value it refuses"""
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert exc.value.code == 2 and f"argument {flag}: invalid choice" in capsys.readouterr().err


def test_trainer_builds_the_solver_for_every_config():
    """what `sample --sampler dpm++` puts in place of the YAML's process, built on the host: the network and the noise schedule of the
    config's own process, the flags' values, and the classifier-free form with the config's guidance scale for the cfg config"""
    import argparse

    from dmme_amd import trainer

    args = argparse.Namespace(sample_steps=None, tau_schedule=None, solver_order=None, clip_x0=False)
    for name, path in CFG.items():
        module = trainer._instantiate(trainer.parse_config(path)["model_spec"])
        old = module.diffusion_model
        new = trainer._dpm_solver(module, args)
        assert isinstance(new, dmme_amd.ClassifierFreeDPMSolver if name == "cfg" else dmme_amd.DPMSolverPP), name
        assert new.model is old.model and torch.equal(new.alpha_bar, old.alpha_bar) and new.sub_timesteps == 20 and new.order == 2 and new.tau_schedule == "logsnr"
        if name == "cfg":
            assert new.guidance_scale == old.guidance_scale and new.p_uncond == old.p_uncond
    args = argparse.Namespace(sample_steps=7, tau_schedule="quadratic", solver_order=1, clip_x0=True)
    new = trainer._dpm_solver(module, args)
    assert (new.sub_timesteps, new.tau_schedule, new.order, new.clip_x0) == (7, "quadratic", 1, True)
