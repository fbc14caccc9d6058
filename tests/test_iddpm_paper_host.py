"""Host-only checks of Improved DDPM as published (strided sampling, the loss-second-moment resampler's state, the runner's
--sample-steps): the timestep spacing and the respaced coefficient rows against the float64 restatement (tests/iddpm_paper_ref.py), the
state_dict contract of `t_sampler`, the YAML route to it, and the argument checks of the new C entry points (no GPU touched)."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib, trainer
from dmme_amd.equations.iddpm import respaced_coefficients, space_timesteps
from dmme_amd.models import iddpm as iddpm_models

from . import iddpm_paper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_KEYS = {"_ts_hist", "_ts_count"}


def _tiny_net():
    return iddpm_models.UNet(3, 4, 8, 2, 0.0, (4, 8), 1, (2,))


def test_space_timesteps_rounds_half_to_even_and_keeps_both_ends():
    assert space_timesteps(100, 7) == [1, 17, 34, 51, 67, 83, 100]  # 16.5 -> 16, 49.5 -> 50, 82.5 -> 82
    for T in (2, 5, 100):
        assert space_timesteps(T, T) == list(range(1, T + 1))
    for T in (2, 3, 10, 64, 100, 1000, 4000):
        for K in sorted({2, 3, 4, 7, 10, 50, 99, 100, T // 2, T - 1, T}):
            if 2 <= K <= T:
                s = space_timesteps(T, K)
                assert s == R.space_timesteps(T, K) and len(s) == K and s[0] == 1 and s[-1] == T
                assert all(b > a for a, b in zip(s, s[1:])), (T, K)
    for T, K in ((100, 1), (100, 101), (100, 0)):
        with pytest.raises(ValueError):
            space_timesteps(T, K)


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("T,K", [(100, 7), (4000, 50)])
def test_respaced_rows_equal_the_float64_rows_rounded_once(schedule, T, K):
    """each value is computed in float64 and rounded once to fp32 (6e-8): rel 1e-6 leaves an order of magnitude of margin"""
    proc = dmme_amd.IDDPM(torch.nn.Identity(), T, schedule=schedule)
    steps = space_timesteps(T, K)
    got = respaced_coefficients(proc.alpha_bar, steps)
    assert got.dtype == torch.float32 and tuple(got.shape) == (K + 1, 4) and bool((got[0] == 0).all())
    want = R.respaced_rows(proc.alpha_bar.reshape(-1).double().numpy(), steps)
    np.testing.assert_allclose(got.double().numpy()[1:], want[1:], rtol=1e-6, atol=0)
    n, rows, ttab = proc._respaced_tables(K)
    assert n == K and ttab == [0] + steps and len(rows) == K + 1
    assert np.array_equal(np.array(rows, dtype=np.float64), got.double().numpy())  # fp32 values held exactly in python floats
    assert rows[1][3] == float(np.float32(np.log(1e-12)))  # beta~'_1 = 0: the clamp


def test_respaced_betas_multiply_back_to_alpha_bar_T():
    """prod_k (1 - beta'_k) = abar_T on the linear schedule (no clip acts there), float64, to 1e-12"""
    for T, K in ((100, 7), (4000, 50)):
        proc = dmme_amd.IDDPM(torch.nn.Identity(), T, schedule="linear")
        abar = proc.alpha_bar.reshape(-1).double().numpy()
        steps = space_timesteps(T, K)
        beta = R.respaced_betas(abar, steps)
        assert beta.max() < 0.999
        assert abs(np.prod(1.0 - beta) / abar[T] - 1.0) <= 1e-12
        rows = respaced_coefficients(proc.alpha_bar, steps).double().numpy()
        np.testing.assert_allclose(np.exp(rows[1:, 2]), beta, rtol=2e-6)  # the rows carry the same betas (|log beta| <= 10, rounded to fp32: 6e-7)


def test_t_sampler_keyword_and_state_dict_contract(tmp_path):
    from dmme_amd.checkpoint import load_checkpoint, save_checkpoint

    with pytest.raises(ValueError, match="t_sampler"):
        dmme_amd.IDDPM(torch.nn.Identity(), 8, t_sampler="importance")
    torch.manual_seed(0)
    plain = dmme_amd.IDDPM(_tiny_net(), 8)
    uni = dmme_amd.IDDPM(_tiny_net(), 8, t_sampler="uniform")
    lsm = dmme_amd.IDDPM(_tiny_net(), 8, "vlb", 0.001, "cosine", 0.008, 0.0001, 0.02, "loss-second-moment")  # the keyword is last
    assert list(plain.state_dict()) == list(uni.state_dict())
    assert set(lsm.state_dict()) - set(plain.state_dict()) == TS_KEYS and set(plain.state_dict()) <= set(lsm.state_dict())
    assert tuple(lsm._ts_hist.shape) == (9, 10) and lsm._ts_hist.dtype == torch.float32
    assert tuple(lsm._ts_count.shape) == (9,) and lsm._ts_count.dtype == torch.int32
    lit_plain = dmme_amd.LitIDDPM(model=_tiny_net(), timesteps=8)
    lit_uni = dmme_amd.LitIDDPM(model=_tiny_net(), timesteps=8, t_sampler="uniform")
    lit_lsm = dmme_amd.LitIDDPM(model=_tiny_net(), timesteps=8, t_sampler="loss-second-moment")
    assert list(lit_plain.state_dict()) == list(lit_uni.state_dict())
    assert set(lit_lsm.state_dict()) - set(lit_plain.state_dict()) == {"diffusion_model." + k for k in TS_KEYS}
    # save -> load_checkpoint on the CPU restores the two buffers bit for bit
    rng = np.random.RandomState(3)
    lit_lsm.diffusion_model._ts_hist.copy_(torch.from_numpy(np.exp(1.5 * rng.standard_normal((9, 10))).astype(np.float32)))
    lit_lsm.diffusion_model._ts_count.copy_(torch.from_numpy(rng.randint(0, 11, size=9).astype(np.int32)))
    path = str(tmp_path / "lsm.ckpt")
    save_checkpoint(path, lit_lsm)
    fresh = dmme_amd.LitIDDPM(model=_tiny_net(), timesteps=8, t_sampler="loss-second-moment")
    assert not torch.equal(fresh.diffusion_model._ts_hist, lit_lsm.diffusion_model._ts_hist)
    load_checkpoint(path, fresh)
    for k in TS_KEYS:
        a, b = getattr(fresh.diffusion_model, k), getattr(lit_lsm.diffusion_model, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k
    with pytest.raises(ValueError, match="weights"):
        uni.training_step(torch.zeros(1, 3, 8, 8), weight=torch.ones(1))
    with pytest.raises(RuntimeError, match="loss-second-moment"):
        uni.draw_timesteps(4)


def test_yaml_t_sampler_reaches_the_constructor(tmp_path):
    path = tmp_path / "iddpm.yaml"
    path.write_text(
        "model:\n  class_path: dmme.LitIDDPM\n  init_args:\n    timesteps: 16\n    loss_type: vlb\n    t_sampler: loss-second-moment\n"
        "    model:\n      class_path: dmme.models.iddpm.UNet\n      init_args:\n        pos_dim: 4\n        emb_dim: 8\n        num_groups: 2\n"
        "        channels_per_depth: [4, 8]\n        num_blocks: 1\n        attention_depths: [2]\n"
    )
    module = trainer.build_module(trainer.parse_config(str(path)))
    idd = module.diffusion_model
    assert isinstance(module, dmme_amd.LitIDDPM) and idd.t_sampler == "loss-second-moment" and idd.loss_type == "vlb"
    assert tuple(idd._ts_hist.shape) == (17, 10)
    # the reference's own YAML (no such key) still builds the uniform sampler with no extra state
    module = trainer.build_module(trainer.parse_config(os.path.join(ROOT, "configs", "iddpm", "cifar10.yaml")))
    assert module.diffusion_model.t_sampler == "uniform" and not any("_ts_" in k for k in module.state_dict())


def test_sample_steps_needs_an_improved_ddpm_config():
    for cfg in ("ddpm", "ddim"):
        with pytest.raises(SystemExit, match="--sample-steps needs an Improved DDPM config"):
            trainer.main(["sample", "--config", os.path.join(ROOT, "configs", cfg, "cifar10.yaml"), "--sample-steps", "7"])
    with pytest.raises(SystemExit, match="belongs to `sample`"):
        trainer.main(["fit", "--config", os.path.join(ROOT, "configs", "iddpm", "cifar10.yaml"), "--sample-steps", "7"])


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    assert lib.dmme_version() >= 109
    p = C.c_void_p(16)
    rows = lambda **kw: lib.dmme_iddpm_loss_rows(*[kw.get(k, d) for k, d in (
        ("model_out", p), ("x_t", p), ("x_0", p), ("target", p), ("t", p), ("coef", p), ("T", 10), ("weight", None), ("B", 2), ("chw", 75),
        ("w_simple", 1.0), ("w_vlb", 1.0), ("loss", p), ("rows", p), ("d_out", None), ("grad_scale", 1.0), ("status", None), ("scratch", p),
        ("stream", None))])
    for bad in (dict(B=0), dict(chw=0), dict(T=0), dict(model_out=None), dict(t=None), dict(coef=None), dict(loss=None), dict(rows=None),
                dict(scratch=None)):
        assert rows(**bad) == -1 and b"iddpm_loss_rows" in lib.dmme_last_error(), bad
    assert lib.dmme_iddpm_prior_rows(None, 1, 16, 0.5, p, None) == -1 and b"iddpm_prior_rows" in lib.dmme_last_error()
    assert lib.dmme_iddpm_prior_rows(p, 0, 16, 0.5, p, None) == -1
    assert lib.dmme_iddpm_prior_rows(p, 1, 0, 0.5, p, None) == -1
    assert lib.dmme_iddpm_prior_rows(p, 1, 16, 1.0, p, None) == -1 and b"alpha_bar_T" in lib.dmme_last_error()
    draw = lambda hist=p, count=p, T=8, H=10, u0=0.001, B=4, t=p, w=p, pp=p: lib.dmme_tsampler_draw(hist, count, T, H, u0, 1, 0, B, t, w, pp, None)
    for bad in (dict(hist=None), dict(count=None), dict(T=0), dict(H=0), dict(B=0), dict(t=None), dict(w=None), dict(pp=None), dict(u0=1.5)):
        assert draw(**bad) == -1 and b"tsampler_draw" in lib.dmme_last_error(), bad
    assert draw(T=1 << 20) == -2  # the prefix sums would not fit in LDS: unsupported, said so
    upd = lambda hist=p, count=p, T=8, H=10, t=p, L=p, B=4: lib.dmme_tsampler_update(hist, count, T, H, t, L, B, None, None)
    for bad in (dict(hist=None), dict(count=None), dict(T=0), dict(H=0), dict(t=None), dict(L=None), dict(B=0)):
        assert upd(**bad) == -1 and b"tsampler_update" in lib.dmme_last_error(), bad
