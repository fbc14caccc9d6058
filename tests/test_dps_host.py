"""CPU: the host side of DPS (dmme_amd.DPS) - the rows against their float64 formulas, the operator presets, the adjoint identity, the
derived bounds of tests/dps_ref.py around a plain fp32 evaluation (the reference alone stays inside them), the header and the bindings,
the C argument checks that need no GPU, the process's own refusals and the trainer's."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from dmme_amd.diffusion_models.dpm_solver import solver_grid
from dmme_amd.diffusion_models.ilvr import resize_matrix

from . import dps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = [((2, 3, 8, 8), "identity", {}), ((2, 3, 12, 20), "average", dict(scale=4)), ((1, 3, 32, 32), "bicubic", dict(scale=4)),
       ((1, 3, 64, 64), "blur", dict(size=9, sigma=2.0))]


def _randn(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _binary(shape, seed, p=0.7):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < p).float()


# ------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("T,n,zeta", [(100, 8, 1.0), (1000, 1000, 0.3), (1000, 37, 0.0)])
def test_rows_match_their_float64_formulas(T, n, zeta):
    proc = dmme_amd.DPS(torch.nn.Identity(), T, n, zeta=zeta)
    ab = proc.alpha_bar.reshape(-1).double().numpy()
    grid = solver_grid(ab, n, "linear")
    assert grid == R.grid(ab, n) and proc._tau_host == grid
    rows64, ttab = dmme_amd.dps_rows(ab, grid, zeta)
    want, want_t = R.rows(ab, grid, zeta)
    assert ttab == want_t == grid and np.allclose(rows64, want, rtol=1e-15, atol=0.0)
    L, rows, tt = proc._chain_tables()
    assert L == len(grid) - 1 == proc.n_rows == proc.chain_length() and tt == grid
    assert np.array_equal(np.asarray(rows, dtype=np.float32), want.astype(np.float32))
    for a in range(1, L + 1):
        ab_a, ab_b = ab[grid[a]], ab[grid[a - 1]]
        alpha = ab_a / ab_b
        c0, c1, c2, At, Bt, z = rows64[a][:6]
        assert abs(c0 * np.sqrt(alpha) - 1) < 1e-14 and abs(c1 * np.sqrt(1 - ab_a) - (1 - alpha)) < 1e-14 and z == zeta
        assert (c2 == 0.0) if a == 1 else abs(c2 ** 2 - (1 - alpha)) < 1e-14  # sigma^2 = 1 - alpha; the last row adds no noise
        assert abs(At ** 2 * ab_a - 1) < 1e-13 and abs(Bt ** 2 * ab_a - (1 - ab_a)) < 1e-13
    assert tuple(rows64[0]) == (1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    from dmme_amd.diffusion_models.chain import chain_draws

    assert chain_draws(_lib.CHAIN_DPS, rows) == (L > 1)


# ------------------------------------------------------------------------------------------ presets
def test_presets():
    S = dmme_amd.SeparableOperator
    eye = S.identity(8, 12)
    assert np.array_equal(eye.Kh, np.eye(8)) and np.array_equal(eye.Kw, np.eye(12)) and (eye.h, eye.H, eye.w, eye.W) == (8, 8, 12, 12)
    bic = S.bicubic(32, 64, 4)
    assert np.array_equal(bic.Kh, resize_matrix(32, 8)) and np.array_equal(bic.Kw, resize_matrix(64, 16)) and (bic.h, bic.w) == (8, 16)
    blur = S.gaussian_blur(64, 32, 9, 2.0)
    avg = S.average(12, 20, 4)
    for op in (eye, bic, blur, avg):
        for K in (op.Kh, op.Kw):
            assert K.dtype == np.float64 and np.allclose(K.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    # the band: 9 taps inside, clipped and renormalised at the border, symmetric weights
    assert np.count_nonzero(blur.Kh[30]) == 9 and np.count_nonzero(blur.Kh[0]) == 5 and np.count_nonzero(blur.Kh[63]) == 5
    assert np.allclose(blur.Kh[30, 26:35], blur.Kh[30, 26:35][::-1]) and abs(blur.Kh[30, 31] / blur.Kh[30, 30] - np.exp(-0.125)) < 1e-14
    assert np.array_equal(avg.Kh, np.kron(np.eye(3), np.full((1, 4), 0.25)))
    # against the restatement's own builders
    for shape, name, kw in OPS:
        op = S.preset(name, shape[2], shape[3], blur_size=kw.get("size", 9), blur_sigma=kw.get("sigma", 2.0), scale=kw.get("scale", 4))
        Kh, Kw = R.operator(name, shape[2], shape[3], **kw)
        assert np.allclose(op.Kh, Kh.numpy(), rtol=0, atol=1e-15) and np.allclose(op.Kw, Kw.numpy(), rtol=0, atol=1e-15), name
        kh32, kw32 = op.device("cpu")
        assert kh32.dtype == torch.float32 and np.array_equal(kh32.numpy(), op.Kh.astype(np.float32)) and op.device("cpu")[0] is kh32
    for bad in (lambda: S.bicubic(32, 32, 5), lambda: S.average(30, 32, 4), lambda: S.gaussian_blur(32, 32, 4, 1.0), lambda: S.gaussian_blur(32, 32, 5, 0.0),
                lambda: S.preset("motion", 32, 32), lambda: S(np.ones((9, 8)), np.eye(8)), lambda: S.identity(0, 8)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("shape,name,kw", OPS)
def test_adjoint_identity(shape, name, kw):
    """<A x, r> = <x, A^T r> in float64, with a mask (A^T takes r already masked)"""
    Kh, Kw = R.operator(name, shape[2], shape[3], **kw)
    x = _randn(1, shape).double()
    ms = (shape[0], shape[1], Kh.shape[0], Kw.shape[0])
    m = _binary(ms, 2).double()
    r = _randn(3, ms).double() * m
    lhs, rhs = float((R.A(x, Kh, Kw, m) * r).sum()), float((x * R.At(r, Kh, Kw)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


# ------------------------------------------------------------------------------------------ the bounds hold a plain fp32 evaluation
@pytest.mark.parametrize("shape,name,kw", OPS)
def test_fp32_evaluation_sits_inside_the_bounds(shape, name, kw):
    Kh, Kw = (R.rounded(K) for K in R.operator(name, shape[2], shape[3], **kw))
    row = dmme_amd.DPS(torch.nn.Identity(), 100, 10)._chain_tables()[1][6]
    x, e = _randn(1, shape), _randn(2, shape)
    ms = (shape[0], shape[1], Kh.shape[0], Kw.shape[0])
    m, y = _binary(ms, 5), 0.5 * _randn(3, ms)
    big = 3.0 * x + 0.7
    err = (R.A(big, Kh, Kw).double() - R.A(big.double(), Kh, Kw)).abs()
    bound = R.measure_bound(big, Kh, Kw)
    print(f"measure {name}: fp32 torch largest err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()) and float(bound.max()) < 1e-4
    g32, d32, ss32, _ = R.adjoint(x, e, y, m, Kh, Kw, row, torch.float32)
    g64, d64, ss64, r64 = R.adjoint(x, e, y, m, Kh, Kw, row, torch.float64)
    bg, bss = R.adjoint_bound(x, e, y, m, Kh, Kw, row)
    eg, ess = (g32.double() - g64).abs(), (ss32.double() - ss64).abs()
    print(f"adjoint {name}: fp32 torch g largest err / bound {float((eg / bg.clamp_min(1e-300)).max()):.3f}, sumsq {float((ess / bss.clamp_min(1e-300)).max()):.3f}")
    assert bool((eg <= bg).all()) and bool((ess <= bss).all())
    assert float(bg.max()) < 1e-4 * max(float(g64.abs().max()), 1.0) and bool((bss <= 1e-3 * ss64.clamp_min(1e-3)).all())  # (the bounds mean something: a sum of 64 x 64 squares in any order alone is 4098 x 2^-24 = 2.4e-4)
    assert bool((r64[m.expand_as(r64) == 0] == 0).all())


@pytest.mark.parametrize("which", ["interior", "last"])
def test_fp32_update_sits_inside_its_bound(which):
    rows = dmme_amd.DPS(torch.nn.Identity(), 100, 10, zeta=0.7)._chain_tables()[1]
    row = rows[7] if which == "interior" else rows[1]
    shape = (2, 3, 32, 32)
    x, e, g, dx, z = (_randn(10 + k, shape) for k in range(5))
    ss = torch.tensor([[0.5, 1.25, 2.0], [0.0, 0.0, 0.0]])
    got = R.update(x, e, g, dx, ss, z, row, torch.float32)
    want = R.update(x, e, g, dx, ss, z, row, torch.float64)
    bound = R.update_bound(x, e, g, dx, ss, z, row)
    err = (got.double() - want).abs()
    print(f"update {which}: fp32 torch largest err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()) and float(bound.max()) < 1e-4
    u = R.update(x, e, g, dx, torch.zeros(2, 3), z, row, torch.float64)
    assert torch.equal(want[1], u[1]) and not torch.equal(want[0], u[0])  # (a zero norm skips the correction)
    row0 = list(row)
    row0[5] = 0.0
    assert torch.equal(R.update(x, e, g * float("nan"), dx, ss, z, row0, torch.float64), u)


# ------------------------------------------------------------------------------------------ the header, the binding, the C argument checks
def test_header_and_version():
    with open(os.path.join(ROOT, "include", "dmme_hip.h")) as f:
        text = f.read()
    assert "DMME_CHAIN_DPS = 13" in text and _lib.CHAIN_DPS == 13
    for sym in ("dmme_dps_capacity", "dmme_dps_measure", "dmme_dps_adjoint", "dmme_chain_adjoint_dps", "dmme_dps_step", "dmme_chain_update_dps",
                "dmme_dps_chain_step"):
        assert f"DMME_API int {sym}(" in text and sym in _lib.PROTOTYPES
    for word in ("{c0 = 1/sqrt(alpha), c1 = (1 - alpha)/sqrt(1 - abar_a), c2 = sqrt(1 - alpha) (0 where b = 0),", "x' = u + (zeta / n_b)((A_t g) - dx)",
                 "one keep-forward plus one input-backward per step"):
        assert word in text, word
    lib = _lib.lib()
    assert lib.dmme_version() >= 120
    assert lib.dmme_dps_capacity() >= 64 * 64


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p, row = C.c_void_p(16), (C.c_float * 8)(1.0, 0.1, 0.2, 1.5, 1.1, 1.0, 0.0, 0.0)
    err = lib.dmme_last_error
    # the measurement: x, Kh, Kw, mask, y_out, B, C, H, W, h, w, stream
    assert lib.dmme_dps_measure(None, p, p, None, p, 1, 3, 8, 8, 8, 8, None) == -1 and b"dps_measure" in err()
    assert lib.dmme_dps_measure(p, None, p, None, p, 1, 3, 8, 8, 8, 8, None) == -1 and b"dps_measure" in err()
    assert lib.dmme_dps_measure(p, p, p, None, None, 1, 3, 8, 8, 8, 8, None) == -1 and b"dps_measure" in err()
    assert lib.dmme_dps_measure(p, p, p, None, p, 0, 3, 8, 8, 8, 8, None) == -1 and b"dps_measure" in err()
    assert lib.dmme_dps_measure(p, p, p, None, p, 1, 3, 8, 8, 9, 8, None) == -1 and b"h <= H" in err()
    assert lib.dmme_dps_measure(p, p, p, None, p, 1, 3, 8, 8, 8, 12, None) == -1 and b"w <= W" in err()
    assert lib.dmme_dps_measure(p, p, p, None, p, 1, 3, 6, 6, 6, 6, None) == -2 and b"multiples of 4" in err()
    cap = lib.dmme_dps_capacity()
    assert lib.dmme_dps_measure(p, p, p, None, p, 1, 3, 64, 128, 16, 32, None) == -2 and str(cap).encode() in err() and 64 * 128 > cap
    assert lib.dmme_dps_measure(p, p, p, None, p, 1, 3, 1024, 4, 1024, 4, None) == -2 and b"dmme_dps_capacity" in err()  # (fits the capacity, not the LDS: Kh is 1024 x 1025)
    # the adjoint: x, model_out, planes, row, y, mask, Kh, Kw, g, d_out, sumsq, B, C, H, W, h, w, stream
    adj = lambda *a: lib.dmme_dps_adjoint(*a)
    assert adj(None, p, 1, row, p, p, p, p, p, p, p, 1, 3, 8, 8, 8, 8, None) == -1 and b"dps_adjoint" in err()
    assert adj(p, p, 1, None, p, p, p, p, p, p, p, 1, 3, 8, 8, 8, 8, None) == -1 and b"dps_adjoint" in err()
    assert adj(p, p, 1, row, p, p, p, p, p, p, None, 1, 3, 8, 8, 8, 8, None) == -1 and b"dps_adjoint" in err()
    assert adj(p, p, 3, row, p, p, p, p, p, p, p, 1, 3, 8, 8, 8, 8, None) == -1 and b"planes" in err()
    assert adj(p, p, 1, row, p, p, p, p, p, p, p, 1, 3, 8, 8, 12, 8, None) == -1 and b"h <= H" in err()
    assert adj(p, p, 1, row, p, p, p, p, p, p, p, 1, 3, 64, 128, 64, 128, None) == -2 and b"dmme_dps_capacity" in err()
    assert lib.dmme_chain_adjoint_dps(p, p, 1, None, p, p, p, p, p, p, p, p, 1, 3, 8, 8, 8, 8, None) == -1 and b"chain_adjoint_dps" in err()
    assert lib.dmme_chain_adjoint_dps(p, p, 1, p, None, p, p, p, p, p, p, p, 1, 3, 8, 8, 8, 8, None) == -1 and b"chain_adjoint_dps" in err()
    assert lib.dmme_chain_adjoint_dps(p, p, 1, p, p, p, p, p, p, p, p, p, 1, 3, 8, 6, 8, 6, None) == -2 and b"multiples of 4" in err()
    # the eager update: x, model_out, g, dx, sumsq, z, row, B, C, H, W, planes, stream
    assert lib.dmme_dps_step(None, p, p, p, p, p, row, 1, 3, 8, 8, 1, None) == -1 and b"dps_step" in err()
    assert lib.dmme_dps_step(p, p, p, p, p, p, None, 1, 3, 8, 8, 1, None) == -1 and b"dps_step" in err()
    assert lib.dmme_dps_step(p, p, p, p, p, None, row, 1, 3, 8, 8, 1, None) == -1 and b"needs z" in err()
    assert lib.dmme_dps_step(p, p, None, p, p, p, row, 1, 3, 8, 8, 1, None) == -1 and b"needs g, dx and sumsq" in err()
    assert lib.dmme_dps_step(p, p, p, p, p, p, row, 1, 3, 8, 8, 0, None) == -1 and b"planes" in err()
    assert lib.dmme_dps_step(p, p, p, p, p, p, row, 1, 3, 5, 5, 1, None) == -2 and b"multiple of 4" in err()
    # the chain update: x, model_out, g, dx, sumsq, noise, step_coef, t_table, state, B, C, H, W, planes, stream
    assert lib.dmme_chain_update_dps(p, p, p, p, p, None, None, p, p, 1, 3, 8, 8, 1, None) == -1 and b"chain_update_dps" in err()
    assert lib.dmme_chain_update_dps(p, p, p, p, p, None, p, p, None, 1, 3, 8, 8, 1, None) == -1 and b"chain_update_dps" in err()
    assert lib.dmme_chain_update_dps(p, p, None, p, p, None, p, p, p, 1, 3, 8, 8, 1, None) == -1 and b"chain_update_dps" in err()
    assert lib.dmme_chain_update_dps(p, p, p, p, p, None, p, p, p, 1, 3, 5, 5, 1, None) == -2 and b"multiple of 4" in err()
    # the capturable step: a null plan
    assert lib.dmme_dps_chain_step(None, p, p, p, p, p, p, p, p, p, p, 8, 8, p, p, p, p, p, p, p, None) == -1 and b"dps_chain_step" in err()
    # the entry points of the table's kinds refuse the new kind
    assert lib.dmme_chain_update(13, p, p, p, p, p, 1, 4, None) == -1 and b"unknown sampler kind 13" in err()
    assert lib.dmme_chain_step(p, p, p, p, p, 13, p, p, p, None) == -1 and b"chain_step: sampler kind 13" in err()


# ------------------------------------------------------------------------------------------ the process
def test_process_refuses_what_is_not_built():
    net = torch.nn.Identity()
    for kw in (dict(prediction="v"), dict(prediction="x0"), dict(threshold="static"), dict(threshold="dynamic")):
        with pytest.raises(NotImplementedError):
            dmme_amd.DPS(net, 100, 8, **kw)
    for kw in (dict(zeta=-1.0), dict(sigma_y=float("nan")), dict(sub_timesteps=0), dict(sub_timesteps=101), dict(operator="blur")):
        with pytest.raises(ValueError):
            dmme_amd.DPS(net, 100, **{"sub_timesteps": 8, **kw})
    proc = dmme_amd.DPS(net, 100, 8, operator=dmme_amd.SeparableOperator.average(32, 32, 4))
    with pytest.raises(NotImplementedError):
        proc.set_threshold("static")
    assert proc.set_threshold("none") is proc
    with pytest.raises(ValueError):
        proc._operator_for(16, 16)
    with pytest.raises(ValueError):
        proc.restore(torch.zeros(1, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        proc.sampling_step(torch.zeros(1, 3, 8, 8), torch.tensor([3]))
    with pytest.raises(NotImplementedError):
        dmme_amd.DPS.from_process(dmme_amd.DDPM(net, 100, prediction="v"), sub_timesteps=8)
    base = dmme_amd.DDPM(net, 100)
    new = dmme_amd.DPS.from_process(base, sub_timesteps=8, zeta=0.5)
    assert torch.equal(new.alpha_bar, base.alpha_bar) and new.zeta == 0.5 and new.operator is None and new._operator_for(8, 12).name == "identity"
    assert dmme_amd.PosteriorChainRunner is dmme_amd.DPS._runner_class and dmme_amd.DPS._chain_kind == 13


# ------------------------------------------------------------------------------------------ the trainer
CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "ddim", "iddpm", "cfg", "vpred")}
MEAS = ["--measurement", "y.npy"]
DPS = ["sample", "--config", CFG["ddpm"], "--sampler", "dps"]


@pytest.mark.parametrize("argv,msg", [
    (DPS, "needs exactly one of --measurement"),
    (DPS + MEAS + ["--image", "x.npy"], "needs exactly one of --measurement"),
    (DPS + MEAS + ["--eta", "0.5"], "--eta does not go with --sampler dps"),
    (DPS + MEAS + ["--steps", "3"], "--steps does not go with --sampler dps"),
    (DPS + MEAS + ["--labels", "3"], "--labels does not go with --sampler dps"),
    (DPS + MEAS + ["--strength", "0.5"], "--strength does not go with --sampler dps"),
    (DPS + MEAS + ["--jump-length", "2"], "--jump-length does not go with --sampler dps"),
    (DPS + MEAS + ["--prediction", "v"], "--prediction v does not go with --sampler dps"),
    (DPS + MEAS + ["--threshold", "static"], "--threshold static does not go with --sampler dps"),
    (DPS + MEAS + ["--down-factor", "4"], "--down-factor belongs to --sampler ilvr"),
    (DPS + MEAS + ["--sr-scale", "4"], "--sr-scale belongs to --sampler ddnm"),
    (DPS + MEAS + ["--gray"], "--gray belongs to --sampler ddnm"),
    (DPS + MEAS + ["--blur-size", "5"], "--blur-size / --blur-sigma belong to --operator blur"),
    (DPS + MEAS + ["--operator", "blur", "--down-scale", "2"], "--down-scale belongs to --operator bicubic / average"),
    (DPS + MEAS + ["--operator", "blur", "--blur-size", "4"], "--blur-size must be an odd number"),
    (DPS + MEAS + ["--operator", "blur", "--blur-sigma", "0"], "--blur-sigma must be positive"),
    (DPS + MEAS + ["--operator", "average", "--down-scale", "0"], "--down-scale must be at least 1"),
    (DPS + MEAS + ["--zeta", "-1"], "--zeta must be at least 0"),
    (DPS + MEAS + ["--sigma-y", "-1"], "--sigma-y must be at least 0"),
    (DPS + MEAS + ["--sample-steps", "0"], "--sample-steps must be at least 1"),
    (["fit", "--config", CFG["ddpm"], "--sampler", "dps"] + MEAS, "belongs to `sample`"),
    (["sample", "--config", CFG["ddpm"], "--zeta", "1"], "--zeta belongs to --sampler dps"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "ddnm", "--measurement", "y.npy", "--operator", "blur", "--blur-size", "5"],
     "--operator, --blur-size belong to --sampler dps"),
    (DPS + ["--measurement", "/nonexistent/y.npy"], "--measurement /nonexistent/y.npy"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


def test_trainer_checks_the_inputs_against_the_operator(tmp_path):
    """a scale that does not divide the image, a mask of the image's resolution or with fractional values and the conditional config are
    refused before anything touches the GPU"""
    from dmme_amd import trainer

    img = tmp_path / "img.npy"
    np.save(img, np.zeros((3, 32, 32), dtype=np.float32))
    meas = tmp_path / "meas.npy"
    np.save(meas, np.zeros((3, 8, 8), dtype=np.float32))
    big_mask = tmp_path / "big.npy"
    np.save(big_mask, np.ones((1, 1, 32, 32), dtype=np.float32))
    soft = tmp_path / "soft.npy"
    np.save(soft, np.full((1, 1, 8, 8), 0.5, dtype=np.float32))
    for argv, msg in ((DPS + ["--image", str(img), "--operator", "bicubic", "--down-scale", "5"], "32 x 32 is not divisible by --down-scale 5"),
                      (DPS + ["--image", str(img), "--operator", "average", "--mask", str(big_mask)], "the mask is at measurement resolution"),
                      (DPS + ["--measurement", str(meas), "--operator", "average", "--mask", str(soft)], "values must be 0 or 1"),
                      (["sample", "--config", CFG["cfg"], "--sampler", "dps", "--measurement", str(meas)], "needs an unconditional config")):
        with pytest.raises(SystemExit) as exc:
            trainer.main(argv)
        assert msg in str(exc.value), exc.value


def test_trainer_builds_the_process_for_every_unconditional_config():
    """what `sample --sampler dps` puts in place of the YAML's process, built on the host: the config's network and noise schedule (the
    iddpm config's cosine table too), the flags' values and their defaults; a v-prediction config is refused"""
    import argparse

    from dmme_amd import trainer

    none = dict(sample_steps=None, operator=None, blur_size=None, blur_sigma=None, down_scale=None, zeta=None, sigma_y=None)
    for name in ("ddpm", "ddim", "iddpm"):
        module = trainer._instantiate(trainer.parse_config(CFG[name])["model_spec"])
        old = module.diffusion_model
        new = trainer._dps_process(module, argparse.Namespace(**none), 32, 32)
        assert isinstance(new, dmme_amd.DPS) and new.model is old.model and torch.equal(new.alpha_bar, old.alpha_bar), name
        assert (new.sub_timesteps, new.zeta, new.sigma_y, new.operator.name, new.chain_length()) == (100, 1.0, 0.0, "identity", 100)
    new = trainer._dps_process(module, argparse.Namespace(**{**none, "sample_steps": 12, "operator": "bicubic", "zeta": 0.4, "sigma_y": 0.05}), 32, 32)
    assert (new.sub_timesteps, new.zeta, new.sigma_y, new.operator.h, new.operator.w) == (12, 0.4, 0.05, 8, 8)
    new = trainer._dps_process(module, argparse.Namespace(**{**none, "operator": "blur", "blur_size": 5, "blur_sigma": 1.5}), 32, 32)
    assert np.array_equal(new.operator.Kh, dmme_amd.SeparableOperator.gaussian_blur(32, 32, 5, 1.5).Kh)
    module = trainer._instantiate(trainer.parse_config(CFG["vpred"])["model_spec"])
    with pytest.raises(SystemExit) as exc:
        trainer._dps_process(module, argparse.Namespace(**none), 32, 32)
    assert "adapter" in str(exc.value)
