"""Host-only checks of ILVR (dmme_amd.ILVR): the low-pass matrix against torch's antialiased bicubic resize in float64 and against the
restatement's (tests/ilvr_ref.py), the rows the package builds (RePaint's reverse half, the conditioning flag, the exact constants, DDPM's
scalars on the full grid), the bound the GPU test of the update relies on (the restatement in fp32 sits inside it), the header and the
binding, the argument checks of the new C entry points, of the constructor and of the trainer's new flags.  No GPU is touched."""

import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmme_amd
from dmme_amd import _lib

from . import ilvr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the filter
@pytest.mark.parametrize("H,W,N", [(8, 8, 2), (12, 20, 4), (32, 32, 8), (64, 64, 16)])
def test_lowpass_matrix_is_torchs_antialiased_bicubic_down_and_up(H, W, N):
    Ph, Pw = dmme_amd.lowpass_matrix(H, N), dmme_amd.lowpass_matrix(W, N)
    assert Ph.shape == (H, H) and Pw.shape == (W, W) and Ph.dtype == np.float64
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(H + W))
    down = F.interpolate(x, size=(H // N, W // N), mode="bicubic", antialias=True, align_corners=False)
    want = F.interpolate(down, size=(H, W), mode="bicubic", antialias=True, align_corners=False)
    got = torch.from_numpy(Ph) @ x @ torch.from_numpy(Pw).T
    err = float((got - want).abs().max())
    print(f"{H}x{W}/{N}: |P x P^T - interpolate| = {err:.2e}")
    assert err <= 1e-12
    for P, n in ((Ph, H), (Pw, W)):
        assert float(np.abs(P.sum(axis=1) - 1.0).max()) <= 1e-15
        assert float((torch.from_numpy(P) - R.lowpass_matrix(n, N)).abs().max()) <= 1e-14
    assert float(np.abs(Ph @ Ph - Ph).max()) > 1e-3  # not idempotent: nothing may assume phi(phi(x)) = phi(x)


def test_lowpass_matrix_of_the_whole_axis_is_an_averaging_matrix():
    """N = n: down to one pixel (a weighted mean of the whole axis, the stretched kernel's weights), up from it (that one value everywhere):
    every row of P is the same weight vector, symmetric, positive and of sum 1; and the filter of a constant is that constant"""
    for n in (4, 8, 32):
        P = dmme_amd.lowpass_matrix(n, n)
        assert np.array_equal(P, np.tile(P[:1], (n, 1))) and bool((P[0] > 0).all()) and abs(P[0].sum() - 1.0) <= 1e-15
        assert np.allclose(P[0], P[0][::-1], rtol=0, atol=1e-16)
        assert np.allclose(P @ np.full(n, 2.5), 2.5, rtol=0, atol=1e-14)


def test_lowpass_matrix_rejects_nonsense():
    for n, N in ((8, 3), (8, 1), (8, 0), (8, -2), (8, 16), (8, 2.5), (0, 2), (8, True)):
        with pytest.raises(ValueError):
            dmme_amd.lowpass_matrix(n, N)


# ------------------------------------------------------------------------------------------ the rows
@pytest.mark.parametrize("T,n,r", [(100, 100, 0), (100, 8, 0), (1000, 20, 5), (1000, 250, 30), (50, 7, 7)])
def test_rows(T, n, r):
    from dmme_amd.diffusion_models.repaint import repaint_rows

    proc = dmme_amd.ILVR(torch.nn.Identity(), T, n, 4, r)
    abar = R.alpha_bar(T)
    g = proc._tau_host
    assert g == R.grid(abar, n) and g[0] == 0 and g[-1] == T and [int(v) for v in proc.tau] == g
    L = len(g) - 1
    rows64, ttab = dmme_amd.ilvr_rows(abar, g, r)
    want, want_t = R.rows(abar, g, r)
    assert rows64.shape == (L + 1, 8) and rows64.dtype == np.float64 and ttab == want_t == g
    assert np.allclose(rows64, want, rtol=1e-12, atol=1e-12)
    # the reverse half is RePaint's on the plain walk over the same grid, to the bit
    paint, ptt = repaint_rows(abar, g, list(range(L, -1, -1)))
    assert ptt == ttab and np.array_equal(rows64[1:, :5], paint[1:, :5])
    for i in range(1, L + 1):
        b = i - 1
        assert rows64[i, 5] == (1.0 if b >= r else 0.0) and rows64[i, 6] == rows64[i, 7] == 0.0
        assert (rows64[i, 2] == 0.0) == (b == 0) and (rows64[i, 4] == 0.0) == (b == 0)
    assert rows64[1, 3] == 1.0
    assert sum(1 for i in range(1, L + 1) if rows64[i, 5] != 0.0) == max(0, L - r)
    # what the process keeps: the rows rounded to fp32; on the full grid DDPM's own scalars
    cnt, rows, tt = proc._chain_tables()
    assert cnt == L == proc.n_levels == proc.chain_length() and tt == ttab
    got = np.array(rows)
    if n == T:
        ddpm = dmme_amd.DDPM(torch.nn.Identity(), T)
        for i in range(1, L + 1):
            t = tt[i]
            assert rows[i][0] == ddpm._c1[t] and rows[i][1] == ddpm._c2[t] and rows[i][2] == (ddpm._sigma[t] if t > 1 else 0.0)
        assert np.array_equal(got[:, 3:], rows64.astype(np.float32).astype(np.float64)[:, 3:])
    else:
        assert np.array_equal(got, rows64.astype(np.float32).astype(np.float64))
    # `generate`: the same rows with g = 0 everywhere
    fn, frows, ftt = proc._free_tables
    assert fn == L and ftt == ttab and all(rw[5] == 0.0 for rw in frows) and all(a[:5] == b[:5] for a, b in zip(frows, rows))


def test_from_process_follows_an_iddpm_cosine_table():
    p = dmme_amd.IDDPM(torch.nn.Identity(), 100)
    s = dmme_amd.ILVR.from_process(p, sub_timesteps=10, down_factor=8, range_level=2)
    assert torch.equal(s.alpha_bar, p.alpha_bar) and s.timesteps == 100 and s.model is p.model and (s.down_factor, s.range_level) == (8, 2)
    ab = p.alpha_bar.reshape(-1).double().numpy()
    want, tt = R.rows(ab, R.grid(ab, 10), 2)
    n, rows, ttab = s._chain_tables()
    assert ttab == tt and n == 10 and np.allclose(np.array(rows), want.astype(np.float32).astype(np.float64), rtol=1e-6, atol=1e-12)


def test_python_surface_and_constructor_errors():
    for name in ("ILVR", "LikeChainRunner", "ilvr_rows", "lowpass_matrix"):
        assert name in dmme_amd.__all__ and hasattr(dmme_amd, name)
    from dmme_amd.diffusion_models.ddpm import ChainRunner, chain_draws

    assert issubclass(dmme_amd.ILVR, dmme_amd.DDPM) and issubclass(dmme_amd.LikeChainRunner, ChainRunner)
    proc = dmme_amd.ILVR(torch.nn.Identity(), 100, 10)
    assert proc._chain_kind == _lib.CHAIN_ILVR == 11 and proc._runner_class is dmme_amd.LikeChainRunner
    assert (proc.sub_timesteps, proc.down_factor, proc.range_level) == (10, 4, 0)
    assert chain_draws(_lib.CHAIN_ILVR, proc._chain_tables()[1]) is True
    for kw in (dict(down_factor=1), dict(down_factor=0), dict(down_factor=2.5), dict(down_factor=True), dict(range_level=-1), dict(range_level=11),
               dict(range_level=1.5), dict(sub_timesteps=0), dict(sub_timesteps=101), dict(sub_timesteps=2.5), dict(alpha_bar=torch.linspace(1, 0.1, 50)),
               dict(alpha_bar=torch.ones(101)), dict(prediction="nope"), dict(threshold="nope")):
        with pytest.raises(ValueError):
            dmme_amd.ILVR(torch.nn.Identity(), 100, **{"sub_timesteps": 10, **kw})
    # an image the filter does not divide, and something that is no image batch: refused on the host before any launch or draw
    with pytest.raises(ValueError, match="not divisible by down_factor"):
        proc.sample_like(torch.zeros(1, 3, 10, 8))
    with pytest.raises(ValueError, match="not divisible by down_factor"):
        proc.low_pass(torch.zeros(1, 3, 8, 6))
    with pytest.raises(ValueError):
        proc.sample_like(torch.zeros(3, 8, 8))
    with pytest.raises(NotImplementedError):
        proc.sampling_step(torch.zeros(1, 3, 8, 8), torch.tensor([3]))


# ------------------------------------------------------------------------------------------ the bound of the GPU test of the update
def _seq_fp32_filter(d, Ph32, Pw32):
    """Ph d Pw^T in float32 with sequential sums and separately rounded products (no fma): the plainest fp32 evaluation"""
    d = d.numpy().astype(np.float32)
    Ph, Pw = Ph32.numpy(), Pw32.numpy()
    T = np.zeros(d.shape, dtype=np.float32)
    for k in range(d.shape[-1]):
        T = (T + d[..., :, k:k + 1] * Pw[None, :, k]).astype(np.float32)
    Fo = np.zeros(d.shape, dtype=np.float32)
    for k in range(d.shape[-2]):
        Fo = (Fo + Ph[:, k:k + 1] * T[..., k:k + 1, :]).astype(np.float32)
    return torch.from_numpy(Fo)


@pytest.mark.parametrize("planes,H,W,N", [(6, 8, 8, 2), (6, 12, 20, 4), (3, 32, 32, 8), (3, 64, 64, 4)])
def test_the_filters_bound_holds_for_a_plain_fp32_evaluation(planes, H, W, N):
    """|err| <= (H + W + 8) 2^-24 (|Ph| |d| |Pw|^T): two chained fp32 dot products of lengths W and H over fp32-rounded tables.  A
    sequential fp32 evaluation without fma must sit inside it (it does, by a factor of 10 to 100), so the bound can be asked of the device"""
    g = torch.Generator().manual_seed(7)
    d = 3.0 * torch.randn(planes, H, W, generator=g) + 0.7
    Ph, Pw = (torch.from_numpy(dmme_amd.lowpass_matrix(n, N).astype(np.float32)) for n in (H, W))
    exact = Ph.double() @ d.double() @ Pw.double().T
    bound = R.filter_bound(d, Ph, Pw)
    ratio = float(((_seq_fp32_filter(d, Ph, Pw).double() - exact).abs() / bound).max())
    print(f"{planes}x{H}x{W}/{N}: sequential fp32 at {ratio:.3f} of the bound")
    assert ratio <= 1.0


@pytest.mark.parametrize("B,H,W,N", [(2, 8, 8, 2), (2, 12, 20, 4), (1, 32, 32, 8)])
def test_the_updates_bound_holds_for_the_restatement_in_fp32(B, H, W, N):
    """2^-24 [8 A + (H + W + 16) (|Ph| A |Pw|^T)] with A = |c0 x| + |c0 c1 e| + |c2 z0| + |ka y| + |ks z1|: a few roundings of u, k, d and the
    final sum (each at most 2^-24 of a value bounded by A, eight of them with room to spare), the filter's own bound with |d| <= A, and
    d's rounding (a few 2^-24 A) carried through |Ph| . |Pw|^T, which the 8 added to H + W + 8 covers.  tests/ilvr_ref.py in fp32 against
    itself in float64 on fp32 rows and tables must sit inside it before the device is asked to"""
    shape = (B, 3, H, W)
    g = torch.Generator().manual_seed(11)
    x, e, y = (torch.randn(shape, generator=g) for _ in range(3))
    z2 = torch.randn((2,) + shape, generator=g)
    rows = R.update_rows(N)
    Ph, Pw = (torch.from_numpy(dmme_amd.lowpass_matrix(n, N).astype(np.float32)).double() for n in (H, W))
    for i, row in rows.items():
        got = R.step(x, e, y, z2, row, Ph, Pw, torch.float32)
        want = R.step(x, e, y, z2, row, Ph, Pw, torch.float64)
        bound = R.update_bound(x, e, y, z2, row, Ph, Pw)
        ratio = float(((got.double() - want).abs() / bound).max())
        print(f"{shape}/{N} row {i}: the restatement in fp32 at {ratio:.3f} of the bound")
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------ the header, the binding, the C argument checks
def test_header_and_version():
    with open(os.path.join(ROOT, "include", "dmme_hip.h")) as f:
        text = f.read()
    assert "DMME_CHAIN_ILVR = 11" in text
    for sym in ("dmme_lowpass", "dmme_ilvr_step", "dmme_chain_update_ilvr", "dmme_ilvr_chain_step", "dmme_lowpass_lds_capacity"):
        assert f"DMME_API int {sym}(" in text and sym in _lib.PROTOTYPES
    assert "DMME_API int64_t dmme_lowpass_scratch_bytes(" in text and "dmme_lowpass_scratch_bytes" in _lib.PROTOTYPES
    lib = _lib.lib()
    assert lib.dmme_version() >= 116
    cap = lib.dmme_lowpass_lds_capacity()
    assert cap >= 64 * 64 and cap < 256 * 256  # 32 x 32 and 64 x 64 take the fused form, 256 x 256 the streaming one
    assert lib.dmme_lowpass_scratch_bytes(24, 256, 256) == 24 * 256 * 256 * 4 and lib.dmme_lowpass_scratch_bytes(0, 8, 8) == 0


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p, row = C.c_void_p(16), (C.c_float * 8)()
    err = lib.dmme_last_error
    # the filter: src, dst, planes, H, W, Ph, Pw, scratch, force_streaming, stream
    assert lib.dmme_lowpass(None, p, 1, 8, 8, p, p, None, 0, None) == -1 and b"lowpass" in err()
    assert lib.dmme_lowpass(p, p, 0, 8, 8, p, p, None, 0, None) == -1 and b"lowpass" in err()
    assert lib.dmme_lowpass(p, p, 1, 8, 8, None, p, None, 0, None) == -1 and b"null table" in err()
    assert lib.dmme_lowpass(p, p, 1, 8, 8, p, None, None, 0, None) == -1 and b"null table" in err()
    assert lib.dmme_lowpass(p, p, 1, 8, 6, p, p, None, 0, None) == -2 and b"width 6" in err()
    # the eager twin: x, model_out, ref, z2, row, Ph, Pw, scratch, B, C, H, W, planes, force_streaming, stream
    assert lib.dmme_ilvr_step(None, p, p, p, row, p, p, None, 1, 3, 8, 8, 1, 0, None) == -1 and b"ilvr_step" in err()
    assert lib.dmme_ilvr_step(p, p, None, p, row, p, p, None, 1, 3, 8, 8, 1, 0, None) == -1 and b"ilvr_step" in err()
    assert lib.dmme_ilvr_step(p, p, p, p, None, p, p, None, 1, 3, 8, 8, 1, 0, None) == -1 and b"ilvr_step" in err()
    assert lib.dmme_ilvr_step(p, p, p, p, row, None, p, None, 1, 3, 8, 8, 1, 0, None) == -1 and b"null table" in err()
    assert lib.dmme_ilvr_step(p, p, p, p, row, p, p, None, 1, 3, 8, 8, 3, 0, None) == -1 and b"planes" in err()
    assert lib.dmme_ilvr_step(p, p, p, p, row, p, p, None, 1, 3, 5, 5, 1, 0, None) == -2 and b"ilvr_step" in err() and b"multiple of 4" in err()
    drawing = (C.c_float * 8)(1.0, 0.0, 0.5, 1.0, 0.0, 0.0, 0.0, 0.0)
    assert lib.dmme_ilvr_step(p, p, p, None, drawing, p, p, None, 1, 3, 8, 8, 1, 0, None) == -1 and b"needs z" in err()
    noising = (C.c_float * 8)(1.0, 0.0, 0.0, 1.0, 0.5, 1.0, 0.0, 0.0)
    assert lib.dmme_ilvr_step(p, p, p, None, noising, p, p, None, 1, 3, 8, 8, 1, 0, None) == -1 and b"needs z" in err()
    # the chain form: x, model_out, ref, noise, Ph, Pw, scratch, step_coef, t_table, state, B, C, H, W, planes, force_streaming, stream
    assert lib.dmme_chain_update_ilvr(p, p, None, None, p, p, None, p, p, p, 1, 3, 8, 8, 1, 0, None) == -1 and b"chain_update_ilvr" in err()
    assert lib.dmme_chain_update_ilvr(p, p, p, None, p, p, None, None, p, p, 1, 3, 8, 8, 1, 0, None) == -1 and b"chain_update_ilvr" in err()
    assert lib.dmme_chain_update_ilvr(p, p, p, None, p, p, None, p, p, None, 1, 3, 8, 8, 1, 0, None) == -1 and b"chain_update_ilvr" in err()
    assert lib.dmme_chain_update_ilvr(p, p, p, None, p, p, None, p, p, p, 1, 3, 8, 8, 5, 0, None) == -1 and b"planes" in err()
    assert lib.dmme_chain_update_ilvr(p, p, p, None, p, p, None, p, p, p, 1, 3, 5, 5, 1, 0, None) == -2 and b"multiple of 4" in err()
    # the capturable step: a null plan
    assert lib.dmme_ilvr_chain_step(None, p, p, p, p, p, p, p, None, p, p, p, None) == -1 and b"ilvr_chain_step" in err()
    # the entry points of the table's kinds refuse the new kind
    assert lib.dmme_chain_update(11, p, p, p, p, p, 1, 4, None) == -1 and b"unknown sampler kind 11" in err()
    assert lib.dmme_chain_step(p, p, p, p, p, 11, p, p, p, None) == -1 and b"chain_step: sampler kind 11" in err()


# ------------------------------------------------------------------------------------------ the trainer
CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "ddim", "iddpm", "cfg")}
IMG = ["--image", "x.npy"]
ILVR = ["sample", "--config", CFG["ddpm"], "--sampler", "ilvr"]


@pytest.mark.parametrize("argv,msg", [
    (ILVR, "--sampler ilvr needs --image"),
    (ILVR + IMG + ["--mask", "m.npy"], "--mask belongs to --sampler repaint / sdedit"),
    (ILVR + IMG + ["--strength", "0.5"], "--strength belongs to --sampler repaint / sdedit"),
    (ILVR + IMG + ["--jump-length", "5"], "--jump-length belongs to --sampler repaint / sdedit"),
    (ILVR + IMG + ["--resamples", "5"], "--resamples belongs to --sampler repaint / sdedit"),
    (ILVR + IMG + ["--jump-length", "5", "--resamples", "2"], "--jump-length, --resamples belong to --sampler repaint / sdedit"),
    (ILVR + IMG + ["--down-factor", "1"], "--down-factor must be at least 2"),
    (ILVR + IMG + ["--range-level", "-1"], "--range-level must be at least 0"),
    (ILVR + IMG + ["--sample-steps", "0"], "--sample-steps must be at least 1"),
    (ILVR + IMG + ["--eta", "0.5"], "--eta does not go with --sampler ilvr"),
    (ILVR + IMG + ["--steps", "3"], "--steps does not go with --sampler ilvr"),
    (ILVR + IMG + ["--labels", "3"], "--labels does not go with --sampler ilvr"),
    (["fit", "--config", CFG["ddpm"], "--sampler", "ilvr"] + IMG, "belongs to `sample`"),
    (["sample", "--config", CFG["ddpm"], "--down-factor", "4"], "--down-factor belongs to --sampler ilvr"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint", "--range-level", "2", "--down-factor", "4"] + IMG, "--down-factor, --range-level belong to --sampler ilvr"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "ilvr", "--image", "/nonexistent/x.npy"], "--image /nonexistent/x.npy"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


def test_trainer_checks_the_image_against_the_down_factor(tmp_path):
    """an image size the filter does not divide, a conditional config and a bad file are refused before anything touches the GPU"""
    from dmme_amd import trainer

    img = tmp_path / "img.npy"
    np.save(img, np.zeros((3, 32, 32), dtype=np.float32))
    odd = tmp_path / "odd.npy"
    np.save(odd, np.zeros((2, 3, 30, 32), dtype=np.float32))
    for argv, msg in ((ILVR + ["--image", str(odd)], "30 x 32 is not divisible by --down-factor 4"),
                      (ILVR + ["--image", str(img), "--down-factor", "5"], "32 x 32 is not divisible by --down-factor 5"),
                      (["sample", "--config", CFG["cfg"], "--sampler", "ilvr", "--image", str(img)], "needs an unconditional config")):
        with pytest.raises(SystemExit) as exc:
            trainer.main(argv)
        assert msg in str(exc.value), exc.value
    ints = tmp_path / "ints.npy"
    np.save(ints, np.zeros((3, 8, 8), dtype=np.int64))
    with pytest.raises(SystemExit) as exc:
        trainer.main(ILVR + ["--image", str(ints)])
    assert "a float array shaped" in str(exc.value)


def test_trainer_builds_the_process_for_every_unconditional_config():
    """what `sample --sampler ilvr` puts in place of the YAML's process, built on the host: the config's network and noise schedule (the iddpm
    config's cosine table too), the flags' values"""
    import argparse

    from dmme_amd import trainer

    for name in ("ddpm", "ddim", "iddpm"):
        module = trainer._instantiate(trainer.parse_config(CFG[name])["model_spec"])
        old = module.diffusion_model
        new = trainer._ilvr_process(module, argparse.Namespace(sample_steps=None, down_factor=None, range_level=None))
        assert isinstance(new, dmme_amd.ILVR) and new.model is old.model and torch.equal(new.alpha_bar, old.alpha_bar), name
        assert (new.sub_timesteps, new.down_factor, new.range_level) == (250, 4, 0) and new.chain_length() == 250
    new = trainer._ilvr_process(module, argparse.Namespace(sample_steps=12, down_factor=8, range_level=3))
    assert (new.sub_timesteps, new.down_factor, new.range_level) == (12, 8, 3)
    with pytest.raises(SystemExit):
        trainer._ilvr_process(module, argparse.Namespace(sample_steps=12, down_factor=8, range_level=13))
