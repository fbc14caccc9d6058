"""Host-only checks of DDNM (dmme_amd.DDNM): the rows the package builds against the formulas in float64 (the exact last row, lambda and
cz with and without measurement noise, RePaint's folded jump), the identities that make A+ the pseudo-inverse of A = M o Pool_s o Gray_g,
the two bounds the GPU tests rely on (the restatement in fp32 sits inside them), the Python surface, the header and the binding, the
argument checks of the new C entry points, of the constructor and of the trainer's new flags.  No GPU is touched."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib

from . import ddnm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the rows
@pytest.mark.parametrize("T,n,sigma_y,travel", [(100, 100, 0.0, (1, 1)), (100, 8, 0.0, (1, 1)), (1000, 12, 0.1, (3, 2)), (1000, 100, 0.1, (1, 1)), (1000, 100, 0.5, (1, 1)),
                                                (1000, 20, 0.5, (5, 3)), (50, 7, 0.0, (2, 2))])
def test_rows(T, n, sigma_y, travel):
    from dmme_amd.diffusion_models.repaint import repaint_rows

    proc = dmme_amd.DDNM(torch.nn.Identity(), T, n, sigma_y=sigma_y, travel_length=travel[0], travel_repeat=travel[1])
    abar = R.alpha_bar(T)
    g = proc._tau_host
    assert g == R.grid(abar, n) and g[0] == 0 and g[-1] == T and [int(v) for v in proc.tau] == g
    walk = dmme_amd.repaint_levels(len(g) - 1, *travel)
    assert proc._walk == walk
    rows64, ttab = dmme_amd.ddnm_rows(abar, g, walk, sigma_y)
    want, want_t = R.rows(abar, g, walk, sigma_y)
    steps = R.transitions(walk)
    L = len(steps)
    assert rows64.shape == (L + 1, 8) and rows64.dtype == np.float64 and ttab == want_t
    assert np.allclose(rows64, want, rtol=1e-12, atol=1e-15)
    # the folded jump and the timesteps are RePaint's on the same walk, to the bit
    paint, ptt = repaint_rows(abar, g, walk)
    assert ptt == ttab and np.array_equal(rows64[1:, 6:8], paint[1:, 5:7])
    ab = np.asarray(abar, dtype=np.float64)
    for k, (a, b, c) in enumerate(steps):
        i = L - k
        ca, cb, cz, at, bt, lam, r0, r1 = rows64[i]
        assert at == 1.0 / np.sqrt(ab[g[a]]) and bt == np.sqrt(1.0 - ab[g[a]]) / np.sqrt(ab[g[a]])
        assert (r1 != 0.0) == (c > b) and cz >= 0.0 and 0.0 <= lam <= 1.0
        if b == 0:
            assert tuple(rows64[i, :3]) == (1.0, 0.0, 0.0) and (r0, r1) == (1.0, 0.0) and lam == (1.0 if sigma_y == 0.0 else 0.0)
            continue
        var = (1.0 - ab[g[a]] / ab[g[b]]) * (1.0 - ab[g[b]]) / (1.0 - ab[g[a]])
        if sigma_y == 0.0:
            assert lam == 1.0 and abs(cz - np.sqrt(var)) <= 1e-15
        else:
            # the total variance of the step is the posterior's: (ca lambda sigma_y)^2 + cz^2 = var wherever lambda < 1 leaves room
            assert abs((ca * lam * sigma_y) ** 2 + cz * cz - var) <= 1e-15 or cz == 0.0
            assert (lam < 1.0) == (np.sqrt(var) < ca * sigma_y)
    assert rows64[1, 5] == (1.0 if sigma_y == 0.0 else 0.0)
    if sigma_y > 0.0 and (n >= 100 or sigma_y >= 0.5):  # (a coarse grid's steps all have sigma above ca sigma_y at sigma_y = 0.1)
        assert any(0.0 < r[5] < 1.0 for r in rows64[2:]), "a noisy measurement shrinks lambda somewhere"
    # what the process keeps: the rows rounded to fp32 once
    cnt, rows, tt = proc._chain_tables()
    assert cnt == L == proc.n_rows == proc.chain_length() and tt == ttab
    assert np.array_equal(np.array(rows), rows64.astype(np.float32).astype(np.float64))
    assert rows[1][:3] == (1.0, 0.0, 0.0) and rows[1][6:] == (1.0, 0.0)


def test_cz_needs_its_max():
    """where lambda < 1 the difference var - (ca lambda sigma_y)^2 is zero in exact arithmetic and comes out below zero in float64 for some
    step of the linear schedule at sigma_y = 0.5: the rows must not hold a NaN"""
    abar = R.alpha_bar(1000)
    g = R.grid(abar, 1000)
    rows64, _ = dmme_amd.ddnm_rows(abar, g, list(range(1000, -1, -1)), 0.5)
    assert bool(np.isfinite(rows64).all()) and float(rows64[:, 2].min()) >= 0.0
    with pytest.raises(ValueError):
        dmme_amd.ddnm_rows(abar, g, [3, 2, 0], 0.0)
    with pytest.raises(ValueError):
        dmme_amd.ddnm_rows(abar, g, [3, 2, 1, 0], -0.1)


def test_from_process_follows_an_iddpm_cosine_table():
    p = dmme_amd.IDDPM(torch.nn.Identity(), 100)
    s = dmme_amd.DDNM.from_process(p, sub_timesteps=10, scale=2, gray=True, sigma_y=0.1, travel_length=2, travel_repeat=2)
    assert torch.equal(s.alpha_bar, p.alpha_bar) and s.timesteps == 100 and s.model is p.model
    assert (s.scale, s.gray, s.sigma_y, s.travel_length, s.travel_repeat) == (2, True, 0.1, 2, 2)
    ab = p.alpha_bar.reshape(-1).double().numpy()
    g = R.grid(ab, 10)
    want, tt = R.rows(ab, g, dmme_amd.repaint_levels(len(g) - 1, 2, 2), 0.1)
    n, rows, ttab = s._chain_tables()
    assert ttab == tt and n == len(tt) - 1 and np.allclose(np.array(rows), want.astype(np.float32).astype(np.float64), rtol=1e-6, atol=1e-12)


# ------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("s", [1, 2, 5])
def test_pseudo_inverse_identities(gray, s):
    """A A+ A = A and A+ A A+ = A+ in float64 on 10 x 20 images under random binary masks (per image and channel, and broadcast); the
    package's host-side `pinv` is the restatement's A+; a fractional mask breaks the first identity, which is why it is refused"""
    proc = dmme_amd.DDNM(torch.nn.Identity(), 100, 10, scale=s, gray=gray)
    g = torch.Generator().manual_seed(100 * s + gray)
    x = torch.randn(2, 3, 10, 20, dtype=torch.float64, generator=g)
    shape = proc.measurement_shape(x.shape)
    assert shape == (2, 1 if gray else 3, 10 // s, 20 // s)
    for mshape in (shape, (1, 1) + shape[2:]):
        m = (torch.rand(mshape, generator=g) < 0.6).double()
        y = R.A(x, s, gray, m)
        assert y.shape == shape
        back = R.A_pinv(y, s, gray, 3, m)
        assert torch.equal(proc.pinv(y, m), back) and back.shape == x.shape
        e1 = float((R.A(back, s, gray, m) - y).abs().max())
        e2 = float((R.A_pinv(R.A(back, s, gray, m), s, gray, 3, m) - back).abs().max())
        print(f"gray {gray} s {s} mask {mshape}: |A A+ A x - A x| = {e1:.2e}, |A+ A A+ y - A+ y| = {e2:.2e}")
        assert e1 <= 1e-15 and e2 <= 1e-15
    half = torch.full(shape, 0.5, dtype=torch.float64)
    y = R.A(x, s, gray, half)
    assert float((R.A(R.A_pinv(y, s, gray, 3, half), s, gray, half) - y).abs().max()) > 1e-3
    with pytest.raises(ValueError, match="0 or 1"):
        proc.pinv(y, half)


# ------------------------------------------------------------------------------------------ the bounds of the GPU tests
@pytest.mark.parametrize("shape,s,gray", [((2, 3, 8, 8), 2, False), ((2, 3, 10, 20), 5, False), ((1, 3, 32, 32), 4, True), ((2, 3, 12, 20), 1, False)])
def test_the_updates_bound_holds_for_the_restatement_in_fp32(shape, s, gray):
    """tests/ddnm_ref.py in fp32 against itself in float64 on fp32 rows must sit inside `update_bound` before the device is asked to"""
    g = torch.Generator().manual_seed(11)
    x, e = (torch.randn(shape, generator=g) for _ in range(2))
    z2 = torch.randn((2,) + shape, generator=g)
    mshape = (shape[0], 1 if gray else shape[1], shape[2] // s, shape[3] // s)
    y = torch.randn(mshape, generator=g)
    m = (torch.rand(mshape, generator=g) < 0.7).float()
    for name, row in R.update_rows().items():
        got = R.step(x, e, y, m, z2, row, s, gray, torch.float32)
        want = R.step(x, e, y, m, z2, row, s, gray, torch.float64)
        bound = R.update_bound(x, e, y, m, z2, row, s, gray)
        ratio = float(((got.double() - want).abs() / bound).max())
        print(f"{shape} s {s} gray {gray} row {name}: the restatement in fp32 at {ratio:.3f} of the bound")
        assert ratio <= 1.0


def _mean32(v):
    """the mean of the last axis in float32 with sequential sums"""
    return (np.cumsum(v.astype(np.float32), axis=-1, dtype=np.float32)[..., -1] / np.float32(v.shape[-1])).astype(np.float32)


@pytest.mark.parametrize("n", [1, 4, 12, 25, 48, 75, 256, 3072])
def test_the_consistency_bound_holds_for_sequential_fp32_sums(n):
    """xh = x0 - (mean(x0) - y) and then mean(xh) against y, all in float32 with sequential sums, over 200 cells of n elements at scales
    0.1 ... 30: inside (2 n + 4) 2^-24 max(|x0|, |xh|, |y|)"""
    rng = np.random.default_rng(n)
    scale = np.exp(rng.uniform(np.log(0.1), np.log(30.0), size=(200, 1)))
    x0 = (scale * rng.standard_normal((200, n))).astype(np.float32)
    y = (scale[:, 0] * rng.standard_normal(200)).astype(np.float32)
    xh = (x0 - (_mean32(x0) - y)[:, None]).astype(np.float32)
    got = _mean32(xh)
    bound = R.consistency_bound(torch.from_numpy(x0).reshape(200, 1, 1, n), torch.from_numpy(xh).reshape(200, 1, 1, n), torch.from_numpy(y).reshape(200, 1, 1, 1),
                                1, False) if n == 1 else None
    M = np.maximum(np.maximum(np.abs(x0).max(axis=1), np.abs(xh).max(axis=1)), np.abs(y)).astype(np.float64)
    mine = (2 * n + 4) * R.EPS * M
    ratio = float((np.abs(got.astype(np.float64) - y.astype(np.float64)) / mine).max())
    print(f"n = {n}: largest |mean(xh) - y| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    if bound is not None:
        assert np.allclose(bound.reshape(-1).numpy(), mine, rtol=1e-12)


# ------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_and_constructor_errors():
    for name in ("DDNM", "RestoreChainRunner", "ddnm_rows"):
        assert name in dmme_amd.__all__ and hasattr(dmme_amd, name)
    from dmme_amd.diffusion_models.ddpm import ChainRunner, chain_draws

    assert issubclass(dmme_amd.DDNM, dmme_amd.DDPM) and issubclass(dmme_amd.RestoreChainRunner, ChainRunner)
    proc = dmme_amd.DDNM(torch.nn.Identity(), 100, 10)
    assert proc._chain_kind == _lib.CHAIN_DDNM == 12 and proc._runner_class is dmme_amd.RestoreChainRunner
    assert (proc.sub_timesteps, proc.scale, proc.gray, proc.sigma_y, proc.travel_length, proc.travel_repeat) == (10, 1, False, 0.0, 1, 1)
    assert dmme_amd.DDNM(torch.nn.Identity()).sub_timesteps == 100
    rows = proc._chain_tables()[1]
    assert chain_draws(_lib.CHAIN_DDNM, rows) is True
    quiet = [(1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0)] * 3
    assert chain_draws(_lib.CHAIN_DDNM, quiet) is False
    assert chain_draws(_lib.CHAIN_DDNM, quiet + [(1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.5, 0.5)]) is True
    assert chain_draws(_lib.CHAIN_DDNM, quiet + [(1.0, 0.0, 0.3, 1.0, 0.0, 1.0, 1.0, 0.0)]) is True
    for kw in (dict(scale=0), dict(scale=2.5), dict(scale=True), dict(sigma_y=-0.1), dict(sigma_y=float("nan")), dict(travel_length=0), dict(travel_repeat=0),
               dict(travel_length=1.5), dict(sub_timesteps=0), dict(sub_timesteps=101), dict(sub_timesteps=2.5), dict(alpha_bar=torch.linspace(1, 0.1, 50)),
               dict(prediction="nope"), dict(threshold="nope")):
        with pytest.raises(ValueError):
            dmme_amd.DDNM(torch.nn.Identity(), 100, **{"sub_timesteps": 10, **kw})
    # refused on the host before any launch or draw: a scale that does not divide the image, a mask that is not binary or of another
    # shape, a measurement of the wrong shape
    sr = dmme_amd.DDNM(torch.nn.Identity(), 100, 10, scale=4)
    with pytest.raises(ValueError, match="not divisible by scale"):
        sr.degrade(torch.zeros(1, 3, 10, 8))
    with pytest.raises(ValueError, match="not divisible by scale"):
        sr.generate((1, 3, 10, 8))
    with pytest.raises(ValueError, match="0 or 1"):
        sr.restore(torch.zeros(1, 3, 2, 2), torch.full((1, 3, 2, 2), 0.5))
    with pytest.raises(ValueError, match="does not broadcast"):
        sr.restore(torch.zeros(1, 3, 2, 2), torch.ones(1, 3, 8, 8))
    with pytest.raises(ValueError, match="does not broadcast"):
        sr.degrade(torch.zeros(1, 3, 8, 8), torch.ones(1, 3, 8, 8))
    with pytest.raises(ValueError):
        sr.restore(torch.zeros(3, 2, 2))
    with pytest.raises(ValueError, match="one channel"):
        dmme_amd.DDNM(torch.nn.Identity(), 100, 10, gray=True).restore(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        proc.sampling_step(torch.zeros(1, 3, 8, 8), torch.tensor([3]))


# ------------------------------------------------------------------------------------------ the header, the binding, the C argument checks
def test_header_and_version():
    with open(os.path.join(ROOT, "include", "dmme_hip.h")) as f:
        text = f.read()
    assert "DMME_CHAIN_DDNM = 12" in text
    for sym in ("dmme_ddnm_measure", "dmme_ddnm_step", "dmme_chain_update_ddnm", "dmme_ddnm_chain_step", "dmme_ddnm_band_capacity"):
        assert f"DMME_API int {sym}(" in text and sym in _lib.PROTOTYPES
    for word in ("ca = sqrt(abar_b) beta/(1 - abar_a)", "{1, 0, 0, A_t, B_t, lambda, 1, 0}", "offset + s * (B*chw/4) + g/4"):
        assert word in text, word
    lib = _lib.lib()
    assert lib.dmme_version() >= 118
    cap = lib.dmme_ddnm_band_capacity()
    assert cap >= 3 * 32 * 256 and cap * 4 <= 160 * 1024


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p, row = C.c_void_p(16), (C.c_float * 8)(1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0)
    err = lib.dmme_last_error
    # the measurement: x, mask, y_out, B, C, H, W, s, gray, stream
    assert lib.dmme_ddnm_measure(None, p, p, 1, 3, 8, 8, 2, 0, None) == -1 and b"ddnm_measure" in err()
    assert lib.dmme_ddnm_measure(p, None, None, 1, 3, 8, 8, 2, 0, None) == -1 and b"ddnm_measure" in err()
    assert lib.dmme_ddnm_measure(p, None, p, 0, 3, 8, 8, 2, 0, None) == -1 and b"ddnm_measure" in err()
    assert lib.dmme_ddnm_measure(p, None, p, 1, 3, 8, 8, 0, 0, None) == -1 and b"ddnm_measure" in err()
    assert lib.dmme_ddnm_measure(p, None, p, 1, 3, 8, 8, 3, 0, None) == -1 and b"does not divide" in err()
    assert lib.dmme_ddnm_measure(p, None, p, 1, 3, 8, 8, 2, 2, None) == -1 and b"gray" in err()
    assert lib.dmme_ddnm_measure(p, None, p, 1, 3, 6, 6, 2, 0, None) == -2 and b"multiples of 4" in err()
    cap = lib.dmme_ddnm_band_capacity()
    assert lib.dmme_ddnm_measure(p, None, p, 1, 3, 64, 512, 32, 1, None) == -2 and str(cap).encode() in err() and 3 * 32 * 512 > cap
    # the eager twin: x, model_out, y, mask, z2, row, B, C, H, W, s, gray, planes, stream
    assert lib.dmme_ddnm_step(None, p, p, p, p, row, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"ddnm_step" in err()
    assert lib.dmme_ddnm_step(p, None, p, p, p, row, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"ddnm_step" in err()
    assert lib.dmme_ddnm_step(p, p, None, p, p, row, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"ddnm_step" in err()
    assert lib.dmme_ddnm_step(p, p, p, None, p, row, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"ddnm_step" in err()
    assert lib.dmme_ddnm_step(p, p, p, p, p, None, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"ddnm_step" in err()
    assert lib.dmme_ddnm_step(p, p, p, p, p, row, 1, 3, 8, 8, 2, 0, 3, None) == -1 and b"planes" in err()
    assert lib.dmme_ddnm_step(p, p, p, p, p, row, 1, 3, 8, 8, 3, 0, 1, None) == -1 and b"does not divide" in err()
    assert lib.dmme_ddnm_step(p, p, p, p, p, row, 1, 3, 5, 5, 1, 0, 1, None) == -2 and b"ddnm_step" in err() and b"multiples of 4" in err()
    assert lib.dmme_ddnm_step(p, p, p, p, p, row, 1, 3, 64, 512, 32, 1, 1, None) == -2 and b"dmme_ddnm_band_capacity" in err()
    drawing = (C.c_float * 8)(0.5, 0.5, 0.3, 1.0, 0.0, 1.0, 1.0, 0.0)
    assert lib.dmme_ddnm_step(p, p, p, p, None, drawing, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"needs z" in err()
    jumping = (C.c_float * 8)(0.5, 0.5, 0.0, 1.0, 0.0, 1.0, 0.8, 0.6)
    assert lib.dmme_ddnm_step(p, p, p, p, None, jumping, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"needs z" in err()
    # the chain form: x, model_out, y, mask, noise, step_coef, t_table, state, B, C, H, W, s, gray, planes, stream
    assert lib.dmme_chain_update_ddnm(p, p, None, p, None, p, p, p, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"chain_update_ddnm" in err()
    assert lib.dmme_chain_update_ddnm(p, p, p, p, None, None, p, p, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"chain_update_ddnm" in err()
    assert lib.dmme_chain_update_ddnm(p, p, p, p, None, p, None, p, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"chain_update_ddnm" in err()
    assert lib.dmme_chain_update_ddnm(p, p, p, p, None, p, p, None, 1, 3, 8, 8, 2, 0, 1, None) == -1 and b"chain_update_ddnm" in err()
    assert lib.dmme_chain_update_ddnm(p, p, p, p, None, p, p, p, 1, 3, 8, 8, 2, 0, 5, None) == -1 and b"planes" in err()
    assert lib.dmme_chain_update_ddnm(p, p, p, p, None, p, p, p, 1, 3, 5, 5, 1, 0, 1, None) == -2 and b"multiples of 4" in err()
    assert lib.dmme_chain_update_ddnm(p, p, p, p, None, p, p, p, 1, 3, 8, 8, 3, 1, 1, None) == -1 and b"does not divide" in err()
    # the capturable step: a null plan
    assert lib.dmme_ddnm_chain_step(None, p, p, p, p, p, p, 2, 0, p, p, p, None) == -1 and b"ddnm_chain_step" in err()
    # the entry points of the table's kinds refuse the new kind
    assert lib.dmme_chain_update(12, p, p, p, p, p, 1, 4, None) == -1 and b"unknown sampler kind 12" in err()
    assert lib.dmme_chain_step(p, p, p, p, p, 12, p, p, p, None) == -1 and b"chain_step: sampler kind 12" in err()


# ------------------------------------------------------------------------------------------ the trainer
CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "ddim", "iddpm", "cfg")}
MEAS = ["--measurement", "y.npy"]
DDNM = ["sample", "--config", CFG["ddpm"], "--sampler", "ddnm"]


@pytest.mark.parametrize("argv,msg", [
    (DDNM, "needs exactly one of --measurement"),
    (DDNM + MEAS + ["--image", "x.npy"], "needs exactly one of --measurement"),
    (DDNM + MEAS + ["--eta", "0.5"], "--eta does not go with --sampler ddnm"),
    (DDNM + MEAS + ["--steps", "3"], "--steps does not go with --sampler ddnm"),
    (DDNM + MEAS + ["--labels", "3"], "--labels does not go with --sampler ddnm"),
    (DDNM + MEAS + ["--guidance-scale", "2"], "--guidance-scale does not go with --sampler ddnm"),
    (DDNM + MEAS + ["--strength", "0.5"], "--strength does not go with --sampler ddnm"),
    (DDNM + MEAS + ["--down-factor", "4"], "--down-factor belongs to --sampler ilvr"),
    (DDNM + MEAS + ["--sr-scale", "0"], "--sr-scale must be at least 1"),
    (DDNM + MEAS + ["--sigma-y", "-1"], "--sigma-y must be at least 0"),
    (DDNM + MEAS + ["--sample-steps", "0"], "--sample-steps must be at least 1"),
    (DDNM + MEAS + ["--jump-length", "0"], "--jump-length must be at least 1"),
    (DDNM + MEAS + ["--resamples", "0"], "--resamples must be at least 1"),
    (["fit", "--config", CFG["ddpm"], "--sampler", "ddnm"] + MEAS, "belongs to `sample`"),
    (["sample", "--config", CFG["ddpm"], "--sr-scale", "4"], "--sr-scale belongs to --sampler ddnm"),
    (["sample", "--config", CFG["ddpm"], "--gray"], "--gray belongs to --sampler ddnm"),
    (["sample", "--config", CFG["ddpm"], "--sigma-y", "0.1"], "--sigma-y belongs to --sampler ddnm"),
    (["sample", "--config", CFG["ddpm"], "--measurement", "y.npy"], "--measurement belongs to --sampler ddnm"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "ilvr", "--image", "x.npy", "--sr-scale", "2", "--gray"], "--sr-scale, --gray belong to --sampler ddnm"),
    (DDNM + ["--measurement", "/nonexistent/y.npy"], "--measurement /nonexistent/y.npy"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


def test_trainer_checks_the_inputs_against_the_operator(tmp_path):
    """a scale that does not divide the image, a grey measurement of three channels, a mask of the image's resolution or with fractional
    values and the conditional config are refused before anything touches the GPU"""
    from dmme_amd import trainer

    img = tmp_path / "img.npy"
    np.save(img, np.zeros((3, 32, 32), dtype=np.float32))
    odd = tmp_path / "odd.npy"
    np.save(odd, np.zeros((2, 3, 30, 32), dtype=np.float32))
    meas = tmp_path / "meas.npy"
    np.save(meas, np.zeros((3, 8, 8), dtype=np.float32))
    big_mask = tmp_path / "big.npy"
    np.save(big_mask, np.ones((1, 1, 32, 32), dtype=np.float32))
    soft = tmp_path / "soft.npy"
    np.save(soft, np.full((1, 1, 8, 8), 0.5, dtype=np.float32))
    for argv, msg in ((DDNM + ["--image", str(odd), "--sr-scale", "4"], "30 x 32 is not divisible by --sr-scale 4"),
                      (DDNM + ["--image", str(img), "--sr-scale", "5"], "32 x 32 is not divisible by --sr-scale 5"),
                      (DDNM + ["--measurement", str(meas), "--gray"], "a --gray measurement has one channel"),
                      (DDNM + ["--image", str(img), "--sr-scale", "4", "--mask", str(big_mask)], "the mask is at measurement resolution"),
                      (DDNM + ["--measurement", str(meas), "--sr-scale", "4", "--mask", str(soft)], "values must be 0 or 1"),
                      (["sample", "--config", CFG["cfg"], "--sampler", "ddnm", "--measurement", str(meas)], "needs an unconditional config")):
        with pytest.raises(SystemExit) as exc:
            trainer.main(argv)
        assert msg in str(exc.value), exc.value


def test_trainer_builds_the_process_for_every_unconditional_config():
    """what `sample --sampler ddnm` puts in place of the YAML's process, built on the host: the config's network and noise schedule (the
    iddpm config's cosine table too), the flags' values and their defaults"""
    import argparse

    from dmme_amd import trainer

    none = dict(sample_steps=None, sr_scale=None, gray=False, sigma_y=None, jump_length=None, resamples=None)
    for name in ("ddpm", "ddim", "iddpm"):
        module = trainer._instantiate(trainer.parse_config(CFG[name])["model_spec"])
        old = module.diffusion_model
        new = trainer._ddnm_process(module, argparse.Namespace(**none))
        assert isinstance(new, dmme_amd.DDNM) and new.model is old.model and torch.equal(new.alpha_bar, old.alpha_bar), name
        assert (new.sub_timesteps, new.scale, new.gray, new.sigma_y, new.travel_length, new.travel_repeat) == (100, 1, False, 0.0, 1, 1)
        assert new.chain_length() == 100
    new = trainer._ddnm_process(module, argparse.Namespace(sample_steps=12, sr_scale=4, gray=True, sigma_y=0.1, jump_length=3, resamples=2))
    assert (new.sub_timesteps, new.scale, new.gray, new.sigma_y, new.travel_length, new.travel_repeat) == (12, 4, True, 0.1, 3, 2)
    assert new.chain_length() == len(R.transitions(dmme_amd.repaint_levels(new.n_levels, 3, 2)))
