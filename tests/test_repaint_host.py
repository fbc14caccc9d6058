"""Host-only checks of RePaint / SDEdit (dmme_amd.RePaint): the level walk against its stated counts and properties and against the
restatement's (tests/repaint_ref.py), the rows the package builds (the fold identity, the exact constants, DDPM's scalars on the full
grid, the timestep table), the schedule taken from another process, the header and the version, the argument checks of the new C entry
points and of the trainer's new flags, the constructor's validation.  No GPU is touched."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib

from . import repaint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS = [(5, 1, 1), (5, 1, 3), (6, 2, 2), (8, 3, 2), (7, 3, 3), (250, 10, 10), (4, 4, 3), (3, 5, 2), (1, 1, 4), (2, 1, 2)]


@pytest.mark.parametrize("n,j,r", WALKS)
def test_walk(n, j, r):
    """starts at n, ends at 0, moves one level at a time, never climbs from level 0, climbs only in runs of exactly j that stay <= n,
    n + (r - 1) j floor((n - 1) / j) downward transitions; j = 1: every step t >= 2 taken r times and the step at t = 1 once"""
    w = dmme_amd.repaint_levels(n, jump_length=j, resamples=r)
    assert w == R.levels(n, j, r)
    assert w[0] == n and w[-1] == 0 and all(abs(b - a) == 1 for a, b in zip(w, w[1:])) and min(w) == 0 and max(w) == n
    assert w.count(0) == 1  # level 0 is the end: nothing climbs from it
    down = sum(1 for a, b in zip(w, w[1:]) if b < a)
    assert down == n + (r - 1) * j * ((n - 1) // j) == R.down_count(n, j, r)
    runs, p = [], 0
    while p + 1 < len(w):
        if w[p + 1] > w[p]:
            q = p
            while q + 1 < len(w) and w[q + 1] > w[q]:
                q += 1
            runs.append((w[p], w[q]))
            p = q
        else:
            p += 1
    assert all(c - b == j and (b - 1) % j == 0 and b >= 1 and c <= n for b, c in runs)
    assert len(runs) == (r - 1) * ((n - 1) // j if j <= n else 0)
    if (n, j, r) in ((4, 4, 3), (3, 5, 2), (1, 1, 4)):
        assert w == list(range(n, -1, -1))  # no room to jump
    if j == 1:
        taken = {t: sum(1 for a, b in zip(w, w[1:]) if a == t and b == t - 1) for t in range(1, n + 1)}
        assert taken[1] == 1 and all(taken[t] == r for t in range(2, n + 1))
    if (n, j, r) == (250, 10, 10):
        assert down == 2410


def test_walk_rejects_nonsense():
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, 0)):
        with pytest.raises(ValueError):
            dmme_amd.repaint_levels(*bad)
    with pytest.raises(ValueError):
        dmme_amd.repaint_rows(R.alpha_bar(10), list(range(11)), [3, 1, 0])


@pytest.mark.parametrize("T,n,j,r", [(100, 100, 3, 2), (100, 8, 3, 2), (1000, 20, 5, 3), (1000, 250, 10, 10), (50, 7, 1, 3)])
def test_rows(T, n, j, r):
    proc = dmme_amd.RePaint(torch.nn.Identity(), T, n, j, r)
    abar = R.alpha_bar(T)
    assert np.array_equal(proc.alpha_bar.reshape(-1).double().numpy(), abar)
    g = proc._tau_host
    assert g == R.grid(abar, n) and g[0] == 0 and g[-1] == T and all(b > a for a, b in zip(g, g[1:])) and [int(v) for v in proc.tau] == g
    if n == T:
        assert g == list(range(T + 1))
    walk = dmme_amd.repaint_levels(len(g) - 1, j, r)
    rows64, ttab = dmme_amd.repaint_rows(abar, g, walk)
    want, want_t = R.rows(abar, g, walk)
    tr = R.transitions(walk)
    n_rows = len(tr)
    assert rows64.shape == (n_rows + 1, 8) and rows64.dtype == np.float64 and ttab == want_t and len(ttab) == n_rows + 1 and ttab[0] == 0
    assert np.allclose(rows64, want, rtol=1e-12, atol=1e-12)
    jumps = 0
    for k, (a, b, c) in enumerate(tr):
        row = rows64[n_rows - k]
        assert ttab[n_rows - k] == g[a]  # the network's timestep
        if c == b:
            assert row[5] == 1.0 and row[6] == 0.0
        else:
            jumps += 1
            prod = np.prod([abar[g[l]] / abar[g[l - 1]] for l in range(b + 1, c + 1)])
            r0 = np.prod([np.sqrt(abar[g[l]] / abar[g[l - 1]]) for l in range(b + 1, c + 1)])
            assert c == b + j and abs(row[5] - r0) <= 1e-12 and abs(row[6] ** 2 - (1.0 - prod)) <= 1e-12
        assert (row[2] == 0.0) == (b == 0) and (row[4] == 0.0) == (b == 0) and row[7] == 0.0
    assert jumps == (r - 1) * ((len(g) - 2) // j)
    last = rows64[1]
    assert last[2] == 0.0 and last[4] == 0.0 and last[3] == 1.0 and last[5] == 1.0 and last[6] == 0.0
    # what the process keeps: the same rows rounded to fp32 (held exactly in python floats); on the full grid DDPM's own scalars
    cnt, rows, tt = proc._chain_tables()
    assert cnt == n_rows == proc.n_rows == len(rows) - 1 and tt == ttab
    got = np.array(rows)
    if n == T:
        ddpm = dmme_amd.DDPM(torch.nn.Identity(), T)
        for i in range(1, n_rows + 1):
            t = tt[i]
            assert rows[i][0] == ddpm._c1[t] and rows[i][1] == ddpm._c2[t] and rows[i][2] == (ddpm._sigma[t] if t > 1 else 0.0)
        assert np.array_equal(got[:, 3:], rows64.astype(np.float32).astype(np.float64)[:, 3:])
        # (and those agree with the float64 values as far as beta can be recovered from the fp32 abar table at all: alpha = abar_t / abar_{t-1}
        # of two values rounded to 2^-24 relative is off by up to 2^-23, which is 1.2e-3 of the smallest beta, 1e-4; c1 is linear in beta)
        assert np.allclose(got[1:, :3], rows64[1:, :3], rtol=1.5e-3, atol=0.0)
    else:
        assert np.array_equal(got, rows64.astype(np.float32).astype(np.float64))
    # SDEdit's tables: the plain walk, loop index = level
    pn, prows, ptt = proc._plain_tables
    assert pn == len(g) - 1 and ptt == g and all(rw[5] == 1.0 and rw[6] == 0.0 for rw in prows)


def test_from_process_follows_an_iddpm_cosine_table():
    p = dmme_amd.IDDPM(torch.nn.Identity(), 100)
    s = dmme_amd.RePaint.from_process(p, sub_timesteps=10, jump_length=2, resamples=2)
    assert torch.equal(s.alpha_bar, p.alpha_bar) and s.timesteps == 100 and s.model is p.model
    assert not torch.equal(s.alpha_bar, dmme_amd.DDPM(torch.nn.Identity(), 100).alpha_bar) and torch.allclose(s._sqrt_alpha_bar, p._sqrt_alpha_bar)
    ab = p.alpha_bar.reshape(-1).double().numpy()
    want, tt = R.rows(ab, R.grid(ab, 10), R.levels(10, 2, 2))
    n, rows, ttab = s._chain_tables()
    assert ttab == tt and n == R.down_count(10, 2, 2) and np.allclose(np.array(rows), want.astype(np.float32).astype(np.float64), rtol=1e-6, atol=1e-12)


def test_python_surface_and_constructor_errors():
    for name in ("RePaint", "PaintChainRunner", "repaint_levels", "repaint_rows"):
        assert name in dmme_amd.__all__ and hasattr(dmme_amd, name)
    assert issubclass(dmme_amd.RePaint, dmme_amd.DDPM)
    from dmme_amd.diffusion_models.ddpm import ChainRunner, chain_draws

    assert issubclass(dmme_amd.PaintChainRunner, ChainRunner)
    proc = dmme_amd.RePaint(torch.nn.Identity(), 100, 10)
    assert proc._chain_kind == _lib.CHAIN_REPAINT == 10 and proc._runner_class is dmme_amd.PaintChainRunner
    assert (proc.sub_timesteps, proc.jump_length, proc.resamples) == (10, 10, 10)
    assert chain_draws(_lib.CHAIN_REPAINT, proc._chain_tables()[1]) is True
    for kw in (dict(jump_length=0), dict(jump_length=1.5), dict(resamples=0), dict(resamples=-1), dict(sub_timesteps=0), dict(sub_timesteps=101),
               dict(sub_timesteps=2.5), dict(alpha_bar=torch.linspace(1, 0.1, 50)), dict(alpha_bar=torch.ones(101))):
        with pytest.raises(ValueError):
            dmme_amd.RePaint(torch.nn.Identity(), 100, **{"sub_timesteps": 10, **kw})
    # the mask: range and shape (checked on the host before any launch)
    like = torch.zeros(2, 3, 8, 8)
    for bad in (torch.full((2, 3, 8, 8), 1.5), torch.full((1, 1, 8, 8), -0.1), torch.zeros(2, 3, 8, 4), torch.zeros(3, 1, 8, 8), torch.zeros(8, 8),
                torch.zeros(1, 2, 8, 8)):
        with pytest.raises(ValueError):
            dmme_amd.RePaint._mask(bad, like)
    m = dmme_amd.RePaint._mask(torch.ones(1, 1, 8, 8), like)
    assert m.shape == like.shape and m.is_contiguous() and m.dtype == torch.float32 and bool((m == 1).all())
    assert bool((dmme_amd.RePaint._mask(None, like) == 0).all())
    for bad in (0.0, -0.5, 1.01):
        with pytest.raises(ValueError):
            proc.edit(torch.zeros(1, 3, 8, 8), bad)
    assert [proc.edit_level(s) for s in (0.001, 0.05, 0.5, 1.0)] == [1, 1, 5, 10] == [R.edit_level(10, s) for s in (0.001, 0.05, 0.5, 1.0)]


def test_header_and_version():
    with open(os.path.join(ROOT, "include", "dmme_hip.h")) as f:
        text = f.read()
    assert "DMME_CHAIN_REPAINT = 10" in text
    for sym in ("dmme_repaint_step", "dmme_chain_update_repaint", "dmme_repaint_chain_step"):
        assert f"DMME_API int {sym}(" in text and sym in _lib.PROTOTYPES
    assert _lib.lib().dmme_version() >= 112


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p, row = C.c_void_p(16), (C.c_float * 8)()
    err = lib.dmme_last_error
    # the eager twin: x, model_out, known, mask, z3, row, B, chw, planes, stream
    assert lib.dmme_repaint_step(None, p, p, p, p, row, 1, 4, 1, None) == -1 and b"repaint_step" in err()
    assert lib.dmme_repaint_step(p, p, None, p, p, row, 1, 4, 1, None) == -1 and b"repaint_step" in err()
    assert lib.dmme_repaint_step(p, p, p, None, p, row, 1, 4, 1, None) == -1 and b"repaint_step" in err()
    assert lib.dmme_repaint_step(p, p, p, p, p, None, 1, 4, 1, None) == -1 and b"repaint_step" in err()
    assert lib.dmme_repaint_step(p, p, p, p, p, row, 1, 4, 3, None) == -1 and b"repaint_step" in err() and b"planes" in err()
    assert lib.dmme_repaint_step(p, p, p, p, p, row, 1, 4, 0, None) == -1 and b"planes" in err()
    assert lib.dmme_repaint_step(p, p, p, p, p, row, 1, 6, 1, None) == -2 and b"repaint_step" in err() and b"multiple of 4" in err()
    drawing = (C.c_float * 8)(1.0, 0.0, 0.5, 1.0, 0.0, 1.0, 0.0, 0.0)
    assert lib.dmme_repaint_step(p, p, p, p, None, drawing, 1, 4, 1, None) == -1 and b"repaint_step" in err() and b"needs z" in err()
    # the chain form: x, model_out, known, mask, noise, step_coef, t_table, state, B, chw, planes, stream
    assert lib.dmme_chain_update_repaint(p, p, None, p, None, p, p, p, 1, 4, 1, None) == -1 and b"chain_update_repaint" in err()
    assert lib.dmme_chain_update_repaint(p, p, p, p, None, None, p, p, 1, 4, 1, None) == -1 and b"chain_update_repaint" in err()
    assert lib.dmme_chain_update_repaint(p, p, p, p, None, p, p, None, 1, 4, 1, None) == -1 and b"chain_update_repaint" in err()
    assert lib.dmme_chain_update_repaint(p, p, p, p, None, p, p, p, 1, 4, 5, None) == -1 and b"planes" in err()
    assert lib.dmme_chain_update_repaint(p, p, p, p, None, p, p, p, 1, 10, 1, None) == -2 and b"chain_update_repaint" in err()
    # the capturable step: a null plan, a null image
    assert lib.dmme_repaint_chain_step(None, p, p, p, p, p, p, p, p, p, None) == -1 and b"repaint_chain_step" in err()
    # the entry points of the 4-wide kinds keep refusing the new kind, with the messages they had
    assert lib.dmme_chain_update(10, p, p, p, p, p, 1, 4, None) == -1 and b"unknown sampler kind 10" in err()
    assert lib.dmme_chain_update(11, p, p, p, p, p, 1, 4, None) == -1 and b"unknown sampler kind 11" in err()
    assert lib.dmme_chain_step(p, p, p, p, p, 10, p, p, p, None) == -1 and b"chain_step: sampler kind 10" in err()
    assert lib.dmme_chain_update_cfg(10, p, p, None, p, p, p, 1, 4, None) == -1 and b"kind 10 is not a classifier-free kind (6, 7)" in err()


CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "ddim", "iddpm", "cfg")}
IMG, MSK = ["--image", "x.npy"], ["--mask", "m.npy"]


@pytest.mark.parametrize("argv,msg", [
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint"] + MSK, "needs --image"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint"] + IMG, "needs --mask"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "sdedit"], "needs --image"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "sdedit"] + IMG, "--strength S in (0, 1]"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "sdedit", "--strength", "0"] + IMG, "--strength S in (0, 1]"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "sdedit", "--strength", "1.5"] + IMG, "--strength S in (0, 1]"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint", "--strength", "0.5"] + IMG + MSK, "--strength belongs to --sampler sdedit"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "sdedit", "--strength", "0.5", "--jump-length", "5"] + IMG, "--jump-length belongs to --sampler repaint"),
    (["sample", "--config", CFG["ddpm"], "--jump-length", "5"], "--jump-length belongs to --sampler repaint / sdedit"),
    (["sample", "--config", CFG["ddim"], "--sampler", "dpm++", "--resamples", "2"] + IMG, "--image, --resamples belong to --sampler repaint / sdedit"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint", "--jump-length", "0"] + IMG + MSK, "--jump-length must be at least 1"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint", "--sample-steps", "0"] + IMG + MSK, "--sample-steps"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint", "--eta", "0.5"] + IMG + MSK, "--eta does not go with --sampler repaint"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "sdedit", "--strength", "0.5", "--steps", "3"] + IMG, "--steps does not go with --sampler sdedit"),
    (["sample", "--config", CFG["cfg"], "--sampler", "repaint"] + IMG + MSK, "needs an unconditional config"),
    (["sample", "--config", CFG["cfg"], "--sampler", "sdedit", "--strength", "0.5"] + IMG, "needs an unconditional config"),
    (["sample", "--config", CFG["cfg"], "--sampler", "repaint", "--labels", "3"] + IMG + MSK, "--labels does not go with --sampler repaint"),
    (["fit", "--config", CFG["ddpm"], "--sampler", "repaint"] + IMG + MSK, "belongs to `sample`"),
    (["fit", "--config", CFG["ddpm"], "--sampler", "sdedit", "--strength", "0.5"] + IMG, "belongs to `sample`"),
    (["fit", "--config", CFG["ddpm"], "--save", "out.npy"], "--save belongs to `sample`"),
    (["sample", "--config", CFG["ddpm"], "--sampler", "repaint", "--image", "/nonexistent/x.npy"] + MSK, "--image /nonexistent/x.npy"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


def test_trainer_rejects_a_bad_image_file(tmp_path):
    from dmme_amd import trainer

    bad = tmp_path / "ints.npy"
    np.save(bad, np.zeros((3, 8, 8), dtype=np.int64))
    with pytest.raises(SystemExit) as exc:
        trainer.main(["sample", "--config", CFG["ddpm"], "--sampler", "sdedit", "--strength", "0.5", "--image", str(bad)])
    assert "a float array shaped" in str(exc.value)
    good = tmp_path / "img.npy"
    np.save(good, np.zeros((3, 8, 8), dtype=np.float32))
    assert tuple(trainer._load_npy(str(good), "--image").shape) == (1, 3, 8, 8)


def test_trainer_builds_the_process_for_every_unconditional_config():
    """what `sample --sampler repaint / sdedit` puts in place of the YAML's process, built on the host: the config's network and noise
    schedule (the iddpm config's cosine table too), the flags' values"""
    import argparse

    from dmme_amd import trainer

    for name in ("ddpm", "ddim", "iddpm"):
        module = trainer._instantiate(trainer.parse_config(CFG[name])["model_spec"])
        old = module.diffusion_model
        new = trainer._paint_process(module, argparse.Namespace(sample_steps=None, jump_length=None, resamples=None))
        assert isinstance(new, dmme_amd.RePaint) and new.model is old.model and torch.equal(new.alpha_bar, old.alpha_bar), name
        assert (new.sub_timesteps, new.jump_length, new.resamples) == (250, 10, 10) and new.n_rows == 2410
    new = trainer._paint_process(module, argparse.Namespace(sample_steps=12, jump_length=3, resamples=2))
    assert (new.sub_timesteps, new.jump_length, new.resamples) == (12, 3, 2)
