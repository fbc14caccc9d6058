"""CPU: the probability-flow ODE (dmme_amd.ProbabilityFlow) without a GPU - the stage tables against the closed forms and against
GeneralizedDDIM's rows, the analytic Gaussian problem in the float64 restatement (tests/pfode_ref.py), the Rademacher restatement, the
derived stage bound against a plain fp32 evaluation, the host's noise rule, and the refusals of the process and of the trainer."""

import os

import numpy as np
import pytest
import torch

from oracle import synth

from . import pfode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [1, 26, 50, 75, 100]


# ------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("direction", ["encode", "decode"])
def test_rows_are_the_closed_forms(direction):
    """the package's float64 rows equal the restatement's; stage A followed by stage B is the direct Heun expression
    x_b = k0 x_a + (k1 / 2)(e_a + e_b) to float64 rounding, for every step of the grid in both directions; the saved buffers hold (x_a, e_a)"""
    import dmme_amd

    ab = R.alpha_bar(100)
    for lik in (False, True):
        rows, ttab = dmme_amd.pf_rows(ab, GRID, direction, likelihood=lik)
        want, wtab = R.tables(ab, GRID, direction, lik)
        assert rows.shape == want.shape and ttab == wtab and np.allclose(rows, want, rtol=1e-15, atol=0)
        assert bool((rows[1:, R.W] != 0).any()) == lik
    n = rows.shape[0] - 1
    assert n == 2 * (len(GRID) - 1) + (1 if direction == "decode" else 0)
    g = GRID if direction == "encode" else GRID[::-1]
    x_a, e_a, e_b = (synth.normal(k, (2, 3, 4, 4)).double() for k in (1, 2, 3))
    for j, (a, b) in enumerate(zip(g, g[1:])):
        k0, k1, h = R.heun(ab, a, b)
        rA, rB = rows[n - 2 * j], rows[n - 2 * j - 1]
        assert (ttab[n - 2 * j], ttab[n - 2 * j - 1]) == (a, b) and rA[R.SAVE] == 1 and rB[R.SAVE] == 0
        junk = torch.full_like(x_a, float("nan"))
        x1, xs, es = R.stage(x_a, junk, e_a, junk, rA)
        assert torch.equal(xs, x_a) and torch.equal(es, e_a)
        assert float((x1 - (k0 * x_a + k1 * e_a)).abs().max()) <= 1e-15 * float(x1.abs().max())
        x2, xs, es = R.stage(x1, xs, e_b, es, rB)
        direct = k0 * x_a + 0.5 * k1 * (e_a + e_b)
        assert float((x2 - direct).abs().max()) <= 4e-16 * float(direct.abs().max() + 1)
        assert abs(rA[R.W] - 0.5 * h * np.sqrt(ab[a])) <= 1e-18 + 1e-15 * abs(rA[R.W]) and abs(rB[R.W] - 0.5 * h * np.sqrt(ab[b])) <= 1e-15 * abs(rB[R.W])
        assert (h > 0) == (direction == "encode")
    if direction == "decode":
        last = rows[1]
        assert ttab[1] == GRID[0] and np.allclose(last[:6], [1 / np.sqrt(ab[1]), 0, -np.sqrt(1 - ab[1]) / np.sqrt(ab[1]), 0, 0, 0], rtol=1e-15)
        raw, rtab = dmme_amd.pf_rows(ab, GRID, "decode", final_denoise=False)
        plain = dmme_amd.pf_rows(ab, GRID, "decode")[0]
        assert raw.shape[0] == n and np.array_equal(raw[1:], plain[2:]) and rtab[1:] == ttab[2:]


def test_stage_a_rows_are_generalized_ddims():
    """an A row's (k0, k1) in fp32 equals GeneralizedDDIM's reverse / encode row for the same pair of timesteps: the Euler method on this
    ODE is that sampler"""
    import dmme_amd

    gd = dmme_amd.GeneralizedDDIM(torch.nn.Identity(), 100, 4, "linear", eta=0.0)
    tau = gd._tau_host
    assert tau == [0, 25, 50, 75, 100]
    pf = dmme_amd.ProbabilityFlow(torch.nn.Identity(), 100, grid=tau[1:])
    n, dec, dtab = pf._tables["decode_raw"]
    for j, i in enumerate(range(4, 1, -1)):  # the reverse steps tau_i -> tau_{i-1}
        row = dec[n - 2 * j]
        assert dtab[n - 2 * j] == tau[i] and (row[0], row[2]) == (gd._rev_rows[i][0], gd._rev_rows[i][1]), i
    n, enc, etab = pf._tables["encode"]
    for j in range(3):  # the encoding steps tau_{1+j} -> tau_{2+j}: GeneralizedDDIM's index S - (1 + j)
        row, theirs = enc[n - 2 * j], gd._enc_rows[4 - (1 + j)]
        assert etab[n - 2 * j] == tau[1 + j] and (row[0], row[2]) == (theirs[0], theirs[1]), j


def test_grid_and_constructor():
    import dmme_amd

    ab = R.alpha_bar(100)
    assert dmme_amd.pf_grid(ab, 4) == [1, 25, 50, 75, 100] and dmme_amd.pf_grid(ab, 4, t_min=25) == [25, 50, 75, 100]
    assert dmme_amd.pf_grid(ab, 100) == list(range(1, 101))
    for sched in ("quadratic", "logsnr"):
        g = dmme_amd.pf_grid(ab, 10, sched)
        assert g[0] == 1 and g[-1] == 100 and all(b > a for a, b in zip(g, g[1:]))
    pf = dmme_amd.ProbabilityFlow(torch.nn.Identity(), 100, nodes=4)
    assert pf._grid == [1, 25, 50, 75, 100] and pf.chain_length() == 9 and pf.nodes == 5 and pf.t_min == 1
    src = dmme_amd.IDDPM(torch.nn.Identity(), 100) if hasattr(dmme_amd, "IDDPM") else None
    if src is not None:
        other = dmme_amd.ProbabilityFlow.from_process(src, nodes=4)
        assert torch.equal(other.alpha_bar, src.alpha_bar) and not torch.equal(other.alpha_bar, pf.alpha_bar)
    for bad in (dict(nodes=0), dict(t_min=0), dict(t_min=100), dict(schedule="cosine"), dict(grid=[1]), dict(grid=[5, 5, 100]), dict(grid=[0, 100]), dict(grid=[1, 101])):
        with pytest.raises(ValueError):
            dmme_amd.ProbabilityFlow(torch.nn.Identity(), 100, **bad)
    with pytest.raises(NotImplementedError):
        pf.sampling_step(None, None)


# ------------------------------------------------------------------------------------------ the analytic Gaussian problem
def test_gaussian_problem_is_second_order():
    """data N(0, 0.25 I), D = 192, T = 1000, the linear schedule: eps(x, t) = sqrt(1 - abar) x / (0.25 abar + 1 - abar) has a diagonal
    Jacobian, so a Rademacher probe is exact and the walk's log p can be held against log p_1(x_0) = log N(x_0; 0, (0.25 abar_1 + 1 - abar_1) I).
    Heun over all 999 steps is within 0.05 nats (measured: 0.009); the error ratio from 50 to 100 nodes lies in [3, 5] (measured 4.0):
    second order; Euler over all 999 steps is worse than Heun at 100 nodes"""
    import dmme_amd

    ab = R.alpha_bar(1000)
    x0 = 0.5 * synth.normal(7, (192,)).double().numpy()
    exact = R.gaussian_exact(ab, 1, x0)
    err = {n: R.gaussian_loglik(ab, dmme_amd.pf_grid(ab, n), x0) - exact for n in (50, 100, 1000)}
    euler = R.gaussian_loglik(ab, dmme_amd.pf_grid(ab, 1000), x0, euler=True) - exact
    print(f"gaussian problem: exact log p_1 {exact:.3f}; Heun error at 50 / 100 / 1000 nodes {err[50]:.4f} / {err[100]:.4f} / {err[1000]:.4f}, ratio "
          f"{err[50] / err[100]:.2f}; Euler at 1000 nodes {euler:.4f}")
    assert len(dmme_amd.pf_grid(ab, 1000)) == 1000
    assert abs(err[1000]) <= 0.05
    assert 3.0 <= err[50] / err[100] <= 5.0
    assert abs(euler) > abs(err[100])


# ------------------------------------------------------------------------------------------ the probe
def test_rademacher_restatement():
    """values are +-1; a numel that is no multiple of 4 cuts the last quad off; the span contract: the next span starts at the next
    counter; the mean over 2^16 values lies within 4 / 256 (four standard deviations)"""
    z = R.rademacher(0x1234567, (1 << 32) + 12, 105)
    assert z.dtype == np.float32 and z.shape == (105,) and set(np.unique(z)) == {-1.0, 1.0}
    full = R.rademacher(0x1234567, (1 << 32) + 12, 108)
    assert np.array_equal(full[:105], z)
    assert np.array_equal(R.rademacher(0x1234567, (1 << 32) + 12 + 26, 4), full[104:108])
    big = R.rademacher(99, 0, 1 << 16)
    assert abs(float(big.mean())) <= 4.0 / 256.0
    p2 = R.probe(5, 3, 2, 105, planes=2)
    assert p2.shape == (2, 210) and np.array_equal(p2[:, :105].reshape(-1), R.rademacher(5, 3, 210)) and not p2[:, 105:].any()
    x = synth.normal(1, (105,)).numpy()
    d = R.dequantize(x, 5, 3)
    assert d.dtype == np.float32 and float(np.abs(d - x).max()) <= 1.0 / 255.0 + 1e-7 and float(np.abs(d - x).max()) > 0.9 / 255.0


def test_plain_fp32_sits_inside_the_stage_bound():
    """the bound the GPU test holds the stage kernel to, shown on the host: a float32 evaluation of the four-term update (rounded
    product, three rounded multiply-adds) is inside 4 * 2^-24 * (|c0 x| + |c1 xs| + |c2 e| + |c3 es|) of float64, for an A row, a B row,
    the closing Euler row and a row with all four terms"""
    import dmme_amd

    rows, _ = dmme_amd.pf_rows(R.alpha_bar(100), GRID, "decode", likelihood=True)
    x, xs, e, es = (3.0 * synth.normal(10 + k, (2, 3, 32, 32)) for k in range(4))
    for row in (rows[9], rows[8], rows[1], np.array([0.7, -1.3, 0.2, 2.5, 0, 1, 0, 0])):
        row = row.astype(np.float32).astype(np.float64)
        want, _, _ = R.stage(x, xs, e, es, row, torch.float64)
        got, _, _ = R.stage(x, xs, e, es, row, torch.float32)
        bound = R.stage_bound(x, xs, e, es, row)
        err = (got.double() - want).abs()
        assert bool((err <= bound).all()) and float((err / bound).max()) > 0.01  # (inside, and not by orders of magnitude: the bound is no blank cheque)


def test_chain_draws_rule():
    """kind 14 draws exactly when a row has w != 0: the sampling and encoding tables leave torch's generator alone"""
    import dmme_amd
    from dmme_amd import _lib
    from dmme_amd.diffusion_models.chain import chain_draws

    pf = dmme_amd.ProbabilityFlow(torch.nn.Identity(), 100, grid=GRID)
    assert _lib.CHAIN_PFODE == 14
    assert chain_draws(_lib.CHAIN_PFODE, pf._tables["likelihood"][1])
    for name in ("decode", "decode_raw", "encode"):
        assert not chain_draws(_lib.CHAIN_PFODE, pf._tables[name][1])
    assert _lib.lib().dmme_version() >= 121


# ------------------------------------------------------------------------------------------ refusals, before anything touches the GPU
def _tiny(precision="fp32", cls=None):
    import dmme_amd

    kw = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=1, dropout=0.0, precision=precision)
    return (cls or dmme_amd.UNet)(**kw) if cls is None else cls(num_classes=5, **kw)


def test_process_refusals():
    """encode and log_likelihood refuse an x0 / v network, x0 thresholding, a class-conditional network, a network that is no dmme_amd
    UNet, train mode and fp16r32 - on CPU tensors, so nothing was launched; decode's tables exist for all of them"""
    import dmme_amd

    x = torch.zeros(1, 3, 8, 8)
    net = _tiny().eval()
    cases = [
        (dmme_amd.ProbabilityFlow(net, 100, 4, prediction="v"), NotImplementedError, "adapter"),
        (dmme_amd.ProbabilityFlow(net, 100, 4, prediction="x0"), NotImplementedError, "adapter"),
        (dmme_amd.ProbabilityFlow(net, 100, 4, threshold="static"), NotImplementedError, "clip"),
        (dmme_amd.ProbabilityFlow(net, 100, 4).set_threshold("dynamic", 0.9), NotImplementedError, "clip"),
        (dmme_amd.ProbabilityFlow(_tiny(cls=dmme_amd.ConditionalUNet).eval(), 100, 4), NotImplementedError, "class-conditional"),
        (dmme_amd.ProbabilityFlow(torch.nn.Identity(), 100, 4), RuntimeError, "dmme_amd UNet"),
        (dmme_amd.ProbabilityFlow(_tiny().train(), 100, 4), RuntimeError, "train mode"),
        (dmme_amd.ProbabilityFlow(_tiny("fp16r32").eval(), 100, 4), NotImplementedError, "fp16r32"),
    ]
    for proc, exc, msg in cases:
        assert proc.chain_length() == 9
        for call in (proc.encode, proc.log_likelihood, proc.bits_per_dim):
            with pytest.raises(exc, match=msg):
                call(x)
    with pytest.raises(ValueError):
        dmme_amd.ProbabilityFlow(net, 100, 4).log_likelihood(torch.zeros(3, 8, 8))


CFG = {k: os.path.join(ROOT, "configs", k, "cifar10.yaml") for k in ("ddpm", "ddim", "iddpm", "cfg", "vpred")}
HEUN = ["sample", "--config", CFG["ddpm"], "--sampler", "heun"]
EVAL = ["evaluate", "--config", CFG["ddpm"]]


@pytest.mark.parametrize("argv,msg", [
    (["fit", "--config", CFG["ddpm"], "--sampler", "heun"], "--sampler heun belongs to `sample`"),
    (HEUN + ["--eta", "0.5"], "--eta does not go with --sampler heun"),
    (HEUN + ["--steps", "3"], "--steps does not go with --sampler heun"),
    (HEUN + ["--labels", "3"], "--labels does not go with --sampler heun"),
    (HEUN + ["--sample-steps", "0"], "--sample-steps must be at least 1"),
    (HEUN + ["--nodes", "10"], "--nodes belongs to `evaluate`"),
    (HEUN + ["--solver-order", "1"], "--solver-order belongs to --sampler dpm++"),
    (["sample", "--config", CFG["ddpm"], "--dequantize"], "--dequantize belongs to `evaluate`"),
    (["sample", "--config", CFG["cfg"], "--sampler", "heun"], "--sampler heun needs an unconditional config"),
    (EVAL, "needs exactly one of --image X.npy"),
    (EVAL + ["--image", "x.npy", "--data", "config"], "needs exactly one of --image X.npy"),
    (EVAL + ["--image", "x.npy", "--sampler", "heun"], "--sampler does not go with `evaluate`"),
    (EVAL + ["--image", "x.npy", "--sampler", "dpm++"], "--sampler dpm++ belongs to `sample`"),
    (EVAL + ["--image", "x.npy", "--sample-steps", "5"], "--sample-steps does not go with `evaluate`"),
    (EVAL + ["--image", "x.npy", "--nodes", "0"], "--nodes must be at least 1"),
    (EVAL + ["--image", "x.npy", "--prediction", "v"], "--prediction v does not go with `evaluate`"),
    (EVAL + ["--image", "x.npy", "--threshold", "static"], "--threshold / --threshold-percentile belong to `sample`"),
    (EVAL + ["--image", "x.npy", "--precision", "fp16r32"], "--precision fp16r32 does not go with `evaluate`"),
    (EVAL + ["--image", "x.npy", "--mask", "m.npy"], "--mask belongs to --sampler repaint / sdedit"),
    (["evaluate", "--config", CFG["cfg"], "--data", "config"], "evaluate needs an unconditional config"),
])
def test_trainer_refuses_what_makes_no_sense(argv, msg):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value), exc.value


def test_trainer_builds_the_process_for_every_config():
    """what `sample --sampler heun` and `evaluate` put in place of the YAML's process, built on the host: the config's network, noise
    schedule (the iddpm config's cosine table too) and prediction, the flags' values and their defaults"""
    import argparse

    import dmme_amd
    from dmme_amd import trainer

    for name in ("ddpm", "ddim", "iddpm", "vpred"):
        module = trainer._instantiate(trainer.parse_config(CFG[name])["model_spec"])
        old = module.diffusion_model
        new = trainer._flow_process(module, argparse.Namespace(command="sample", sample_steps=None, nodes=None, tau_schedule=None), 50)
        assert isinstance(new, dmme_amd.ProbabilityFlow) and new.model is old.model and torch.equal(new.alpha_bar, old.alpha_bar), name
        assert new.prediction == old.prediction and new.schedule == "linear" and new._grid[0] == 1 and new._grid[-1] == old.timesteps and new.nodes == 51
    new = trainer._flow_process(module, argparse.Namespace(command="evaluate", sample_steps=None, nodes=12, tau_schedule="logsnr"), 100)
    assert new.schedule == "logsnr" and new.nodes <= 13 and new._grid[-1] == old.timesteps
    with pytest.raises(SystemExit) as exc:
        trainer._flow_process(module, argparse.Namespace(command="evaluate", sample_steps=None, nodes=10 ** 6, tau_schedule=None), 100)
    assert "nodes" in str(exc.value)
