"""CPU: Analytic-DPM's host side (dmme_amd.AnalyticDPM) - the variance table against the exact posterior variance of Gaussian data, the
hand-set tables it contains (G = 1: GeneralizedDDIM's rows bit for bit; G = 0: the paper's upper bound), the estimation schedule, the
state_dict round trip, the refusals, the ABI, and the float64 restatement's bounds (tests/analytic_ref.py) held against plain fp32 numpy."""

import numpy as np
import pytest
import torch

from oracle import synth

from . import analytic_ref as R


EPS64 = 2.0 ** -53


def _proc(T=100, K=10, schedule="linear", eta=1.0, **kw):
    import dmme_amd

    return dmme_amd.AnalyticDPM(torch.nn.Identity().eval(), T, K, schedule, eta, **kw)


def _cosine_abar(T, s=0.008):
    f = np.cos((np.arange(T + 1) / T + s) / (1 + s) * np.pi / 2) ** 2
    return np.clip(f / f[0], 1e-9, 1.0)


# ------------------------------------------------------------------------------------------ 1. the table on Gaussian data
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_table_equals_the_exact_gaussian_posterior_variance(schedule, eta):
    """x_0 ~ N(0, s2 I) under the optimal predictor: G = (1 - a) / (a s2 + 1 - a), and sigma_i^2 must be the exact Var(x_{tau_{i-1}} | x_{tau_i}),
    lambda^2 + c^2 / (1 / s2 + a / (1 - a)), to float64 round-off - for the package's table builder and for the restatement.  Round-off: the
    table takes G as a float64 number and forms 1 - G, which carries the relative error eps64 / (1 - G) of G's own rounding (it matters
    where abar is tiny, at the end of the cosine schedule); c is a difference of two roots A - r, each good to eps64, so c^2 carries
    4 eps64 (A + r) / |c| (it matters where eta = 0 and the steps are short), and so does the exact formula's c; a dozen further operations."""
    import dmme_amd

    T = 100
    ab = R.alpha_bar(T) if schedule == "linear" else _cosine_abar(T)
    worst = 0.0
    for K in (2, 10, T):
        tau = [int(v) for v in dmme_amd.equations.ddim.linear_tau(T, K)]
        for s2 in (0.25, 1.0, 3.0):
            G = R.gaussian_moments(ab, s2)
            got = dmme_amd.analytic_rows(ab, tau, eta, G)
            ref = R.table(ab, tau, eta, G)
            for i in range(1, K + 1):
                a, p = ab[tau[i]], ab[tau[i - 1]]
                want = R.gaussian_posterior_variance(a, p, ref["lam2"][i], s2)
                root, A = np.sqrt(max(1 - p - ref["lam2"][i], 0.0)), np.sqrt((1 - a) * p / a)
                cond = (A + root) / abs(A - root)
                for name, v in (("package", got[i][2]), ("restatement", ref["sigma2"][i])):
                    rel = abs(v - want) / want
                    worst = max(worst, rel)
                    assert rel <= 16 * EPS64 * (1.0 + 1.0 / (1.0 - G[tau[i]]) + cond), (name, schedule, eta, K, s2, i, v, want)
                assert abs(got[i][0] - ref["k0"][i]) <= 2 * EPS64 * ref["k0"][i] and abs(got[i][1] - ref["k1"][i]) <= 8 * EPS64 * (root + ref["k0"][i])
    print(f"{schedule} eta {eta}: largest relative distance from the exact posterior variance {worst:.2e}")


# ------------------------------------------------------------------------------------------ 2. the hand-set tables, the bounds
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("T,K", [(100, 10), (1000, 50), (100, 100)])
def test_hand_set_tables_recovered_and_bounds(T, K, eta):
    import dmme_amd

    proc = _proc(T, K, eta=eta)
    hand = dmme_amd.GeneralizedDDIM(torch.nn.Identity(), T, K, "linear", eta)
    proc.set_moments(np.ones(T + 1))
    assert proc.sampling_rows() == hand._rev_rows and proc._chain_tables() == hand._chain_tables() and proc.draws() == hand._draws
    v = proc.variances()
    assert np.array_equal(v[:, 0], v[:, 1])
    proc.set_moments(np.zeros(T + 1))
    v0 = proc.variances()
    assert np.array_equal(v0[:, 0], v0[:, 2]) 
    np.testing.assert_allclose(v0[:, 2], R.table(proc._ab64, proc._tau_host, eta, np.zeros(T + 1))["upper"], rtol=1e-13)
    rng = np.random.RandomState(3)
    proc.set_moments(rng.uniform(0.0, 1.0, T + 1))
    v = proc.variances()
    assert bool(np.all(v[1:, 1] <= v[1:, 0])) and bool(np.all(v[1:, 0] <= v[1:, 2])) and bool(np.all(v[1:, 0] > 0.0))
    rows = proc.sampling_rows()
    assert rows[1][2] == 0.0 and all(rows[i][2] == float(np.float32(np.sqrt(v[i, 0]))) for i in range(2, K + 1))  # the last step returns the mean
    assert all(rows[i][:2] == hand._rev_rows[i][:2] for i in range(K + 1))
    assert proc.draws()  # (at eta = 0 too: the optimal variance of a deterministic mean is not zero)


# ------------------------------------------------------------------------------------------ 3. schedule, round trip, refusals
@pytest.mark.parametrize("T,B,m", [(100, 8, 1), (100, 25, 3), (7, 16, 2), (12, 5, 64)])
def test_schedule_gives_every_timestep_the_same_count(T, B, m):
    import dmme_amd

    passes = dmme_amd.moment_schedule(T, B, m)
    assert len(passes) == -(-T * m // B) and all(len(p) == B for p in passes[:-1]) and 1 <= len(passes[-1]) <= B
    if T % B == 0:
        assert len(passes) == (T // B) * m
    for k, p in enumerate(passes):
        assert np.array_equal(p, 1 + (np.arange(len(p)) + k * B) % T)
    counts = np.bincount(np.concatenate(passes), minlength=T + 1)
    assert counts[0] == 0 and bool(np.all(counts[1:] == m))


def test_tensor_data_is_walked_with_a_shift_per_sweep():
    """n == T: without the shift timestep t would meet image t - 1 in every sweep; with it, m sweeps show it m different images.  n and T
    with a common factor: a timestep's images leave its residue class.  One sweep (m = 1) is the plain cyclic walk."""
    from dmme_amd.diffusion_models.analytic import moment_images

    T, m = 12, 5
    for n in (12, 8, 4, 7):
        idx = moment_images(0, T * m, T, n).reshape(m, T)
        assert np.array_equal(idx[0], np.arange(T) % n)
        for t in range(T):
            assert len(set(idx[:, t].tolist())) == min(m, n), (n, t, idx[:, t])
        assert np.array_equal(np.concatenate([moment_images(0, 17, T, n), moment_images(17, T * m - 17, T, n)]), idx.reshape(-1))  # any batching


def test_state_dict_round_trip_and_runner_key():
    import dmme_amd

    T, K = 100, 10
    a = _proc(T, K)
    assert a.tau_schedule == "linear" and a.eta == 1.0  # the defaults of this class
    assert isinstance(a, dmme_amd.GeneralizedDDIM) and "AnalyticDPM" in dmme_amd.__all__
    assert sorted(a.state_dict()) == ["_g_count", "_g_sum"] and a._g_sum.dtype == torch.float64 and a._g_count.dtype == torch.int64
    assert tuple(a._g_sum.shape) == tuple(a._g_count.shape) == (T + 1,)
    assert "_g_sum" not in dmme_amd.GeneralizedDDIM(torch.nn.Identity(), T, K, "linear", 1.0).state_dict()
    G = np.random.RandomState(1).uniform(0.1, 0.9, T + 1)
    a.set_moments(G)
    np.testing.assert_array_equal(a.moments()[1:], G[1:])
    assert np.isnan(a.moments()[0])
    a._g_sum[5], a._g_count[5] = 9.0, 4  # a mean above 1 is clipped
    assert a.moments()[5] == 1.0
    a.set_moments(G)
    b = _proc(T, K)
    v0 = b._table_version
    b.load_state_dict(a.state_dict())
    assert torch.equal(b._g_sum, a._g_sum) and torch.equal(b._g_count, a._g_count) and b.sampling_rows() == a.sampling_rows()
    assert b._table_version > v0  # a runner captured over the old table is not reused
    lit = dmme_amd.LitDDIM(diffusion_model=a)
    assert "diffusion_model._g_sum" in lit.state_dict() and "diffusion_model._g_count" in lit.state_dict()
    v = a._table_version
    a.set_moments(np.full(T + 1, 0.5))
    assert a._table_version == v + 1 and a.sampling_rows() != b.sampling_rows()


def test_refusals():
    import dmme_amd

    with pytest.raises(ValueError, match="not strictly increasing"):
        _proc(1000, 50, "quadratic")  # tau_1 = round(1000 / 2500) = 0
    with pytest.raises(ValueError, match="not strictly increasing"):
        _proc(10, 10, "quadratic")
    _proc(1000, 20, "quadratic")  # (tau_1 = 2: fine)
    with pytest.raises(ValueError, match="eta"):
        _proc(eta=1.5)
    p = _proc(100, 10)
    with pytest.raises(RuntimeError, match="timestep 10 "):
        p._chain_tables()
    G = np.full(101, 0.5)
    p.set_moments(G)
    p._g_count[30] = 0
    p._moments_changed()
    with pytest.raises(RuntimeError, match="timestep 30 "):
        p._chain_tables()
    p._g_count[30], p._g_count[31] = 1, 0  # a timestep off the grid is not needed
    p._moments_changed()
    assert len(p.sampling_rows()) == 11
    with pytest.raises(ValueError, match="set_moments"):
        p.set_moments(np.full(100, 0.5))
    with pytest.raises(ValueError, match="set_moments"):
        p.set_moments(np.full(101, 1.5))
    half = _proc(100, 10, eta=0.5).set_moments(G)
    with pytest.raises(ValueError, match="eta = 1"):
        half.bits_per_dim(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="variance"):
        p.bits_per_dim(torch.zeros(1, 3, 8, 8), variance="learned")
    with pytest.raises(RuntimeError, match="GPU"):
        p.estimate_moments(torch.zeros(4, 3, 8, 8))
    p.model.train()  # a network that draws dropout masks is not the one that samples
    with pytest.raises(RuntimeError, match="train mode"):
        p.estimate_moments(torch.zeros(4, 3, 8, 8))
    with pytest.raises(RuntimeError, match="train mode"):
        p.bits_per_dim(torch.zeros(1, 3, 8, 8))
    p.model.eval()
    p.set_moments(G)
    assert int(p._g_count.sum()) == 100 and int(p.reset_moments()._g_count.sum()) == 0 and float(p._g_sum.abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="timestep 10 "):
        p.sampling_rows()
    with pytest.raises(ValueError):
        dmme_amd.moment_schedule(10, 0, 1)


def test_trainer_flags_are_checked_before_anything_touches_the_gpu():
    import os

    from dmme_amd import trainer

    cfg = ["--config", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "ddpm", "cifar10.yaml")]
    an = ["--sampler", "analytic"]
    for argv, msg in ((["sample", "--variance", "beta"], "belongs to --sampler analytic"), (["sample", "--moments", "g.npy", "--moment-images", "4"], "belong to --sampler analytic"),
                      (["fit"] + an, "belongs to `sample` and `evaluate`"), (["sample"] + an + ["--variance", "beta"], "--variance belongs to `evaluate`"),
                      (["sample"] + an + ["--tau-schedule", "logsnr"], "logsnr"), (["sample"] + an + ["--steps", "3"], "--steps does not go"),
                      (["sample"] + an + ["--moments", "g.npy", "--moment-images", "4", "--data", "config"], "give one of them"), (["sample"] + an + ["--sample-steps", "0"], "at least 1"), (["sample"] + an + ["--moment-images", "4"], "needs --data config"),
                      (["sample"] + an + ["--eta", "1.5"], "outside"), (["evaluate"] + an + ["--eta", "0.5", "--image", "x.npy"], "eta = 1"),
                      (["evaluate"] + an, "needs --image"), (["evaluate"] + an + ["--nodes", "10", "--image", "x.npy"], "probability-flow likelihood")):
        with pytest.raises(SystemExit, match=msg):
            trainer.main(argv + cfg)


def test_vlb_table_columns():
    """the device table of the bound: the mean's scalars are the sampling row's, column 2 holds the variance asked for, column 3 the
    posterior's, columns 4 and 5 dmme_q_sample's own fp32 tables; the floors at i = 1"""
    T, K = 100, 5
    p = _proc(T, K).set_moments(np.linspace(1.0, 0.2, T + 1))
    ref = R.table(p._ab64, p._tau_host, 1.0, p.moments())
    ab, tau = p._ab64, p._tau_host
    for variance, want in (("analytic", ref["sigma2"]), ("beta", np.array([0.0] + [1 - ab[tau[i]] / ab[tau[i - 1]] for i in range(1, K + 1)])), ("beta-tilde", ref["lam2"])):
        tab = p._vlb_table(variance)
        assert tab.dtype == np.float32 and tab.shape == (K + 1, 8)
        for i in range(1, K + 1):
            assert tab[i, 0] == p.sampling_rows()[i][0] and tab[i, 1] == p.sampling_rows()[i][1]
            assert tab[i, 2] == np.float32(np.log(max(want[i], 1e-12))) and tab[i, 3] == np.float32(np.log(max(ref["lam2"][i], 1e-12)))
            assert tab[i, 4] == p._sqrt_alpha_bar[tau[i]].item() and tab[i, 5] == p._sqrt_one_minus_alpha_bar[tau[i]].item()
    assert p._vlb_table("beta-tilde")[1, 2] == np.float32(np.log(1e-12))


def test_abi():
    import ctypes as C

    from dmme_amd import _lib

    lib = _lib.lib()
    assert lib.dmme_version() >= 122
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    moment = lambda **kw: lib.dmme_analytic_moment(*[kw.get(k, d) for k, d in (
        ("out", p), ("stride", 16), ("t", p), ("T", 10), ("B", 1), ("chw", 16), ("sum", p), ("count", p), ("rows", None), ("status", None), ("scratch", p), ("stream", None))])
    for bad in (dict(out=None), dict(t=None), dict(sum=None), dict(count=None), dict(scratch=None), dict(B=0), dict(chw=0), dict(T=0), dict(stride=15)):
        assert moment(**bad) == -1 and b"analytic_moment" in lib.dmme_last_error(), bad
    rows = lambda **kw: lib.dmme_analytic_vlb_rows(*[kw.get(k, d) for k, d in (
        ("out", p), ("stride", 16), ("x_t", p), ("x_0", p), ("idx", p), ("coef", p), ("S", 5), ("B", 1), ("chw", 16), ("rows", p), ("status", None), ("scratch", p),
        ("stream", None))])
    for bad in (dict(out=None), dict(x_t=None), dict(x_0=None), dict(idx=None), dict(coef=None), dict(rows=None), dict(scratch=None), dict(B=0), dict(chw=0), dict(S=0),
                dict(stride=8)):
        assert rows(**bad) == -1 and b"analytic_vlb_rows" in lib.dmme_last_error(), bad


# ------------------------------------------------------------------------------------------ 4. the restatement's bounds against plain fp32
def _pixel_grid(seed, shape):
    k = synth.randint(seed, 0, 256, int(np.prod(shape))).reshape(shape).to(torch.float32)
    for b in range(shape[0]):  # both ends in every image (the open-ended bins of the discrete NLL)
        k[b].reshape(-1)[0], k[b].reshape(-1)[1] = 255.0, 0.0
    return (k / 127.5 - 1.0).numpy()


@pytest.mark.parametrize("chw", [105, 3072])
def test_fp32_rows_sit_inside_the_derived_bounds(chw):
    """the KL and NLL rows in plain fp32 numpy, in the device's order of operations, against float64 under kl_bound / nll_bound, for the rows
    of a 5-step and of a 100-step table over T = 100 and for all three variances.  "beta-tilde" at i = 1 is the floored variance 1e-12: every
    bin probability sits at the floor of the logarithm or next to it, where the row has no finite bound (and no meaning); it is left out."""
    B = 3
    x0 = _pixel_grid(1, (B, chw))
    worst = {"kl": 0.0, "nll": 0.0}
    for K in (5, 100):
        p = _proc(100, K).set_moments(np.linspace(0.95, 0.3, 101))
        for variance in ("analytic", "beta", "beta-tilde"):
            tab = p._vlb_table(variance)
            for i in sorted({1, 2, K // 2 + 1, K} - ({1} if variance == "beta-tilde" else set())):
                row = tab[i]
                z = synth.normal(10 + i, (B, chw)).numpy()
                x_t = (row[R.SA] * x0 + row[R.S1] * z).astype(np.float32)
                e = (z + 0.3 * synth.normal(50 + i, (B, chw)).numpy()).astype(np.float32)
                if i == 1:
                    got, want, bound = R.nll_row_f32(e, x_t, x0, row), R.nll_row(e, x_t, x0, row), R.nll_bound_analytic(e, x_t, x0, row)
                else:
                    got, want, bound = R.kl_row_f32(e, x_t, x0, row), R.kl_row(e, x_t, x0, row), R.kl_bound(e, x_t, x0, row)
                err = np.abs(got.astype(np.float64) - want)
                assert bool(np.all(np.isfinite(bound))) and bool(np.all(bound <= 1e-3 * np.abs(want) + 1e-6)), (K, variance, i, bound, want)  # the bound says something
                assert bool(np.all(err <= bound)), (K, variance, i, err, bound)
                key = "nll" if i == 1 else "kl"
                worst[key] = max(worst[key], float((err / bound).max()))
            if variance == "beta-tilde":  # sd = 1e-6: the elements are counted (some means are put inside their bin, one next to an edge)
                row = tab[1]
                z = synth.normal(11, (B, chw)).numpy()
                e = z.astype(np.float32)
                x_t = ((x0 - row[R.K1] * e) / row[R.K0]).astype(np.float32)  # mean = x0 up to rounding ...
                x_t[:, ::3] += np.float32(0.5)                                # ... one element in three far above its bin (but where x0 = 1: the open top bin holds it still)
                x_t[:, 1] += np.float32(1.0 / 255.0) / row[R.K0]              # ... and one on the bin's edge
                lo, hi, n_out, n_und = R.nll_saturated_interval(e, x_t, x0, row)
                got = R.nll_row_f32(e, x_t, x0, row).astype(np.float64)
                assert bool(np.all(lo * (1 - 4 * R.U) <= got)) and bool(np.all(got <= hi * (1 + 4 * R.U))), (K, lo, got, hi)
                assert bool(np.all(n_out >= 0.95 * (chw // 3))) and bool(np.all(n_out < chw)) and bool(np.all(n_und >= 1)) and bool(np.all(n_und <= 0.05 * chw + 2)), (n_out, n_und)
    print(f"chw {chw}: largest err / bound: KL {worst['kl']:.3f}, NLL {worst['nll']:.3f}")


def test_moment_bound_and_ordered_accumulation():
    e = synth.normal(4, (5, 3072)).numpy()
    got = (e.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32).astype(np.float64) / 3072
    assert bool(np.all(np.abs(got - R.moment(e)) <= R.moment_bound(e)))
    assert R.sum_depth(105) == 1 + 10 and R.sum_depth(3072) == 4 + 10 and R.sum_depth(1 << 20) == 128 + 10
    T = 10
    sums, counts = np.zeros(T + 1), np.zeros(T + 1, dtype=np.int64)
    m = np.array([0.1, 0.2, 0.4, 0.8, 1.6])
    assert R.accumulate(sums, counts, [3, 7, 3, 1, 7], m, T) == 0
    assert sums[3] == 0.1 + 0.4 and sums[7] == 0.2 + 1.6 and sums[1] == 0.8 and counts.tolist() == [0, 1, 0, 2, 0, 0, 0, 2, 0, 0, 0]
    assert R.accumulate(sums, counts, [0, T + 1, 2], m[:3], T) == 1 and counts[2] == 1 and sums[2] == 0.4 and counts.sum() == 6
    # the restatement's accumulation over the package's schedule: every timestep is counted images_per_timestep times, in any batching
    import dmme_amd

    for B in (3, 10, 16):
        sums, counts = np.zeros(T + 1), np.zeros(T + 1, dtype=np.int64)
        for t in dmme_amd.moment_schedule(T, B, 4):
            assert R.accumulate(sums, counts, t, np.full(len(t), 0.25), T) == 0
        assert counts.tolist() == [0] + [4] * T and np.array_equal(sums[1:], np.ones(T))
