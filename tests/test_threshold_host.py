"""CPU: the host side of x0 thresholding - the restatement's quantile against numpy.quantile, the table against float64, the (k, frac)
edge cases, argument validation of the constructors and `set_threshold`, the runner key, and the trainer's flag refusals."""

import os

import numpy as np
import pytest
import torch

from . import pred_ref as PR
from . import threshold_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {n: os.path.join(ROOT, "configs", n, "cifar10.yaml") for n in ("ddpm", "ddim", "iddpm", "cfg", "vpred")}
Q_RTOL = 4 * 2.0**-24  # four float32 roundings between the exact order statistics and q: frac, the gap, the product, the sum


@pytest.mark.parametrize("n", [1, 2, 5, 192, 3072, 12288])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.995, 1.0, 0.3333])
def test_float32_quantile_against_numpy(n, p):
    rng = np.random.RandomState(n)
    for scale, quant in ((1.0, None), (40.0, None), (1.0, 8.0)):
        a = np.abs(rng.standard_normal(n) * scale).astype(np.float32)
        if quant:
            a = (np.round(a * quant) / quant).astype(np.float32)  # heavy ties
        got, ak, ak1 = R.quantile32(a, p)
        want = np.quantile(a.astype(np.float64), p, method="linear")
        assert got.dtype == np.float32
        assert abs(float(got) - want) <= Q_RTOL * abs(want), (n, p, scale, quant, float(got), want)
        srt = np.sort(a)
        k, frac = R.rank(p, n)
        assert ak == srt[k] and (ak1 is None) == (frac == 0) and (ak1 is None or ak1 == srt[k + 1])


def test_rank_edge_cases():
    """p = 1, p = 0, n = 1 and an integral p (n - 1): frac is exactly 0 there, so a_{k+1} (which may not exist) is never read; the
    package's `threshold_rank` is the restatement's"""
    from dmme_amd.diffusion_models.ddpm import threshold_rank

    for n in (1, 2, 5, 3072, 3 * 256 * 256):
        assert R.rank(1.0, n) == (n - 1, 0.0) and R.rank(0.0, n) == (0, 0.0)
    assert R.rank(0.5, 1) == (0, 0.0) and R.rank(0.995, 1) == (0, 0.0)
    assert R.rank(0.5, 5) == (2, 0.0) and R.rank(0.25, 9) == (2, 0.0) and R.rank(0.75, 3073) == (2304, 0.0)
    k, frac = R.rank(0.995, 3072)
    assert k == 3055 and frac == np.float32(0.995 * 3071 - 3055) and 0 < frac < 1
    for n in (1, 2, 5, 192, 3072, 36864, 3 * 256 * 256):
        for p in (0.0, 0.5, 0.995, 1.0, 1.0 / 3.0):
            k, frac = threshold_rank(p, n)
            rk, rfrac = R.rank(p, n)
            assert (k, np.float32(frac)) == (rk, rfrac) and isinstance(k, int) and isinstance(frac, float)
            assert 0 <= k < n and 0.0 <= frac <= 1.0 and (k + 1 < n or frac == 0.0)
    for p in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            threshold_rank(p, 10)


def test_table_rows_against_float64():
    """the [T+1][4] table a process registers: the float64 formulas over its own alpha_bar rounded once - bit for bit, the NaN row
    included - on the linear schedule, on a cosine one installed later, and on IDDPM's own; the rows invert each other in float64"""
    import dmme_amd
    from dmme_amd.diffusion_models.ddpm import threshold_table

    net = torch.nn.Identity()
    lin = dmme_amd.DDPM(net, 1000, threshold="static")
    cos = dmme_amd.DDPM(net, 1000, threshold="dynamic")
    cos._use_alpha_bar(torch.from_numpy(PR.cosine_alpha_bar(1000)).to(torch.float32))
    idd = dmme_amd.IDDPM(net, 1000).set_threshold("dynamic", 0.9)
    for p in (lin, cos, idd):
        ab = p.alpha_bar.reshape(-1).double().numpy()
        got = p._thr_tab.numpy().reshape(-1, 4)
        want = R.table64(ab)
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32), equal_nan=True)
        assert np.isnan(got[0]).all() and np.isfinite(got[1:]).all()
        np.testing.assert_allclose(threshold_table(ab), want, rtol=1e-15, equal_nan=True)
        A, B, C, D = want[1:].T
        sa, sd = np.sqrt(ab[1:]), np.sqrt(1 - ab[1:])
        np.testing.assert_allclose(A * sa, 1.0, rtol=1e-14)
        np.testing.assert_allclose(B * sa, sd, rtol=1e-14)
        np.testing.assert_allclose(C * sd, 1.0, rtol=1e-14)
        np.testing.assert_allclose(D * sd, sa, rtol=1e-14)
        assert "_thr_tab" not in p.state_dict()
    assert idd.threshold_percentile == 0.9
    # float64 round trip through the stage's two maps: eps -> x0 -> eps
    rng = np.random.RandomState(0)
    x, e = rng.standard_normal(1000), rng.standard_normal(1000)
    tab = R.table64(lin.alpha_bar.reshape(-1).double().numpy())[1:]
    x0 = tab[:, 0] * x - tab[:, 1] * e
    np.testing.assert_allclose(tab[:, 2] * x - tab[:, 3] * x0, e, rtol=0, atol=1e-9 * np.abs(tab[:, 3] * x0).max())


def test_restatement_properties():
    """what the design promises, on the restatement itself: an image that is never clipped keeps its bits, dynamic mode with a quantile
    at or below 1 equals static mode, the float32 and float64 forms agree, and the clipped x0 the rewritten eps implies is in [-1, 1]"""
    ab = PR.linear_alpha_bar(1000)
    t32, t64 = R.table32(ab), R.table64(ab)
    rng = np.random.RandomState(1)
    B, chw, t = 3, 192, [1, 500, 1000]
    x = rng.standard_normal((B, chw)).astype(np.float32)
    e = rng.standard_normal((B, chw)).astype(np.float32)
    for mode, p in ((R.STATIC, None), (R.DYNAMIC, 0.5), (R.DYNAMIC, 0.995)):
        got, info = R.threshold(mode, e, x, t32, t, p)
        want, info64 = R.threshold(mode, e, x, t64, t, p, dtype=np.float64)
        assert got.dtype == np.float32 and want.dtype == np.float64
        keep = ~info["mask"]
        assert np.array_equal(got[keep].view(np.uint32), e[keep].view(np.uint32))
        # the x0 the new eps implies, in float64, is the clamped and rescaled one
        for b in range(B):
            A, Bc = t64[t[b], 0], t64[t[b], 1]
            x0_new = A * x[b].astype(np.float64) - Bc * want[b]
            assert np.abs(x0_new).max() <= 1.0 + 1e-9 * max(1.0, Bc * np.abs(want[b]).max())
    small = (e * 0).astype(np.float32), (x * np.float32(0.2)).astype(np.float32)
    st, _ = R.threshold(R.STATIC, small[0], small[1], t32, [1], None)
    dy, info = R.threshold(R.DYNAMIC, small[0], small[1], t32, [1], 0.995)
    assert (info["s"] == 1).all() and np.array_equal(st.view(np.uint32), dy.view(np.uint32))


def test_argument_validation():
    import dmme_amd
    from dmme_amd import _lib

    net = torch.nn.Identity()
    for kw in (dict(threshold="clip"), dict(threshold="Static"), dict(threshold=None), dict(threshold_percentile=1.5), dict(threshold_percentile=-0.1),
               dict(threshold_percentile=float("nan")), dict(threshold_percentile="0.9"), dict(threshold_percentile=True)):
        with pytest.raises(ValueError):
            dmme_amd.DDPM(net, 10, **kw)
    with pytest.raises(TypeError):
        dmme_amd.DDPM(net, 10, 1e-4, 0.02, "eps", "uniform", 5.0, "static")  # keyword-only
    p = dmme_amd.DDPM(net, 10)
    assert (p.threshold, p.threshold_percentile, p._thr) == ("none", 0.995, _lib.THRESHOLD_NONE) and not hasattr(p, "_thr_tab")
    for bad in (("clip", None), ("dynamic", 2.0), ("dynamic", -1.0), ("static", "x")):
        with pytest.raises(ValueError):
            p.set_threshold(*bad)
    assert (p.threshold, p._thr) == ("none", _lib.THRESHOLD_NONE)  # a refused setting changes nothing
    assert p.set_threshold("dynamic", 0.9) is p and (p.threshold, p.threshold_percentile, p._thr) == ("dynamic", 0.9, _lib.THRESHOLD_DYNAMIC)
    assert p.set_threshold("static").threshold_percentile == 0.9 and p._thr == _lib.THRESHOLD_STATIC and p._thr_tab.numel() == 4 * 11
    assert p.set_threshold("none")._thr == _lib.THRESHOLD_NONE
    # every constructor that passes prediction= passes the thresholding too, and from_process copies it
    kw = dict(threshold="dynamic", threshold_percentile=0.75)
    tiny = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    cond = dmme_amd.ConditionalUNet(num_classes=3, **tiny)
    clf = dmme_amd.EncoderClassifier(num_classes=3, **tiny)
    procs = [dmme_amd.DDIM(net, 20, 5, **kw), dmme_amd.GeneralizedDDIM(net, 20, 5, eta=0.5, **kw), dmme_amd.DPMSolverPP(net, 20, 5, **kw), dmme_amd.RePaint(net, 20, 10, 2, 2, **kw),
             dmme_amd.ClassifierFreeDDPM(cond, 20, **kw), dmme_amd.ClassifierFreeDDIM(cond, 20, 5, **kw), dmme_amd.ClassifierFreeDPMSolver(cond, 20, 5, **kw),
             dmme_amd.ClassifierGuidedDDPM(net, clf, 20, **kw), dmme_amd.ClassifierGuidedDDIM(net, clf, 20, 5, **kw)]
    for q in procs:
        assert (q.threshold, q.threshold_percentile, q._thr) == ("dynamic", 0.75, _lib.THRESHOLD_DYNAMIC), type(q).__name__
        ab = q.alpha_bar.reshape(-1).double().numpy()
        assert np.array_equal(q._thr_tab.numpy().reshape(-1, 4), R.table32(ab), equal_nan=True), type(q).__name__
    base = dmme_amd.IDDPM(net, 20).set_threshold("static")
    for q in (dmme_amd.DPMSolverPP.from_process(base, sub_timesteps=5), dmme_amd.RePaint.from_process(base, sub_timesteps=10, jump_length=2, resamples=2)):
        assert q.threshold == "static" and np.array_equal(q._thr_tab.numpy(), base._thr_tab.numpy(), equal_nan=True)
    assert dmme_amd.DPMSolverPP.from_process(base, sub_timesteps=5, threshold="none").threshold == "none"
    # DPMSolverPP's own clip stays what it was, next to the new setting
    both = dmme_amd.DPMSolverPP(net, 20, 5, clip_x0=True, threshold="static")
    assert both.clip_x0 is True and both._rows[1][5] == 1.0 and dmme_amd.DPMSolverPP(net, 20, 5, threshold="static")._rows[1][5] == 0.0


def test_runner_key_changes_with_the_setting():
    import dmme_amd

    class Net(torch.nn.Identity):
        _dtype = 0

    p = dmme_amd.DDPM(Net(), 10)
    x = torch.zeros(2, 3, 4, 4)
    keys = [p._runner_key(x, True)]
    for mode, pct in (("static", None), ("dynamic", None), ("dynamic", 0.9), ("none", None)):
        p.set_threshold(mode, pct)
        keys.append(p._runner_key(x, True))
    assert len(set(keys[:4])) == 4 and keys[4] != keys[0]  # (the percentile stays 0.9 behind "none": one more runner at the most)
    p.set_threshold("none", 0.995)
    assert p._runner_key(x, True) == keys[0]
    cond = dmme_amd.ConditionalUNet(num_classes=3, pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    c = dmme_amd.ClassifierFreeDDPM(cond, 10, guidance_scale=2.5)
    k0 = c._runner_key(x, True)
    assert c.set_threshold("dynamic")._runner_key(x, True) != k0 and k0[-1] == 2.5


@pytest.mark.parametrize("argv,msg", [
    (["fit", "--config", CFG["ddpm"], "--threshold", "static"], "belong to `sample`"),
    (["fit", "--config", CFG["cfg"], "--threshold-percentile", "0.9"], "belong to `sample`"),
    (["sample", "--config", CFG["ddpm"], "--threshold-percentile", "0.9"], "belongs to --threshold dynamic"),
    (["sample", "--config", CFG["ddpm"], "--threshold", "static", "--threshold-percentile", "0.9"], "belongs to --threshold dynamic"),
    (["sample", "--config", CFG["iddpm"], "--threshold", "dynamic", "--threshold-percentile", "1.5"], "outside [0, 1]"),
    (["sample", "--config", CFG["ddim"], "--sampler", "ddim-paper", "--threshold", "dynamic", "--threshold-percentile", "-0.5"], "outside [0, 1]"),
])
def test_trainer_refusals_through_main(argv, msg):
    """exits with a message before the configuration is read or a GPU is touched, like the solver's flag checks"""
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(argv)
    assert msg in str(exc.value)


def test_trainer_refuses_an_unknown_mode(capsys):
    from dmme_amd import trainer

    with pytest.raises(SystemExit) as exc:
        trainer.main(["sample", "--config", CFG["ddpm"], "--threshold", "clip"])
    assert exc.value.code == 2 and "--threshold" in capsys.readouterr().err
