"""-m gpu: Improved DDPM as published (Nichol & Dhariwal 2021) - the per-image loss rows (dmme_iddpm_loss_rows), the prior term
(dmme_iddpm_prior_rows), the loss-second-moment resampler (dmme_tsampler_draw / dmme_tsampler_update), and through the public
interface the strided sampling chain, the importance-weighted training step and `bits_per_dim` - against oracle/iddpm.py, the
existing dmme_iddpm_loss and the float64 restatement tests/iddpm_paper_ref.py."""

import math

import numpy as np
import pytest
import torch

from oracle import iddpm as OI
from oracle import synth

from . import iddpm_paper_ref as R
from . import philox_ref as P

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
T_ROWS, B_ROWS = 100, 5
T_OF_ROW = [1, 1, 2, T_ROWS, 7]
SHAPES = {75: (5, 5), 3072: (32, 32), 12288: (64, 64)}  # chw -> (h, w): ragged and below one block; several passes per thread; the 64x64 image


# ------------------------------------------------------------------------------------------ helpers
def _coef(T, schedule):
    import dmme_amd

    return dmme_amd.IDDPM(torch.nn.Identity(), T, schedule=schedule)._coef.cuda().contiguous()


def _pixel_grid(seed, shape):
    """x_0 on the 8-bit grid k/127.5 - 1, both ends present"""
    k = synth.randint(seed, 0, 256, int(np.prod(shape))).reshape(shape).to(torch.float32)
    k.reshape(-1)[0], k.reshape(-1)[1] = 0.0, 255.0
    for b in range(shape[0]):  # both ends in every image (the open-ended bins of the discrete NLL)
        k[b].reshape(-1)[2], k[b].reshape(-1)[3] = 255.0, 0.0
    return k / 127.5 - 1.0


def _inputs(chw, B=B_ROWS, seed=0):
    h, w = SHAPES[chw]
    mo = 0.5 * synth.normal(900 + seed, (B, 6, h, w))
    x_t = synth.normal(901 + seed, (B, 3, h, w))
    tgt = synth.normal(902 + seed, (B, 3, h, w))
    x0 = _pixel_grid(903 + seed, (B, 3, h, w))
    return mo, x_t, x0, tgt


def _loss_old(mo, x_t, x0, tgt, t, coef, w_simple, w_vlb, want_grad=True):
    from dmme_amd import _lib

    B = mo.size(0)
    loss = torch.empty(3, device="cuda")
    d_out = torch.full_like(mo, 7.0) if want_grad else None
    scratch = torch.empty(1024, device="cuda")
    _lib.check(_lib.lib().dmme_iddpm_loss(_lib.ptr(mo), _lib.ptr(x_t), _lib.ptr(x0), _lib.ptr(tgt), _lib.ptr(t), _lib.ptr(coef), B, x_t[0].numel(),
                                          w_simple, w_vlb, _lib.ptr(loss), _lib.ptr(d_out), 1.0, _lib.ptr(scratch), _lib.stream_ptr()))
    return loss, d_out


def _loss_rows(mo, x_t, x0, tgt, t, coef, T, w_simple, w_vlb, weight=None, want_grad=True):
    from dmme_amd import _lib

    B = mo.size(0)
    loss = torch.empty(3, device="cuda")
    rows = torch.empty((3, B), device="cuda")
    d_out = torch.full_like(mo, 7.0) if want_grad else None
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(64 * B, device="cuda")
    _lib.check(_lib.lib().dmme_iddpm_loss_rows(_lib.ptr(mo), _lib.ptr(x_t), _lib.ptr(x0), _lib.ptr(tgt), _lib.ptr(t), _lib.ptr(coef), T, _lib.ptr(weight), B,
                                               x_t[0].numel(), w_simple, w_vlb, _lib.ptr(loss), _lib.ptr(rows), _lib.ptr(d_out), 1.0, _lib.ptr(status),
                                               _lib.ptr(scratch), _lib.stream_ptr()))
    return loss, rows, d_out, int(status.item())


def _oracle_rows(mo, x_t, x0, tgt, t, tabs):
    """(S_b, V_b) image by image on the CPU: the plain MSE and oracle.iddpm.loss_vlb"""
    beta, alpha, abar = tabs
    S, V = [], []
    for b in range(mo.size(0)):
        tb = t[b : b + 1]
        bt, at, ab, abp = OI._col(beta, tb), OI._col(alpha, tb), OI._col(abar, tb), OI._col(abar, tb - 1)
        eps, var = OI.forward_model(mo[b : b + 1], bt, ab, abp)
        S.append(float(torch.mean((tgt[b : b + 1] - eps) ** 2)))
        V.append(float(OI.loss_vlb(eps, var, x_t[b : b + 1], tb, x0[b : b + 1], bt, at, ab, abp)))
    return np.array(S), np.array(V)


def _assert_rows_close(got, want, t, what):
    """rtol 2e-5 (the project's tolerance for this loss), 5e-4 for the ill-conditioned t == 1 rows"""
    for b, tb in enumerate(t):
        rtol = 5e-4 if tb == 1 else 2e-5
        print(f"{what}[{b}] t={tb}: got {got[b]:.9g} want {want[b]:.9g} rel {abs(got[b] - want[b]) / abs(want[b]):.2e} (<= {rtol})")
    for b, tb in enumerate(t):
        np.testing.assert_allclose(got[b], want[b], rtol=5e-4 if tb == 1 else 2e-5, err_msg=f"{what}[{b}] t={tb}")


# ------------------------------------------------------------------------------------------ A1: dmme_iddpm_loss_rows
@pytest.mark.parametrize("schedule", ["cosine", "linear"])
@pytest.mark.parametrize("chw", sorted(SHAPES))
def test_loss_rows_without_weights_equals_the_existing_kernel(chw, schedule):
    """same per-element arithmetic: d_out bit for bit; the three means differ in summation order only (rtol 2e-5)"""
    coef = _coef(T_ROWS, schedule)
    mo, x_t, x0, tgt = (v.cuda() for v in _inputs(chw))
    t = torch.tensor(T_OF_ROW).cuda()
    for w_simple, w_vlb in ((1.0, 0.05), (0.0, 1.0)):
        want_loss, want_d = _loss_old(mo, x_t, x0, tgt, t, coef, w_simple, w_vlb)
        loss, rows, d_out, status = _loss_rows(mo, x_t, x0, tgt, t, coef, T_ROWS, w_simple, w_vlb)
        assert status == 0
        assert torch.equal(d_out, want_d)
        print(f"chw {chw} {schedule} w=({w_simple}, {w_vlb}): loss {loss.tolist()} existing {want_loss.tolist()}")
        np.testing.assert_allclose(loss.cpu().numpy(), want_loss.cpu().numpy(), rtol=2e-5)


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
@pytest.mark.parametrize("chw", sorted(SHAPES))
def test_loss_rows_vs_oracle_image_by_image(chw, schedule):
    coef = _coef(T_ROWS, schedule)
    mo, x_t, x0, tgt = _inputs(chw)
    S, V = _oracle_rows(mo, x_t, x0, tgt, torch.tensor(T_OF_ROW), OI.schedule_tables(T_ROWS, schedule))
    mo, x_t, x0, tgt = (v.cuda() for v in (mo, x_t, x0, tgt))
    t = torch.tensor(T_OF_ROW).cuda()
    w_simple, w_vlb = 0.75, 0.05
    loss, rows, d_unw, status = _loss_rows(mo, x_t, x0, tgt, t, coef, T_ROWS, w_simple, w_vlb)
    r = rows.cpu().numpy().astype(np.float64)
    assert status == 0
    _assert_rows_close(r[0], S, [0] * B_ROWS, "S")  # (the MSE rows are well conditioned at every t)
    _assert_rows_close(r[1], V, T_OF_ROW, "V")
    # the defining formulas of rows[2], loss[0..2] from rows[0..1], with and without weights
    np.testing.assert_allclose(r[2], w_simple * r[0] + w_vlb * r[1], rtol=1e-6)
    np.testing.assert_allclose(loss.cpu().numpy(), [r[2].mean(), r[0].mean(), r[1].mean()], rtol=1e-6)
    weight = (0.25 + 2.0 * torch.rand(B_ROWS, generator=torch.Generator().manual_seed(5))).cuda()
    loss_w, rows_w, d_w, status = _loss_rows(mo, x_t, x0, tgt, t, coef, T_ROWS, w_simple, w_vlb, weight)
    assert status == 0 and torch.equal(rows_w, rows)
    wn = weight.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(loss_w.cpu().numpy(), [(wn * r[2]).mean(), r[0].mean(), r[1].mean()], rtol=1e-6)
    np.testing.assert_array_max_ulp(d_w.cpu().numpy(), (d_unw * weight.reshape(-1, 1, 1, 1)).cpu().numpy(), maxulp=1)
    # deterministic: a second run gives the same bits
    loss_2, rows_2, d_2, _ = _loss_rows(mo, x_t, x0, tgt, t, coef, T_ROWS, w_simple, w_vlb, weight)
    assert torch.equal(loss_2, loss_w) and torch.equal(rows_2, rows_w) and torch.equal(d_2, d_w)


def test_loss_rows_never_indexes_with_a_timestep_outside_the_table():
    """t = [0, T + 1, 3]: images 0 and 1 become NaN (rows, gradient, the three means), image 2 is untouched by them, status is set"""
    coef = _coef(T_ROWS, "cosine")
    mo, x_t, x0, tgt = (v[:3].contiguous().cuda() for v in _inputs(75))
    good = torch.tensor([3, 3, 3]).cuda()
    _, rows_ok, d_ok, status = _loss_rows(mo, x_t, x0, tgt, good, coef, T_ROWS, 1.0, 0.05)
    assert status == 0
    loss, rows, d_out, status = _loss_rows(mo, x_t, x0, tgt, torch.tensor([0, T_ROWS + 1, 3]).cuda(), coef, T_ROWS, 1.0, 0.05)
    assert status == 1
    assert bool(torch.isnan(rows[:, :2]).all()) and bool(torch.isnan(loss).all()) and bool(torch.isnan(d_out[:2]).all())
    assert torch.equal(rows[:, 2], rows_ok[:, 2]) and torch.equal(d_out[2], d_ok[2])
    loss, rows, d_out, status = _loss_rows(mo, x_t, x0, tgt, torch.tensor([-5, 1 << 40, 3]).cuda(), coef, T_ROWS, 0.0, 1.0, want_grad=False)
    assert status == 1 and bool(torch.isnan(rows[:, :2]).all()) and bool(torch.isfinite(rows[:, 2]).all())


# ------------------------------------------------------------------------------------------ A2: dmme_iddpm_prior_rows
@pytest.mark.parametrize("chw", [75, 3072])
def test_prior_rows_vs_float64(chw):
    from dmme_amd import _lib

    h, w = SHAPES[chw]
    x0 = _pixel_grid(11, (4, 3, h, w))
    x0_dev = x0.cuda()
    for abar_T in (float(np.float32(0.3660)), float(np.float32(4.1e-5)), float(np.float32(1.9e-15))):  # linear T = 100, linear T = 1000, cosine
        prior = torch.empty(4, device="cuda")
        _lib.check(_lib.lib().dmme_iddpm_prior_rows(_lib.ptr(x0_dev), 4, chw, abar_T, _lib.ptr(prior), _lib.stream_ptr()))
        want = R.prior_rows(x0.numpy(), abar_T)
        print(f"prior chw {chw} abar_T {abar_T:.3e}: got {prior.tolist()} want {want.tolist()}")
        np.testing.assert_allclose(prior.cpu().numpy(), want, rtol=1e-5)


# ------------------------------------------------------------------------------------------ A4: dmme_tsampler_update
def _update(hist, count, T, H, t, L):
    from dmme_amd import _lib

    h, c = torch.from_numpy(hist).cuda(), torch.from_numpy(count).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    tt, LL = torch.tensor(t, dtype=torch.int64).cuda(), torch.from_numpy(np.asarray(L, dtype=np.float32)).cuda()
    _lib.check(_lib.lib().dmme_tsampler_update(_lib.ptr(h), _lib.ptr(c), T, H, _lib.ptr(tt), _lib.ptr(LL), len(t), _lib.ptr(status), _lib.stream_ptr()))
    return h.cpu().numpy(), c.cpu().numpy(), int(status.item())


def test_tsampler_update_is_the_push_loop_bit_for_bit():
    """T = 6, H = 10, B = 37: timestep 2 occurs 23 times (wraps the ring twice), 4 starts at count 9, 5 is absent; a NaN loss and a
    t = 0 are skipped and flagged"""
    T, H, B = 6, 10, 37
    rng = np.random.RandomState(7)
    hist = np.exp(rng.standard_normal((T + 1, H))).astype(np.float32)
    count = np.array([0, 3, 2, 10, 9, 6, 0], dtype=np.int32)
    t = [2] * 23 + [4, 4, 4, 1, 1, 3, 3, 6, 6, 6, 1, 3, 0, 6]
    assert len(t) == B and 5 not in t
    t = [t[i] for i in rng.permutation(B)]
    L = np.exp(rng.standard_normal(B)).astype(np.float32)
    L[t.index(6)], L[t.index(1)] = np.nan, np.inf  # (timestep 2 keeps its 23 pushes)
    want_h, want_c = hist.copy(), count.copy()
    assert R.push(want_h, want_c, t, L, T, H) == 1
    got_h, got_c, status = _update(hist, count, T, H, t, L)
    assert status == 1 and np.array_equal(got_c, want_c) and np.array_equal(got_h.view(np.uint32), want_h.view(np.uint32))
    assert want_c[2] == H and np.array_equal(got_h[5], hist[5]) and np.array_equal(got_h[0], hist[0])
    # a clean batch leaves the flag alone; an out-of-range count is clamped, never used as a position
    clean_t, clean_L = [1, 2, 2, 6], [0.5, 0.25, 0.125, 2.0]
    want_h, want_c = hist.copy(), count.copy()
    assert R.push(want_h, want_c, clean_t, clean_L, T, H) == 0
    got_h, got_c, status = _update(hist, count, T, H, clean_t, clean_L)
    assert status == 0 and np.array_equal(got_c, want_c) and np.array_equal(got_h, want_h)
    wild = count.copy()
    wild[1], wild[2] = -7, 1 << 30
    got_h, got_c, status = _update(hist, wild, T, H, clean_t, clean_L)
    assert got_c[1] == 1 and got_h[1, 0] == 0.5 and got_c[2] == H and got_h[2, H - 1] == 0.125 and got_h[2, H - 2] == 0.25


# ------------------------------------------------------------------------------------------ A3: dmme_tsampler_draw
U0 = 0.001


def _draw(hist, count, T, H, B, seed, offset):
    from dmme_amd import _lib

    h, c = torch.from_numpy(hist).cuda(), torch.from_numpy(count).cuda()
    t = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    w = torch.empty(B, device="cuda")
    p = torch.empty(T + 1, device="cuda")
    _lib.check(_lib.lib().dmme_tsampler_draw(_lib.ptr(h), _lib.ptr(c), T, H, U0, seed, offset, B, _lib.ptr(t), _lib.ptr(w), _lib.ptr(p), _lib.stream_ptr()))
    return t.cpu().numpy(), w.cpu().numpy(), p.cpu().numpy()


def _check_draws(t, w, p, T, B, seed, offset):
    assert t.min() >= 1 and t.max() <= T
    u = P.uniforms(seed, offset, B)
    bad = R.bin_violations(p, u, t, T)
    assert bad.size == 0, f"{bad.size} draws outside their bin, e.g. b = {bad[:5]}, t = {t[bad[:5]]}, u = {u[bad[:5]]}"


def _warm_state(T, H, seed):
    rng = np.random.RandomState(seed)
    hist = np.exp(1.5 * rng.standard_normal((T + 1, H))).astype(np.float32)
    return hist, np.full(T + 1, H, dtype=np.int32)


def test_tsampler_draw_is_uniform_with_unit_weights_until_warm():
    T, H, B = 64, 10, 4096
    hist, count = _warm_state(T, H, 1)
    count[17] = H - 1  # one short of warm
    count[0] = 0       # (row 0 is unused: it does not count)
    seed, offset = 2021, 12345
    t, w, p = _draw(hist, count, T, H, B, seed, offset)
    assert np.all(w == np.float32(1.0))
    assert p[0] == 0.0 and np.all(p[1:] == np.float32(1.0) / np.float32(T))
    _check_draws(t, w, p, T, B, seed, offset)
    assert len(np.unique(t)) == T


@pytest.mark.parametrize("seed,offset", [(2021, 0), (0xDEADBEEFCAFE, (1 << 40) + 3)])
def test_tsampler_draw_warm_vs_float64(seed, offset):
    T, H, B = 64, 10, 4096
    hist, count = _warm_state(T, H, 2)
    count[0] = 0
    t, w, p = _draw(hist, count, T, H, B, seed, offset)
    warm, want_p = R.probabilities(hist, count, T, H, U0)
    assert warm and p[0] == 0.0
    print(f"warm T={T}: max rel error of p {np.max(np.abs(p[1:] / want_p[1:] - 1)):.2e}; sum p {p.astype(np.float64).sum():.9f}")
    np.testing.assert_allclose(p[1:], want_p[1:], rtol=1e-5)  # ~80 fp32 roundings of 6e-8: 12 for s_t, 64 for the sum, a few for the mix
    _check_draws(t, w, p, T, B, seed, offset)  # every draw, none excluded
    assert len(np.unique(t)) == T
    np.testing.assert_allclose(w, 1.0 / (T * p.astype(np.float64)[t]), rtol=1e-6)  # two roundings
    assert w.min() < 0.5 and w.max() > 2.0  # (these inputs do spread the weights)
    t2, w2, p2 = _draw(hist, count, T, H, B, seed, offset)
    assert np.array_equal(t, t2) and np.array_equal(w.view(np.uint32), w2.view(np.uint32)) and np.array_equal(p.view(np.uint32), p2.view(np.uint32))


def test_tsampler_draw_scans_more_timesteps_than_one_block_has_threads():
    """T = 4000 (the IDDPM config): indices stay in range and p is right; the bin check is about a bin wide there, which is accepted"""
    T, H, B = 4000, 10, 64
    hist, count = _warm_state(T, H, 3)
    seed, offset = 77, 1 << 33
    t, w, p = _draw(hist, count, T, H, B, seed, offset)
    warm, want_p = R.probabilities(hist, count, T, H, U0)
    assert warm
    print(f"warm T={T}: max rel error of p {np.max(np.abs(p[1:] / want_p[1:] - 1)):.2e}; sum p {p.astype(np.float64).sum():.9f}")
    np.testing.assert_allclose(p[1:], want_p[1:], rtol=1e-5)
    assert abs(p.astype(np.float64).sum() - 1.0) < 1e-5
    _check_draws(t, w, p, T, B, seed, offset)
    np.testing.assert_allclose(w, 1.0 / (T * p.astype(np.float64)[t]), rtol=1e-6)
    t2, w2, p2 = _draw(hist, count, T, H, B, seed, offset)
    assert np.array_equal(t, t2) and np.array_equal(w, w2) and np.array_equal(p, p2)
    # one timestep short of warm at this size too: uniform, unit weights
    count[T] = H - 1
    t, w, p = _draw(hist, count, T, H, B, seed, offset)
    assert np.all(w == np.float32(1.0)) and np.all(p[1:] == np.float32(1.0) / np.float32(T))
    _check_draws(t, w, p, T, B, seed, offset)


# ------------------------------------------------------------------------------------------ through the public interface
def _tiny(seed=31):
    from .test_gpu_iddpm import _build

    return _build(OI.TINY, seed, "fp32")[0]


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_respaced_chain_step_by_step(schedule):
    """T = 100, K = 7: at every step the network is evaluated at s_k (the runner's model_out equals a separate model(x, s_k) call), the
    update is the float64 one on that model_out with the Philox normals of the chain's offsets, the last step adds no noise; the
    replayed graph and the eager launches agree bit for bit"""
    import dmme_amd

    T, K, B = 100, 7, 2
    net = _tiny()
    idd = dmme_amd.IDDPM(net, T, schedule=schedule).cuda()
    steps = R.space_timesteps(T, K)
    rows = R.respaced_rows(idd.alpha_bar.reshape(-1).double().cpu().numpy(), steps)
    shape = (B, 3, 32, 32)
    numel = int(np.prod(shape))
    x0 = synth.normal(5, shape).cuda()
    xe, xg = x0.clone(), x0.clone()
    seed, off0 = 2021, 1000
    eager = idd.respaced_runner(xe, K, use_graph=False)
    assert eager.kind == dmme_amd._lib.CHAIN_IDDPM and eager.n_steps == K and eager.ttab.tolist() == [0] + steps
    eager.set(K, seed, off0)
    with torch.no_grad():
        for j, k in enumerate(range(K, 0, -1)):
            before = xe.clone()
            eager.step()
            out = eager.out.clone()
            assert torch.equal(out, net(before, torch.tensor([steps[k - 1]], device="cuda"))), f"step {k}: the network did not see t = {steps[k - 1]}"
            z = P.normals(seed, off0 + j * (numel // 4), numel).reshape(shape)
            want = R.chain_step(before.cpu().numpy(), out.cpu().numpy(), z, rows[k], add_noise=k != 1)
            np.testing.assert_allclose(xe.cpu().numpy(), want, atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=0, err_msg=f"{schedule} step {k}")
            if k == 1:  # the noise the last step leaves out would have been far outside that tolerance
                noisy = R.chain_step(before.cpu().numpy(), out.cpu().numpy(), z, rows[k], add_noise=True)
                assert float(np.abs(noisy - want).max()) > 1e-3
        graph = idd.respaced_runner(xg, K, use_graph=True)
        graph.set(K, seed, off0)
        for _ in range(K):
            graph.step()
        torch.cuda.synchronize()
    assert graph.graph is not None or getattr(net, "_graph_disabled", False)
    assert torch.equal(xg, xe)


def test_generate_with_sample_steps():
    """the public call: right shape, finite, K network evaluations' worth of Philox draws, equal to the eager loop under the same seed;
    `sample_steps=None` is the full chain as before"""
    import dmme_amd
    from dmme_amd import _lib

    T, K = 100, 7
    net = _tiny()
    idd = dmme_amd.IDDPM(net, T).cuda()
    shape = (2, 3, 32, 32)
    torch.manual_seed(11)
    img = idd.generate(shape, sample_steps=K)
    assert tuple(img.shape) == shape and bool(torch.isfinite(img).all())
    assert getattr(idd, f"_runner_k{K}") is not None and getattr(idd, "_runner", None) is None
    n, rows, ttab = idd._respaced_tables(K)
    torch.manual_seed(11)
    x = dmme_amd.gaussian(shape, device="cuda")
    with torch.no_grad():
        for k in range(K, 0, -1):
            out = net(x, idd.timestep_tensor(ttab[k], x.device))
            z = dmme_amd.gaussian_like(x)
            c = rows[k]
            _lib.check(_lib.lib().dmme_iddpm_step(_lib.ptr(x), _lib.ptr(out), _lib.ptr(z), c[0], c[1], c[2], c[3], int(ttab[k] != 1), 2, 3072, _lib.stream_ptr()))
    assert torch.equal(img, x)
    lit = dmme_amd.LitIDDPM(diffusion_model=idd)
    torch.manual_seed(11)
    assert torch.equal(lit.generate(shape, sample_steps=K), img)
    with pytest.raises(ValueError):
        idd.generate(shape, sample_steps=1)
    short = dmme_amd.IDDPM(net, 12).cuda()
    torch.manual_seed(3)
    a = short.generate(shape)
    torch.manual_seed(3)
    b = short.generate(shape, sample_steps=None)
    assert torch.equal(a, b) and short._runner is not None


def test_weighted_training_step_and_the_resampler_state(tmp_path):
    import dmme_amd
    from dmme_amd.checkpoint import load_checkpoint, save_checkpoint
    from dmme_amd.diffusion_models.iddpm import TS_HISTORY as H

    T, B = 8, 16
    net = _tiny()
    uni = dmme_amd.IDDPM(net, T, loss_type="vlb").cuda()
    lsm = dmme_amd.IDDPM(net, T, loss_type="vlb", t_sampler="loss-second-moment").cuda()
    x0 = _pixel_grid(21, (B, 3, 32, 32)).cuda()
    z = synth.normal(22, (B, 3, 32, 32)).cuda()
    t_inj = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8] * 2).cuda()
    with torch.no_grad():
        want = uni.training_step(x0, t=t_inj, noise=z)
        got = lsm.training_step(x0, t=t_inj, noise=z)  # before warm-up, injected t: every weight is 1
    print(f"cold weighted step {got.item():.9g} vs uniform module {want.item():.9g}")
    np.testing.assert_allclose(got.item(), want.item(), rtol=2e-5)
    assert lsm.last_draw.weight is None and int(lsm._ts_count.sum()) == B
    hist, count = np.zeros((T + 1, H), dtype=np.float32), np.zeros(T + 1, dtype=np.int32)
    assert R.push(hist, count, t_inj.tolist(), lsm.last_draw.rows[2].cpu().numpy(), T, H) == 0
    assert np.array_equal(lsm._ts_hist.cpu().numpy(), hist) and np.array_equal(lsm._ts_count.cpu().numpy(), count)

    torch.manual_seed(4)
    steps = 0
    while not np.all(count[1:] == H):
        assert steps < 200, f"not warm after 200 steps: count = {count.tolist()}"
        with torch.no_grad():
            loss = lsm.training_step(x0)
        draw = lsm.last_draw
        assert bool((draw.weight == 1.0).all()) and int(draw.t.min()) >= 1 and int(draw.t.max()) <= T
        assert R.push(hist, count, draw.t.tolist(), draw.rows[2].cpu().numpy(), T, H) == 0
        assert np.array_equal(lsm._ts_hist.cpu().numpy(), hist) and np.array_equal(lsm._ts_count.cpu().numpy(), count), steps
        steps += 1
    print(f"warm after {steps} steps of {B} draws")

    # warm: a weighted step with its backward
    net.zero_grad(set_to_none=True)
    loss = lsm.training_step(x0)
    loss.backward()
    draw = lsm.last_draw
    p = lsm._ts_p.cpu().numpy().astype(np.float64)
    warm, want_p = R.probabilities(hist, count, T, H, 0.001)
    assert warm and abs(p.sum() - 1.0) < 1e-5 and p[1:].max() > 1.5 * p[1:].min()
    np.testing.assert_allclose(p[1:], want_p[1:], rtol=1e-5)
    w, rows = draw.weight.cpu().numpy().astype(np.float64), draw.rows.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(w, 1.0 / (T * p[draw.t.cpu().numpy()]), rtol=1e-6)
    # fp32 products and a sum over 16 images, at most 32 roundings of 6e-8
    np.testing.assert_allclose(loss.item(), (w * rows[2]).mean(), rtol=2e-6)
    assert math.isfinite(loss.item())
    grads = [q.grad for q in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    assert R.push(hist, count, draw.t.tolist(), draw.rows[2].cpu().numpy(), T, H) == 0
    assert np.array_equal(lsm._ts_hist.cpu().numpy(), hist)
    lsm.check_t_sampler()  # nothing was skipped

    # save -> a fresh module -> the same draw at the same generator state
    path = str(tmp_path / "lsm.ckpt")
    save_checkpoint(path, lsm)
    fresh = dmme_amd.IDDPM(_tiny(seed=32), T, loss_type="vlb", t_sampler="loss-second-moment")
    load_checkpoint(path, fresh)
    fresh.cuda()
    assert torch.equal(fresh._ts_hist, lsm._ts_hist) and torch.equal(fresh._ts_count, lsm._ts_count)
    torch.manual_seed(99)
    t_a, w_a = lsm.draw_timesteps(64)
    torch.manual_seed(99)
    t_b, w_b = fresh.draw_timesteps(64)
    assert torch.equal(t_a, t_b) and torch.equal(w_a, w_b) and not bool((w_a == 1.0).all())


def test_bits_per_dim_vs_oracle():
    """T = 6, B = 3, injected noise, x_0 on the pixel grid.  Reference: per step, oracle.iddpm.loss_vlb image by image on the GPU
    model's own output for that step (x_t from the same dmme_q_sample call), plus the float64 prior, over ln 2"""
    import dmme_amd
    from dmme_amd import _lib

    T, B = 6, 3
    shape = (B, 3, 32, 32)
    net = _tiny()
    x0 = _pixel_grid(41, shape)
    noise = torch.stack([synth.normal(50 + k, shape) for k in range(T)])
    for schedule in ("cosine", "linear"):
        idd = dmme_amd.IDDPM(net, T, schedule=schedule).cuda()
        got = idd.bits_per_dim(x0.cuda(), noise=noise.cuda())
        assert tuple(got.terms.shape) == (B, T) and tuple(got.total.shape) == (B,) and tuple(got.prior.shape) == (B,)
        again = idd.bits_per_dim(x0.cuda(), noise=noise.cuda())
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        tabs = OI.schedule_tables(T, schedule)
        want = np.zeros((B, T))
        x_t, tgt = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
        x0_dev, noise_dev = x0.cuda(), noise.cuda()
        for step in range(T, 0, -1):
            t = torch.full((B,), step, dtype=torch.int64)
            t_dev = t.cuda()
            _lib.check(_lib.lib().dmme_q_sample(_lib.ptr(x0_dev), _lib.ptr(noise_dev[step - 1]), _lib.ptr(idd._sqrt_alpha_bar),
                                                _lib.ptr(idd._sqrt_one_minus_alpha_bar), _lib.ptr(t_dev), B, 3072, _lib.ptr(x_t), _lib.ptr(tgt), _lib.stream_ptr()))
            with torch.no_grad():
                out = net(x_t, t_dev)
            _, V = _oracle_rows(out.cpu(), x_t.cpu(), x0, tgt.cpu(), t, tabs)
            want[:, step - 1] = V / LN2
        terms = got.terms.cpu().numpy().astype(np.float64)
        for step in range(1, T + 1):
            _assert_rows_close(terms[:, step - 1], want[:, step - 1], [step] * B, f"{schedule} L_{step - 1}")
        want_prior = R.prior_rows(x0.numpy(), float(idd.alpha_bar.reshape(-1)[T])) / LN2
        prior = got.prior.cpu().numpy().astype(np.float64)
        print(f"{schedule}: total {got.total.tolist()} want {(want_prior + want.sum(axis=1)).tolist()}; prior {prior.tolist()}")
        np.testing.assert_allclose(prior, want_prior, rtol=1e-5)
        np.testing.assert_allclose(got.total.cpu().numpy(), want_prior + want.sum(axis=1), rtol=5e-4)  # bounded by its worst term
        np.testing.assert_allclose(got.total.cpu().numpy(), prior + terms.sum(axis=1), rtol=1e-6)
