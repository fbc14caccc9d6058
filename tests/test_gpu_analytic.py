"""-m gpu: Analytic-DPM (dmme_amd.AnalyticDPM) on the MI355X - the statistics pass (dmme_analytic_moment) and the rows of the K-step bound
(dmme_analytic_vlb_rows) against the float64 restatement tests/analytic_ref.py under its derived bounds (built from the precision of fp32, the
kernels' order of operations and their summation shape, not measured; tests/test_analytic_host.py holds plain fp32 numpy against the same
bounds on the CPU), the NLL row against dmme_iddpm_loss_rows', and through the public interface on the tiny UNet: `estimate_moments` against
an eager restatement on the same Philox words and the oracle network, `generate` through the captured chain against the eager loop (bit for
bit) and against GeneralizedDDIM's, `bits_per_dim` term by term, the checkpoint, and a bf16 chain.  Every comparison prints its figures."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import analytic_ref as R
from . import philox_ref as P

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 105 values: the element tail and an odd row; two images of 3072: quads, more than one partial workgroup; five images with duplicate timesteps
CASES = [((1, 3, 5, 7), [4]), ((2, 3, 32, 32), [3, 9]), ((5, 3, 32, 32), [3, 7, 3, 1, 7])]
T_MOM = 10
NAN = float("nan")


def _L():
    from dmme_amd import _lib

    return _lib


def _pixel_grid(seed, shape):
    """x_0 on the 8-bit grid k/127.5 - 1, both ends present in every image (the open-ended bins of the discrete NLL)"""
    k = synth.randint(seed, 0, 256, int(np.prod(shape))).reshape(shape).to(torch.float32)
    for b in range(shape[0]):
        k[b].reshape(-1)[0], k[b].reshape(-1)[1] = 255.0, 0.0
    return k / 127.5 - 1.0


def _planes(eps, planes):
    """(B, planes * chw): the eps plane first; a second plane holds NaN (it is never read)"""
    e = eps.reshape(eps.shape[0], -1)
    return e.contiguous() if planes == 1 else torch.cat([e, torch.full_like(e, NAN)], dim=1).contiguous()


# ------------------------------------------------------------------------------------------ 5. dmme_analytic_moment
class _Tables:
    """sum / count of T + 1 entries between two guard values"""

    def __init__(self, T):
        self.T = T
        self.sum_buf = torch.full((T + 3,), 7.0, dtype=torch.float64, device="cuda")
        self.count_buf = torch.full((T + 3,), 7, dtype=torch.int64, device="cuda")
        self.sum, self.count = self.sum_buf[1:T + 2], self.count_buf[1:T + 2]
        self.sum.copy_(0.5 * torch.arange(T + 1, dtype=torch.float64))
        self.count.copy_(torch.arange(T + 1) % 3)
        self.sum0, self.count0 = self.sum.cpu().numpy().copy(), self.count.cpu().numpy().copy()

    def guards_intact(self):
        return (float(self.sum_buf[0]) == 7.0 and float(self.sum_buf[-1]) == 7.0 and int(self.count_buf[0]) == 7 and int(self.count_buf[-1]) == 7
                and float(self.sum[0]) == self.sum0[0] and int(self.count[0]) == self.count0[0])


def _moment(out, stride, t, tabs, chw, rows=True):
    L = _L()
    B = out.shape[0]
    r = torch.full((B,), 7.0, device="cuda") if rows else None
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(32 * B, device="cuda")
    tt = torch.tensor(t, dtype=torch.int64, device="cuda")
    L.check(L.lib().dmme_analytic_moment(L.ptr(out), stride, L.ptr(tt), tabs.T, B, chw, L.ptr(tabs.sum), L.ptr(tabs.count), L.ptr(r), L.ptr(status), L.ptr(scratch),
                                         L.stream_ptr()), "dmme_analytic_moment")
    torch.cuda.synchronize()
    return r, int(status.item())


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("shape,t", CASES)
def test_moment_vs_float64(shape, t, planes):
    """rows, sum and count against float64 inside moment_bound (a timestep that occurs twice: the sum of its images' bounds); a second call
    accumulates; nothing outside entries 1..T is written; two runs give equal bits"""
    B, chw = shape[0], int(np.prod(shape[1:]))
    eps = (0.25 + 0.1 * np.arange(B)).reshape(B, 1, 1, 1).astype(np.float32) * synth.normal(7, shape).numpy()
    e64 = eps.reshape(B, -1).astype(np.float64)
    out = _planes(torch.from_numpy(eps), planes).cuda()
    m, bound = R.moment(e64), R.moment_bound(e64)
    tabs = _Tables(T_MOM)
    want_s, want_c = tabs.sum0.copy(), tabs.count0.copy()
    per_t = np.zeros(T_MOM + 1)
    np.add.at(per_t, t, bound)
    for call in (1, 2):
        rows, status = _moment(out, planes * chw, t, tabs, chw)
        assert status == 0 and R.accumulate(want_s, want_c, t, m, T_MOM) == 0
        err_r = np.abs(rows.cpu().numpy().astype(np.float64) - m)
        err_s = np.abs(tabs.sum.cpu().numpy() - want_s)
        print(f"moment {shape} planes {planes} call {call}: rows {rows.tolist()}; rows err / bound {float((err_r / bound).max()):.3f}, "
              f"largest sum err {float(err_s.max()):.3e} (bound {float((call * per_t).max()):.3e})")
        assert bool(np.all(err_r <= bound)) and bool(np.all(err_s <= call * per_t + 1e-15 * np.abs(want_s)))
        assert np.array_equal(tabs.count.cpu().numpy(), want_c) and tabs.guards_intact()
    again = _Tables(T_MOM)
    for _ in range(2):
        rows2, _ = _moment(out, planes * chw, t, again, chw)
    assert torch.equal(again.sum, tabs.sum) and torch.equal(again.count, tabs.count) and torch.equal(rows2, rows)
    none = _Tables(T_MOM)
    assert _moment(out, planes * chw, t, none, chw, rows=False) == (None, 0)  # rows is optional


def test_moment_never_indexes_with_a_timestep_outside_the_tables():
    """t = [0, T + 1, 3]: images 0 and 1 add nothing and get a NaN row, the status word is set, image 2's row and sum carry the bits of a call
    that holds image 2 alone; the guards stand"""
    shape = (3, 3, 5, 7)
    chw = 105
    out = synth.normal(8, shape).reshape(3, -1).contiguous().cuda()
    alone = _Tables(T_MOM)
    rows_ok, status = _moment(out[2:], chw, [3], alone, chw)
    assert status == 0
    for bad in ([0, T_MOM + 1, 3], [-5, 1 << 40, 3]):
        tabs = _Tables(T_MOM)
        rows, status = _moment(out, chw, bad, tabs, chw)
        assert status == 1 and bool(torch.isnan(rows[:2]).all()) and torch.equal(rows[2:], rows_ok)
        assert torch.equal(tabs.sum, alone.sum) and torch.equal(tabs.count, alone.count) and tabs.guards_intact()


# ------------------------------------------------------------------------------------------ 6. dmme_analytic_vlb_rows
S_ROWS = 5
IDX = {1: [[1], [2]], 2: [[1, 3]], 5: [[3, 5, 3, 1, 5]]}


def _vlb_table(variance="analytic"):
    import dmme_amd

    p = dmme_amd.AnalyticDPM(torch.nn.Identity(), 100, S_ROWS).set_moments(np.linspace(0.95, 0.3, 101))
    return p._vlb_table(variance)


def _vlb_inputs(shape, idx, tab, seed=0):
    """x_0 on the pixel grid, x_t = sa x_0 + s1 z at each image's own index, eps_theta = z + 0.3 noise: what a trained network would see"""
    B = shape[0]
    x0 = _pixel_grid(20 + seed, shape).reshape(B, -1).numpy()
    z = synth.normal(21 + seed, shape).reshape(B, -1).numpy()
    rows = tab[np.clip(idx, 1, tab.shape[0] - 1)]
    x_t = (rows[:, R.SA:R.SA + 1] * x0 + rows[:, R.S1:R.S1 + 1] * z).astype(np.float32)
    e = (z + 0.3 * synth.normal(22 + seed, shape).reshape(B, -1).numpy()).astype(np.float32)
    return e, x_t, x0


def _vlb(out, stride, x_t, x_0, idx, tab):
    L = _L()
    B, chw = x_t.shape[0], x_t.shape[1]
    rows = torch.full((B,), 7.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(32 * B, device="cuda")
    ii = torch.tensor(idx, dtype=torch.int64, device="cuda")
    coef = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.float32)).reshape(-1).cuda()
    L.check(L.lib().dmme_analytic_vlb_rows(L.ptr(out), stride, L.ptr(x_t), L.ptr(x_0), L.ptr(ii), L.ptr(coef), tab.shape[0] - 1, B, chw, L.ptr(rows), L.ptr(status),
                                           L.ptr(scratch), L.stream_ptr()), "dmme_analytic_vlb_rows")
    torch.cuda.synchronize()
    return rows, int(status.item())


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("shape", [c[0] for c in CASES])
def test_vlb_rows_vs_float64(shape, planes):
    """the KL rows and the NLL row against float64 inside kl_bound / nll_bound, at index mixes that hold 1 and indices above it, for the
    analytic and the beta variance; two runs give equal bits"""
    B, chw = shape[0], int(np.prod(shape[1:]))
    for variance in ("analytic", "beta"):
        tab = _vlb_table(variance)
        for idx in IDX[B]:
            e, x_t, x0 = _vlb_inputs(shape, idx, tab)
            want, bound, status = R.vlb_rows(e, x_t, x0, idx, tab)
            assert status == 0 and bool(np.all(np.isfinite(bound))) and bool(np.all(bound <= 1e-3 * np.abs(want) + 1e-6))  # the bound says something
            args = (_planes(torch.from_numpy(e), planes).cuda(), planes * chw, torch.from_numpy(x_t).cuda(), torch.from_numpy(x0).cuda(), idx, tab)
            rows, status = _vlb(*args)
            err = np.abs(rows.cpu().numpy().astype(np.float64) - want)
            print(f"vlb rows {shape} planes {planes} {variance} idx {idx}: {rows.tolist()}; float64 {want.tolist()}; err / bound {(err / bound).tolist()}")
            assert status == 0 and bool(np.all(err <= bound))
            rows2, _ = _vlb(*args)
            assert torch.equal(rows, rows2)


def test_vlb_rows_never_index_outside_the_table():
    """idx = [0, S + 1, 3] (and far outside): NaN rows and the status word for the first two, image 2 carries the bits of a clean call"""
    shape = (3, 3, 5, 7)
    tab = _vlb_table()
    e, x_t, x0 = _vlb_inputs(shape, [3, 3, 3], tab)
    dev = [torch.from_numpy(v).cuda() for v in (e, x_t, x0)]
    good, status = _vlb(dev[0], 105, dev[1], dev[2], [3, 3, 3], tab)
    assert status == 0 and bool(torch.isfinite(good).all())
    for bad in ([0, S_ROWS + 1, 3], [-7, 1 << 40, 3]):
        rows, status = _vlb(dev[0], 105, dev[1], dev[2], bad, tab)
        assert status == 1 and bool(torch.isnan(rows[:2]).all()) and torch.equal(rows[2:], good[2:])


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 32, 32)])
def test_nll_row_against_iddpm_loss_rows(shape):
    """index 1 against dmme_iddpm_loss_rows at t == 1 on a two-plane buffer whose v = 1 gives the same log-variance.  From the mean on the
    two kernels evaluate the same expressions; the means differ in form (here (k0 x_t) + (k1 eps), there c0 (x_t - c1 eps)), so the rows are
    not bit-equal: both lie inside their own derived bound of one float64 value (c0 = 1.25, c1 = 0.5 make k1 = -c0 c1 exact)"""
    L = _L()
    B, chw = shape[0], int(np.prod(shape[1:]))
    c0, c1 = 1.25, 0.5
    lv = np.float32(math.log(0.01))
    x0 = _pixel_grid(30, shape).reshape(B, -1).numpy()
    e = (0.2 * synth.normal(31, shape).reshape(B, -1).numpy()).astype(np.float32)
    x_t = ((x0 + 0.1 * synth.normal(32, shape).reshape(B, -1).numpy()) / c0 + c1 * e).astype(np.float32)  # the mean lands 0.1 z from x0, sd = 0.1
    tab = np.zeros((2, 8), dtype=np.float32)
    tab[1] = (c0, -c0 * c1, lv, lv, 0.5, 0.5, 0, 0)
    out = torch.cat([torch.from_numpy(e), torch.ones(B, chw)], dim=1).contiguous().cuda()
    x_t_d, x0_d = torch.from_numpy(x_t).cuda(), torch.from_numpy(x0).cuda()
    mine, status = _vlb(out, 2 * chw, x_t_d, x0_d, [1] * B, tab)
    assert status == 0
    coef = torch.tensor([[0.0] * 8, [c0, c1, float(lv), float(lv) - 1.0, 0, 0, 0, 0]], dtype=torch.float32).reshape(-1).cuda()
    loss, rows = torch.empty(3, device="cuda"), torch.empty((3, B), device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = torch.ones(B, dtype=torch.int64, device="cuda")
    L.check(L.lib().dmme_iddpm_loss_rows(L.ptr(out), L.ptr(x_t_d), L.ptr(x0_d), L.ptr(x_t_d), L.ptr(t), L.ptr(coef), 1, None, B, chw, 0.0, 1.0, L.ptr(loss), L.ptr(rows),
                                         None, 1.0, L.ptr(st), L.ptr(torch.empty(64 * B, device="cuda")), L.stream_ptr()), "dmme_iddpm_loss_rows")
    torch.cuda.synchronize()
    theirs = rows[1]
    e64, xt64 = e.astype(np.float64), x_t.astype(np.float64)
    mean = c0 * (xt64 - c1 * e64)
    want = R.nll_row(e, x_t, x0, tab[1])
    b_mine = R.nll_bound_analytic(e, x_t, x0, tab[1])
    # there: c1 eps, the difference and the product with c0 round once each; its partial sums are added in fp32 (up to 32 of them) and scaled
    d_theirs = abs(c0) * R.U * (np.abs(c1 * e64) + np.abs(xt64 - c1 * e64)) + R.U * np.abs(mean)
    b_theirs = R.nll_bound(mean, d_theirs, x0, float(lv)) + 36 * R.U * np.abs(want)
    dist = np.abs(mine.cpu().numpy().astype(np.float64) - theirs.cpu().numpy().astype(np.float64))
    print(f"NLL row {shape}: here {mine.tolist()}, dmme_iddpm_loss_rows {theirs.tolist()}, float64 {want.tolist()}; distance / bound {(dist / (b_mine + b_theirs)).tolist()}")
    assert int(st.item()) == 0 and bool(np.all(np.abs(mine.cpu().numpy() - want) <= b_mine)) and bool(np.all(dist <= b_mine + b_theirs))


# ------------------------------------------------------------------------------------------ 7. on the tiny UNet
T, K, SHAPE = 100, 5, (2, 3, 32, 32)
UNET_TOL = 1e-5  # the tiny UNet's fp32 parity with the oracle


def _tiny(seed=11, precision="fp32"):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision=precision)
    net.load_state_dict(O.make_state_dict(cfg, seed), strict=True)
    return net.cuda().eval()


def _oracle(seed=11):
    cfg = O.TINY
    sd = {k: v.double() if v.is_floating_point() else v for k, v in O.make_state_dict(cfg, seed).items()}
    return lambda x, t: O.unet_forward(sd, cfg, x, t)


def _images(n=8):
    return (0.5 * synth.normal(42, (n, 3, 32, 32))).clamp(-1.0, 1.0)


@pytest.fixture(scope="module")
def estimated():
    """the process with its moments estimated once: 8 images, one per timestep, passes of 8 (the last of 4), seed 5"""
    import dmme_amd

    proc = dmme_amd.AnalyticDPM(_tiny(), T, K).cuda()
    G = proc.estimate_moments(_images().cuda(), images_per_timestep=1, batch_size=8, seed=5)
    return proc, G


def test_estimate_moments_vs_eager_restatement(estimated):
    """the sums against a restatement on the CPU: the same images and timesteps (tests/test_analytic_host.py: the schedule), the normals of
    the run's Philox spans (seed 5, pass k at the quads the passes before it took), x_t in fp32 as dmme_q_sample forms it, the oracle network
    in float64.  Bound per timestep: moment_bound plus the UNet's parity tolerance through d(eps^2) = 2 |eps| d(eps)"""
    import dmme_amd

    proc, G = estimated
    imgs = _images()
    model = _oracle()
    sa, s1 = proc._sqrt_alpha_bar.cpu().numpy(), proc._sqrt_one_minus_alpha_bar.cpu().numpy()
    want_s, want_c = np.zeros(T + 1), np.zeros(T + 1, dtype=np.int64)
    bound = np.zeros(T + 1)
    off = 0
    passes = dmme_amd.moment_schedule(T, 8, 1)
    assert len(passes) == 13 and len(passes[-1]) == 4
    for k, t in enumerate(passes):
        B = len(t)
        x = imgs[(np.arange(B) + 8 * k) % 8].numpy()
        z = P.normals(5, off, B * 3072).astype(np.float32).reshape(x.shape)
        off += B * 3072 // 4
        f = lambda v: v[t].reshape(B, 1, 1, 1)
        x_t = f(sa) * x + f(s1) * z  # fp32: the product, the product, the sum
        with torch.no_grad():
            e = model(torch.from_numpy(x_t).double(), torch.from_numpy(t)).numpy().reshape(B, -1)
        assert R.accumulate(want_s, want_c, t, R.moment(e), T) == 0
        np.add.at(bound, t, R.moment_bound(e) + (2.0 * np.abs(e) * UNET_TOL + UNET_TOL ** 2).mean(axis=1))
    got_s, got_c = proc._g_sum.cpu().numpy(), proc._g_count.cpu().numpy()
    err = np.abs(got_s - want_s)
    print(f"estimate_moments: G between {np.nanmin(G):.4f} and {np.nanmax(G):.4f}; largest |sum - restatement| {err.max():.3e}, largest err / bound {(err[1:] / bound[1:]).max():.3f}")
    assert np.array_equal(got_c, want_c) and bool(np.all(got_c[1:] == 1)) and got_c[0] == 0
    assert bool(np.all(err[1:] <= bound[1:])) and got_s[0] == 0.0
    np.testing.assert_array_equal(G[1:], np.clip(got_s[1:], 0.0, 1.0))


def test_generate_captured_equals_eager_and_differs_from_generalized_ddim(estimated):
    """`generate` (the captured GDDIM chain step, replayed K times) equals the eager `sampling_step` loop bit for bit under one seed; with
    G = 1 it is GeneralizedDDIM(eta = 1)'s output bit for bit, with the estimated moments it is not; new moments replace the runner"""
    import dmme_amd

    proc, G = estimated
    net = proc.model
    torch.manual_seed(77)
    got = proc.generate(SHAPE).clone()
    runner = proc._runner
    assert runner is not None and runner.kind == dmme_amd._lib.CHAIN_GDDIM and (runner.graph is not None or getattr(net, "_graph_disabled", False))
    torch.manual_seed(77)
    x = dmme_amd.gaussian(SHAPE, device="cuda")
    with torch.no_grad():
        for i in range(K, 0, -1):
            x = proc.sampling_step(x, torch.tensor([i], device="cuda"))
    assert torch.equal(got, x) and bool(torch.isfinite(got).all())
    hand = dmme_amd.GeneralizedDDIM(net, T, K, "linear", eta=1.0).cuda()
    torch.manual_seed(77)
    want_hand = hand.generate(SHAPE).clone()
    assert not torch.equal(got, want_hand)
    ones = dmme_amd.AnalyticDPM(net, T, K).cuda().set_moments(np.ones(T + 1))
    torch.manual_seed(77)
    assert torch.equal(ones.generate(SHAPE), want_hand)
    old = ones._runner
    ones.set_moments(G_filled(G))
    torch.manual_seed(77)
    assert torch.equal(ones.generate(SHAPE), got) and ones._runner is not old
    print(f"generate: max |analytic - hand-set| {float((got - want_hand).abs().max()):.3e}; k2 analytic {[r[2] for r in proc.sampling_rows()]}, hand-set {[r[2] for r in hand._rev_rows]}")


def G_filled(G):
    g = np.array(G, dtype=np.float64)
    g[0] = 0.0
    return g


@pytest.mark.parametrize("variance", ["analytic", "beta", "beta-tilde"])
def test_bits_per_dim_vs_float64(estimated, variance):
    """term by term against the float64 restatement fed the device's own x_t (the same dmme_q_sample call on the injected noise) and network
    outputs, inside kl_bound / nll_bound over ln 2 plus the roundings of the division; the prior as tests/test_gpu_iddpm_paper.py holds it
    (rtol 1e-5); the total is the fp32 sum of its parts.  "beta-tilde": the decoder term sits on the floored variance 1e-12
    (sd = 1e-6), where every element's NLL is 0 or log 1e12 but for those on a bin's edge: the row must lie inside the interval that
    counting the decided elements gives (analytic_ref.nll_saturated_interval)"""
    L = _L()
    proc, _ = estimated
    B = SHAPE[0]
    x0 = _pixel_grid(41, SHAPE)
    noise = torch.stack([synth.normal(50 + k, SHAPE) for k in range(K)])
    got = proc.bits_per_dim(x0.cuda(), variance=variance, noise=noise.cuda())
    again = proc.bits_per_dim(x0.cuda(), variance=variance, noise=noise.cuda())
    assert tuple(got.terms.shape) == (B, K) and tuple(got.total.shape) == (B,) and all(torch.equal(a, b) for a, b in zip(got, again))
    tab = proc._vlb_table(variance)
    tau = proc._tau_host
    x0_d, noise_d = x0.cuda(), noise.cuda()
    x_t = torch.empty(SHAPE, device="cuda")
    terms = got.terms.cpu().numpy().astype(np.float64)
    want = np.zeros((B, K))
    for i in range(K, 0, -1):
        t = torch.full((B,), tau[i], dtype=torch.int64, device="cuda")
        L.check(L.lib().dmme_q_sample(L.ptr(x0_d), L.ptr(noise_d[i - 1]), L.ptr(proc._sqrt_alpha_bar), L.ptr(proc._sqrt_one_minus_alpha_bar), L.ptr(t), B, 3072,
                                      L.ptr(x_t), None, L.stream_ptr()), "dmme_q_sample")
        with torch.no_grad():
            out = proc.model(x_t, t)
        args = (out.cpu().numpy().reshape(B, -1), x_t.cpu().numpy().reshape(B, -1), x0.numpy().reshape(B, -1), [i] * B, tab)
        if i == 1 and variance == "beta-tilde":
            lo, hi, n_out, n_und = R.nll_saturated_interval(*args[:3], tab[1])
            nats = terms[:, 0] * LN2
            print(f"bits/dim beta-tilde term 1: {nats.tolist()} nats inside [{lo.tolist()}, {hi.tolist()}]; of 3072 elements {n_out.tolist()} lie outside their bin, "
                  f"{n_und.tolist()} are undecided")
            assert bool(np.all(lo * (1 - 4 * R.U) <= nats)) and bool(np.all(nats <= hi * (1 + 4 * R.U)))
            assert bool(np.all(n_und <= 0.01 * 3072))  # the interval says something: at most one element in a hundred sits on a bin's edge
            continue
        rows, bound, status = R.vlb_rows(*args)
        want[:, i - 1] = rows / LN2
        err = np.abs(terms[:, i - 1] - want[:, i - 1])
        lim = bound / LN2 + 2 * R.U * np.abs(want[:, i - 1])
        print(f"bits/dim {variance} term {i} (t = {tau[i]}): {terms[:, i - 1].tolist()}, float64 {want[:, i - 1].tolist()}, err {err.tolist()}, bound {lim.tolist()}")
        assert status == 0 and bool(np.all(err <= lim))
    want_prior = R.prior_rows(x0.numpy(), float(proc.alpha_bar.reshape(-1)[tau[K]])) / LN2
    prior = got.prior.cpu().numpy().astype(np.float64)
    print(f"bits/dim {variance}: total {got.total.tolist()}, prior {prior.tolist()}, KL sum {terms[:, 1:].sum(axis=1).tolist()}, decoder {terms[:, 0].tolist()}")
    np.testing.assert_allclose(prior, want_prior, rtol=1e-5)
    np.testing.assert_allclose(got.total.cpu().numpy(), prior + terms.sum(axis=1), rtol=1e-6)
    assert bool(torch.isfinite(got.total).all())


def test_checkpoint_carries_the_moments(estimated, tmp_path):
    import dmme_amd
    from dmme_amd.checkpoint import load_checkpoint, save_checkpoint

    proc, _ = estimated
    path = str(tmp_path / "analytic.ckpt")
    save_checkpoint(path, dmme_amd.LitDDIM(diffusion_model=proc))
    fresh = dmme_amd.AnalyticDPM(_tiny(seed=12), T, K)
    load_checkpoint(path, dmme_amd.LitDDIM(diffusion_model=fresh))
    fresh.cuda()
    assert torch.equal(fresh._g_sum, proc._g_sum) and torch.equal(fresh._g_count, proc._g_count) and fresh.sampling_rows() == proc.sampling_rows()
    torch.manual_seed(3)
    a = proc.generate(SHAPE)
    torch.manual_seed(3)
    assert torch.equal(fresh.generate(SHAPE), a)


# ------------------------------------------------------------------------------------------ 8. bf16
def test_bf16_chain_is_finite():
    """the chain of section 7 (T = 100, K = 5, eta = 1) on the default UNet in bf16, its moments estimated in bf16 too (one image per timestep):
    finite; the distance from the fp32 plan under the same moments and seed is printed, not asserted"""
    import dmme_amd

    sd = O.make_state_dict(O.UNetConfig(), 5)
    nets = {}
    for precision in ("bf16", "fp32"):
        nets[precision] = dmme_amd.UNet(precision=precision)
        nets[precision].load_state_dict(sd)
        nets[precision].cuda().eval()
    p16 = dmme_amd.AnalyticDPM(nets["bf16"], T, K).cuda()
    G = p16.estimate_moments(_images().cuda(), images_per_timestep=1, batch_size=25, seed=5)
    assert bool(np.all(np.isfinite(G[1:]))) and bool(np.all(p16._g_count.cpu().numpy()[1:] == 1))
    p32 = dmme_amd.AnalyticDPM(nets["fp32"], T, K).cuda().set_moments(G_filled(G))
    torch.manual_seed(9)
    a = p16.generate(SHAPE)
    torch.manual_seed(9)
    b = p32.generate(SHAPE)
    print(f"bf16 chain: max |bf16 - fp32| {float((a - b).abs().max()):.3e} on |x| <= {float(b.abs().max()):.3f}; G between {np.nanmin(G):.4f} and {np.nanmax(G):.4f}")
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    bpd = p16.bits_per_dim(_pixel_grid(41, SHAPE).cuda())
    assert bool(torch.isfinite(bpd.total).all())


# ------------------------------------------------------------------------------------------ 9. the trainer's commands
def test_trainer_sample_then_evaluate(tmp_path):
    """`sample --sampler analytic --data config` estimates the moments (one image per timestep) on the YAML's data module, samples and writes
    them into a checkpoint; they are the moments of the network that samples: a module built the same way under the same seed, put in eval
    mode, gives the same sums bit for bit through `estimate_moments` (a network left in train mode would have drawn dropout masks).
    `evaluate --sampler analytic` on that checkpoint finds the moments there and prints bits/dim with its three parts"""
    import dmme_amd
    from dmme_amd import trainer

    ckpt, image = str(tmp_path / "analytic.ckpt"), str(tmp_path / "x.npy")
    config = os.path.join(ROOT, "configs", "ddpm", "cifar10.yaml")
    np.save(image, _pixel_grid(41, SHAPE).numpy())
    base = ["timeout", "-k", "10", "300", sys.executable, "-m", "dmme_amd.trainer"]
    tail = ["--config", config, "--sampler", "analytic", "--sample-steps", "5", "--num-images", "2", "--batch-size", "125"]
    runs = {"sample": ["sample", "--data", "config", "--moment-images", "1", "--save-checkpoint", ckpt],
            "evaluate": ["evaluate", "--ckpt-path", ckpt, "--image", image, "--variance", "beta"]}
    rec = {}
    for name, extra in runs.items():
        res = subprocess.run(base + extra + tail, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=330)
        assert res.returncode == 0, (name, res.returncode, res.stdout[-1000:], res.stderr[-2000:])
        rec[name] = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    print(rec)
    assert rec["sample"]["images"] == [2, 3, 32, 32] and rec["sample"]["finite"] is True
    assert rec["sample"]["analytic"] == {"sample_steps": 5, "eta": 1.0, "tau_schedule": "linear", "moments": "estimated on the data module"}
    ev = rec["evaluate"]
    assert ev["moments"] == "checkpoint" and ev["variance"] == "beta" and ev["sample_steps"] == 5 and len(ev["per_image"]) == 2
    assert all(math.isfinite(ev[k]) for k in ("bits_per_dim", "prior", "kl_sum", "decoder"))
    assert abs(ev["bits_per_dim"] - (ev["prior"] + ev["kl_sum"] + ev["decoder"])) <= 1e-4 * abs(ev["bits_per_dim"])
    # the same estimation by hand on the eval network: the trainer's seed, its module, its loader, then estimate_moments
    state = torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"]
    conf = trainer.parse_config(config)
    conf["precision"] = conf["sample_precision"]
    torch.manual_seed(conf["seed"] if isinstance(conf["seed"], int) and not isinstance(conf["seed"], bool) else 1337)
    module = trainer.build_module(conf).cuda()
    assert module.training and module.diffusion_model.model.training  # (what `sample` starts from)
    module.eval()
    proc = dmme_amd.AnalyticDPM(module.diffusion_model.model, module.diffusion_model.timesteps, 5).cuda()
    proc.estimate_moments(trainer._data_loader(conf, 125), images_per_timestep=1, batch_size=125, seed=None)
    got_s, got_c = state["diffusion_model._g_sum"], state["diffusion_model._g_count"]
    diff = float((got_s - proc._g_sum.cpu()).abs().max())
    print(f"trainer path against estimate_moments on the eval network: largest |difference of the sums| {diff:.3e}")
    assert torch.equal(got_c, proc._g_count.cpu()) and bool((got_c[1:] == 1).all()) and torch.equal(got_s, proc._g_sum.cpu())


def test_moments_and_bound_refuse_a_network_in_train_mode():
    import dmme_amd

    proc = dmme_amd.AnalyticDPM(_tiny().train(), T, K).cuda()
    for call in (lambda: proc.estimate_moments(_images().cuda(), 1, 8), lambda: proc.set_moments(np.full(T + 1, 0.5)).bits_per_dim(_pixel_grid(41, SHAPE).cuda())):
        with pytest.raises(RuntimeError, match="train mode"):
            call()
    assert int(proc._g_count.sum()) == T  # (only what set_moments installed: nothing was launched)
