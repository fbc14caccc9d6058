"""-m gpu: the kernels that turn gradients into weights - dmme_grad_norm, dmme_adam_step, dmme_adam_step_amp, dmme_amp_scale, the bf16
exchange kernels - through the C ABI against the float64 restatement of tests/optim_ref.py (pinned against torch on the CPU by
tests/test_optim_host.py), and FusedAdam on the device: grad_norm() and the build-on-CPU / load / .cuda() order.

BOUNDS (derived, not fitted; u = 2^-24, gamma_k = k u / (1 - k u)).

dmme_grad_norm.  The launch is 1024 blocks x 256 threads x float4, so one sweep of the grid covers 2^20 elements and a buffer of n
elements takes s = ceil(n / 2^20) sweeps.  All summands are squares, so the relative error of the sum is at most gamma_L, L the longest
chain of roundings one summand goes through:
    1           its own square
    4 s         per thread and sweep three additions inside the float4 (or the scalar tail) and one into the accumulator
    6 + 4       the block sum: six butterfly steps inside a 64-lane wave, then the four wave totals one after another
    4           the final kernel: each of 256 threads adds four of the 1024 partials
    6 + 4       its block sum
L = 25 + 4 s.  The square root halves the relative error and adds its own rounding (allowed one ulp = 2 u):  |norm - ref| <= (gamma_L / 2
+ 2 u) ref.  For n <= 2^20 that is 16.5 u = 9.8e-7.

dmme_adam_step / dmme_adam_step_amp, ONE step from identical float32 inputs: tests/optim_ref.py, above `adam_step_bounds` - the operation
count of the update (21 u relative at a large step count) plus the conditioning of the two bias corrections, 2 u (cond - 1) each (sqrt
halves the second), cond = 1 / (1 - b^t): 6.2e-5 at t = 1, 7.3e-6 at t = 10, 1.3e-6 from t = 1000 on; m carries an ABSOLUTE bound (its two
terms may cancel), which the update inherits; p adds one ulp of p unless it starts at 0.  (A bound relative to |dp| ALONE does not exist:
where b1 m and (1 - b1) g cancel, dp is as small as one likes while m's rounding error is not.  The moments here carry signs of their
own, so such elements are in every case; the inherited term is 9 u of the update's size WITHOUT the cancellation, under half the
relative part.)  The scalars reach the kernel as float32, so the restatement rounds them first (`round_scalars=True`).

Two hundred steps: kernel and torch.optim.Adam in float32 are two float32 evaluations of one recurrence that differ in the order of
their operations; each is held against the float64 evaluation of the recurrence IT was given (the kernel: float32 scalars; torch: Python
doubles), and the kernel's error may be at most twice torch's plus one ulp of the value.  Measured on an MI355X, kernel / torch: p 1.07 (max)
and 1.00 (rms), EMA 0.74 and 0.70.  (Both EMA copies drift by about 1.5e-6, a hundred ulps: at d = 0.9999 the product d x ema rounds
the same way step after step.  That is float32 EMA as the reference runs it, not this kernel.)

The exchange kernels and dmme_amp_scale are exact: bit for bit (NaN compared as NaN)."""

import copy
import math

import pytest
import torch

from oracle import unet as O

from . import optim_ref as R
from .test_optim_host import B1, B2, DECAY, EPS, LR, small_gradient_case

pytestmark = pytest.mark.gpu

SWEEP = 1 << 20  # elements one sweep of either grid covers: 1024 x 256 x 4 (norm), 4096 x 256 (Adam, exchange)
U = R.U32


def _L():
    from dmme_amd import _lib

    return _lib, _lib.lib()


def _dev(x):
    return None if x is None else x.detach().float().cuda().contiguous()


# ---------------------------------------------------------------- dmme_grad_norm
NORM_SIZES = [1, 2, 3, 4, 5, 7, 1023, SWEEP - 1, SWEEP + 5, 3 * SWEEP + 2]


def norm_rel_bound(n):
    sweeps = -(-n // SWEEP)
    return R.gamma(25 + 4 * sweeps) / 2 + 2 * U


def _norm(g):
    _lib, lib = _L()
    out, scratch = torch.full((1,), -1.0, device="cuda"), torch.empty(1024, device="cuda")
    _lib.check(lib.dmme_grad_norm(_lib.ptr(g), g.numel(), _lib.ptr(out), _lib.ptr(scratch), _lib.stream_ptr()), "dmme_grad_norm")
    return float(out.item())


@pytest.mark.parametrize("n", NORM_SIZES)
def test_grad_norm_against_float64(n):
    gen = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=gen)
    worst = 0.0
    for mag in (1e-4, 1.0, 65536.0):
        g = (base * mag).cuda()
        want = R.grad_norm(g)
        got = _norm(g)
        worst = max(worst, abs(got - want) / want / norm_rel_bound(n))
        assert abs(got - want) <= norm_rel_bound(n) * want, (n, mag, got, want)
    # no element dropped or counted twice: a single 3 at either end
    for where in (0, n - 1):
        g = torch.zeros(n, device="cuda")
        g[where] = 3.0
        assert abs(_norm(g) - 3.0) <= norm_rel_bound(n) * 3.0, (n, where)
    print(f"n = {n}: worst error {worst:.2f} of the bound {norm_rel_bound(n):.2e}")


@pytest.mark.parametrize("n", NORM_SIZES)
def test_grad_norm_is_not_finite_when_any_element_is_not(n):
    """the norm is the fused pass's inf / NaN detector: index 0, the last element (the scalar tail when n % 4 != 0), the last whole float4"""
    places = {0, n - 1}
    if n >= 4:
        places |= {(n // 4) * 4 - 1, (n // 4) * 4 - 4}
    base = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
    for where in sorted(places):
        for bad in (math.inf, -math.inf, math.nan):
            g = base.clone()
            g[where] = bad
            assert not math.isfinite(_norm(g)), (n, where, bad)


# ---------------------------------------------------------------- dmme_adam_step
def _case(n, seed, g_norm, p_zero=False):
    """gradient of L2 norm `g_norm`, moments of the gradient's size with signs of their own (m's two terms cancel in half the elements)"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(n, generator=gen)
    g = (g.double() * (g_norm / max(float(g.double().norm()), 1e-30))).float()
    s = g_norm / math.sqrt(n)
    m = torch.randn(n, generator=gen) * s
    v = (torch.randn(n, generator=gen) * s) ** 2 + 1e-30
    p = torch.zeros(n) if p_zero else torch.randn(n, generator=gen) * 0.05
    ema = p + torch.randn(n, generator=gen) * 1e-3
    return p, g, m, v, ema


def _run_adam(p, g, m, v, ema, t, norm, max_norm, decay, gs, lr=LR, eps=EPS):
    _lib, lib = _L()
    P, G, M, V, E = (_dev(x) for x in (p, g, m, v, ema))
    N = None if norm is None else torch.tensor([norm], dtype=torch.float32, device="cuda")
    _lib.check(lib.dmme_adam_step(_lib.ptr(P), _lib.ptr(G), _lib.ptr(M), _lib.ptr(V), _lib.ptr(E), P.numel(), lr, B1, B2, eps, t, _lib.ptr(N), max_norm, decay, gs,
                                  _lib.stream_ptr()), "dmme_adam_step")
    torch.cuda.synchronize()
    assert torch.equal(G.cpu(), g)  # the gradient buffer is read only
    return {"p": P.cpu(), "m": M.cpu(), "v": V.cpu(), "ema": None if E is None else E.cpu()}


def _check_step(got, args, what=""):
    """every element of m, v, p, ema within the derived bound of the restatement; -> the worst error in units of the bound"""
    want = dict(zip(("p", "m", "v", "ema"), R.adam_step(*args, round_scalars=True)))
    bound = R.adam_step_bounds(*args)
    worst = {}
    for k in ("m", "v", "p", "ema"):
        if want[k] is None:
            assert got[k] is None
            continue
        err = (got[k].double() - want[k]).abs()
        ratio = torch.where(err > 0, err / bound[k], torch.zeros_like(err))
        worst[k] = float(ratio.max())
        assert bool((err <= bound[k]).all()), f"{what}: {k} off by {worst[k]:.3g} bounds at element {int(ratio.argmax())} of {err.numel()}"
    return worst


ADAM_SIZES = [1, 5, 255, 257, SWEEP + 3, 2 * SWEEP + 5]  # the last two take a second and a third sweep of the 4096 x 256 grid
# regime -> (norm of the mean gradient, max_norm, norm pointer given, EMA given, grad_scale)
REGIMES = {
    "clipped": (3.0, 1.0, True, True, 1.0),
    "not_clipped": (0.3, 1.0, True, True, 1.0),
    "max_norm_0": (3.0, 0.0, True, True, 1.0),
    "norm_null": (3.0, 1.0, False, True, 1.0),
    "ema_null": (3.0, 1.0, True, False, 1.0),
    "grad_scale_eighth_clipped": (3.0, 1.0, True, True, 0.125),
    "grad_scale_eighth_not_clipped": (0.3, 1.0, True, True, 0.125),
}


@pytest.mark.parametrize("n", ADAM_SIZES)
@pytest.mark.parametrize("regime", list(REGIMES))
def test_adam_step_regimes(regime, n):
    mean_norm, max_norm, with_norm, with_ema, gs = REGIMES[regime]
    p, g, m, v, ema = _case(n, 100 + n % 97, mean_norm / gs)  # the buffer holds sums: 1 / grad_scale times the mean gradient
    m, v = m * gs, v * gs * gs  # (the moments are of the MEAN gradient's size)
    norm = R.f32(R.grad_norm(g)) if with_norm else None
    t = 10
    args = (p, g, m, v, ema if with_ema else None, LR, B1, B2, EPS, t, norm, max_norm, DECAY, gs)
    got = _run_adam(p, g, m, v, ema if with_ema else None, t, norm, max_norm, DECAY, gs)
    worst = _check_step(got, args, f"{regime}, n = {n}")
    # the regime is the one its name says: clipping changes the update, and only where it should
    unclipped = R.adam_step(p, g, m, v, None, LR, B1, B2, EPS, t, None, 0.0, DECAY, gs, round_scalars=True)[1]
    same = bool(((got["m"].double() - unclipped).abs() <= R.adam_step_bounds(*args)["m"]).all())
    assert same == (regime not in ("clipped", "ema_null", "grad_scale_eighth_clipped")), regime
    print(f"{regime}, n = {n}: worst error in units of the bound {worst}")


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 200_000])
@pytest.mark.parametrize("clipped", [True, False])
def test_adam_step_precision_from_p_zero_at_many_step_counts(t, clipped):
    """p = 0, so p_new IS the update and no ulp of p hides its error: the relative bound (6.2e-5 at t = 1 ... 1.3e-6 from t = 1000 on)
    plus what m's own rounding carries into it"""
    n = SWEEP + 3
    p, g, m, v, ema = _case(n, 7 + t % 13, 3.0 if clipped else 0.3, p_zero=True)
    norm = R.f32(R.grad_norm(g))
    args = (p, g, m, v, ema, LR, B1, B2, EPS, t, norm, 1.0, DECAY, 1.0)
    worst = _check_step(_run_adam(p, g, m, v, ema, t, norm, 1.0, DECAY, 1.0), args, f"t = {t}")
    print(f"t = {t}, clipped = {clipped}: relative bound {R.update_rel_bound(B1, B2, t):.2e}; worst error in units of the bound {worst}")


@pytest.mark.parametrize("t", [1, 2, 3])
def test_adam_step_places_eps_where_adam_does(t):
    """|g| log-uniform in [1e-10, 1e-6] against eps = 1e-8: the kernel meets the bound, and on the same data a restatement with eps
    under the square root, or added before the bias correction, misses it (tests/test_optim_host.py: by at least ten bounds)"""
    p, g, m, v = small_gradient_case(t)
    args = (p, g, m, v, None, LR, B1, B2, EPS, t, None, 0.0, 0.0, 1.0)
    got = _run_adam(p, g, m, v, None, t, None, 0.0, 0.0, 1.0)
    worst = _check_step(got, args, f"small gradients, t = {t}")
    bound = R.adam_step_bounds(*args)["p"]
    for mutant in (R.adam_step_eps_inside_sqrt, R.adam_step_eps_before_bias_correction):
        off = (got["p"].double() - mutant(*args, round_scalars=True)[0]).abs() / bound
        print(f"t = {t}: the kernel sits {float(off.median()):.3g} bounds (median) from {mutant.__name__}")
        assert bool((off > 1.0).all())  # every element misses
    print(f"t = {t}: worst error in units of the bound {worst}")


def test_two_hundred_steps_drift_no_worse_than_torch_fp32():
    """the shipped scalars (configs/ddpm/cifar10.yaml: lr 2e-4, betas 0.9 / 0.999, eps 1e-8, clip 1.0, EMA 0.9999), n = 50 000, a
    gradient norm that swings between 0.2 and 1.8 (crossing the clip threshold every 20 steps, both ways); dmme_grad_norm feeds the
    clip, as in FusedAdam.step"""
    _lib, lib = _L()
    n, steps = 50_000, 200
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen) * 0.05
    grads = []
    for k in range(steps):
        g = torch.randn(n, generator=gen)
        grads.append(g * ((1.0 + 0.8 * math.sin(2 * math.pi * (k + 0.5) / 40)) / float(g.double().norm())))
    norms = [R.grad_norm(g) for g in grads]
    crossings = sum((a > 1.0) != (b > 1.0) for a, b in zip(norms, norms[1:]))
    assert crossings >= 8 and min(norms) < 0.3 and max(norms) > 1.7
    # float64, twice: with the float32 scalars the kernel is handed, and with the doubles torch is handed
    ref = {}
    for rounded in (True, False):
        p, m, v, ema = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p0.double()
        for k, g in enumerate(grads):
            p, m, v, ema = R.adam_step(p, g, m, v, ema, LR, B1, B2, EPS, k + 1, norms[k], 1.0, DECAY, 1.0, round_scalars=rounded)
        ref[rounded] = (p, ema)
    # the kernel
    P, M, V, E = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), p0.cuda()
    N, scratch = torch.zeros(1, device="cuda"), torch.empty(1024, device="cuda")
    for k, g in enumerate(grads):
        G = g.cuda()
        _lib.check(lib.dmme_grad_norm(_lib.ptr(G), n, _lib.ptr(N), _lib.ptr(scratch), _lib.stream_ptr()), "dmme_grad_norm")
        _lib.check(lib.dmme_adam_step(_lib.ptr(P), _lib.ptr(G), _lib.ptr(M), _lib.ptr(V), _lib.ptr(E), n, LR, B1, B2, EPS, k + 1, _lib.ptr(N), 1.0, DECAY, 1.0,
                                      _lib.stream_ptr()), "dmme_adam_step")
    torch.cuda.synchronize()
    # torch in float32 on the same device
    tp = p0.cuda().requires_grad_(True)
    topt = torch.optim.Adam([tp], lr=LR, betas=(B1, B2), eps=EPS)
    tema = p0.cuda()
    for g in grads:
        tp.grad = g.cuda()
        torch.nn.utils.clip_grad_norm_([tp], 1.0)
        topt.step()
        tema.mul_(DECAY).add_(tp.detach(), alpha=1.0 - DECAY)
    for name, ours, theirs, (want_k, want_t) in (("p", P, tp.detach(), (ref[True][0], ref[False][0])), ("ema", E, tema, (ref[True][1], ref[False][1]))):
        ek = (ours.cpu().double() - want_k).abs()
        et = (theirs.cpu().double() - want_t).abs()
        ulp_max, ulp_rms = 2.0**-23 * float(want_k.abs().max()), 2.0**-23 * float(want_k.pow(2).mean().sqrt())
        rk, rt = float(ek.pow(2).mean().sqrt()), float(et.pow(2).mean().sqrt())
        print(f"{name} after {steps} steps: kernel max {float(ek.max()):.3e} rms {rk:.3e}; torch fp32 max {float(et.max()):.3e} rms {rt:.3e}; "
              f"ratio max {float(ek.max()) / float(et.max()):.2f} rms {rk / rt:.2f}; the scalars' rounding alone moves it by {float((want_k - want_t).abs().max()):.3e}")
        assert float(ek.max()) <= 2.0 * float(et.max()) + ulp_max, name  # measured ratio: 1.07 (p), 0.74 (ema)
        assert rk <= 2.0 * rt + ulp_rms, name  # measured ratio: 1.00 (p), 0.70 (ema)


# ---------------------------------------------------------------- dmme_adam_step_amp, dmme_amp_scale
def _run_amp(p, buf, m, v, ema, state, max_norm, decay, gs, growth=2.0, backoff=0.5, interval=2000, norm=None):
    """-> tensors after the step, the scaler state after it, the norm the pass read (dmme_grad_norm of the buffer unless given)"""
    _lib, lib = _L()
    P, G, M, V, E = (_dev(x) for x in (p, buf, m, v, ema))
    A = torch.tensor(state, dtype=torch.float32, device="cuda")
    N, scratch = torch.zeros(1, device="cuda"), torch.empty(1024, device="cuda")
    if norm is None:
        _lib.check(lib.dmme_grad_norm(_lib.ptr(G), G.numel(), _lib.ptr(N), _lib.ptr(scratch), _lib.stream_ptr()), "dmme_grad_norm")
    else:
        N.fill_(norm)
    _lib.check(lib.dmme_adam_step_amp(_lib.ptr(P), _lib.ptr(G), _lib.ptr(M), _lib.ptr(V), _lib.ptr(E), P.numel(), LR, B1, B2, EPS, _lib.ptr(N), max_norm, decay, gs,
                                      _lib.ptr(A), growth, backoff, interval, _lib.stream_ptr()), "dmme_adam_step_amp")
    torch.cuda.synchronize()
    return {"p": P.cpu(), "m": M.cpu(), "v": V.cpu(), "ema": None if E is None else E.cpu()}, A.cpu().tolist(), float(N.item())


AMP_REGIMES = {k: REGIMES[k] for k in ("clipped", "not_clipped", "max_norm_0", "ema_null", "grad_scale_eighth_clipped", "grad_scale_eighth_not_clipped")}


@pytest.mark.parametrize("n", [5, 257, SWEEP + 3])
@pytest.mark.parametrize("log2_S", [-14, 16, 24])
@pytest.mark.parametrize("regime", list(AMP_REGIMES))
def test_adam_step_amp_regimes(regime, log2_S, n):
    """the buffer holds S x (1 / grad_scale) x the mean gradient; bias correction from the state's steps-taken (9 -> t = 10)"""
    mean_norm, max_norm, _, with_ema, gs = AMP_REGIMES[regime]
    S = 2.0**log2_S
    p, g, m, v, ema = _case(n, 300 + n % 89, mean_norm / gs)
    m, v = m * gs, v * gs * gs
    buf = g * S  # (exact: a power of two, no overflow or underflow at these magnitudes)
    ema = ema if with_ema else None
    state = [S, 1.0, 9.0, 0.0, 4.0, 0.0, 0.0, 0.0]
    got, after, norm = _run_amp(p, buf, m, v, ema, state, max_norm, DECAY, gs, interval=3, norm=R.f32(R.grad_norm(buf)))
    *_, want_state = R.amp_step(p, buf, m, v, ema, LR, B1, B2, EPS, norm, max_norm, DECAY, gs, state, 2.0, 0.5, 3, round_scalars=True)
    assert after == want_state == [S, 2.0, 10.0, 0.0, 4.0, 0.0, 0.0, 0.0]
    args = (p, buf, m, v, ema, LR, B1, B2, EPS, 10, norm, max_norm, DECAY, R.f32(gs) / S)
    want_p = R.amp_step(p, buf, m, v, ema, LR, B1, B2, EPS, norm, max_norm, DECAY, gs, state, 2.0, 0.5, 3, round_scalars=True)[0]
    assert torch.equal(want_p, R.adam_step(*args, round_scalars=True)[0])  # (the bounds below are for the step amp_step takes)
    worst = _check_step(got, args, f"{regime}, S = 2^{log2_S}, n = {n}")
    print(f"{regime}, S = 2^{log2_S}, n = {n}: worst error in units of the bound {worst}")


@pytest.mark.parametrize("n", [7, SWEEP + 3])  # n % 4 == 3: the last element sits in the norm's scalar tail
@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
@pytest.mark.parametrize("where", ["first", "last"])
def test_adam_step_amp_skips_a_non_finite_step(bad, where, n):
    assert n % 4 == 3
    p, g, m, v, ema = _case(n, 17, 3.0)
    buf = g * 1024.0
    buf[0 if where == "first" else n - 1] = bad
    state = [1024.0, 2.0, 6.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    got, after, norm = _run_amp(p, buf, m, v, ema, state, 1.0, DECAY, 0.125, interval=3)
    assert not math.isfinite(norm)
    for k, before in (("p", p), ("m", m), ("v", v), ("ema", ema)):
        assert torch.equal(got[k].view(torch.int32), before.view(torch.int32)), k  # bit-identical
    # scale x back-off, tracker 0, steps taken unchanged, found_inf, skipped + 1
    assert after == [512.0, 0.0, 6.0, 1.0, 2.0, 0.0, 0.0, 0.0]
    assert after == R.amp_step(p, buf, m, v, ema, LR, B1, B2, EPS, norm, 1.0, DECAY, 0.125, state, 2.0, 0.5, 3, round_scalars=True)[4]


@pytest.mark.parametrize("interval", [1, 3])
def test_adam_step_amp_grows_the_scale_exactly_at_the_interval(interval):
    """seven steps, the fifth not finite: state and tensors carried on BOTH sides (each step is held to its own one-step bound from the
    kernel's own previous output); the scale doubles exactly when the tracker reaches `interval`"""
    n = 257
    gen = torch.Generator().manual_seed(3)
    p, _, m, v, ema = _case(n, 19, 1.0)
    m, v = torch.zeros(n), torch.zeros(n)
    state = R.amp_init(256.0)
    scales = []
    for k in range(7):
        g = torch.randn(n, generator=gen) * (0.2 if k % 2 else 0.01)
        buf = g * R.f32(state[R.SCALE])
        if k == 4:
            buf[n - 1] = math.inf
        got, after, norm = _run_amp(p, buf, m, v, ema, state, 1.0, DECAY, 1.0, interval=interval)
        *_, want_state = R.amp_step(p, buf, m, v, ema, LR, B1, B2, EPS, norm, 1.0, DECAY, 1.0, state, 2.0, 0.5, interval, round_scalars=True)
        assert after == want_state, (k, after, want_state)
        if k != 4:
            _check_step(got, (p, buf, m, v, ema, LR, B1, B2, EPS, int(state[R.STEPS]) + 1, norm, 1.0, DECAY, 1.0 / state[R.SCALE]), f"step {k}")
        p, m, v, ema, state = got["p"], got["m"], got["v"], got["ema"], after
        scales.append(state[R.SCALE])
    want = {1: [512.0, 1024.0, 2048.0, 4096.0, 2048.0, 4096.0, 8192.0], 3: [256.0, 256.0, 512.0, 512.0, 256.0, 256.0, 256.0]}[interval]
    assert scales == want and state[R.STEPS] == 6.0 and state[R.SKIPPED] == 1.0


@pytest.mark.parametrize("n", [0, 1, SWEEP + 3])
def test_amp_scale_is_one_product_per_element(n):
    _lib, lib = _L()
    d = torch.randn(max(n, 1), generator=torch.Generator().manual_seed(n)) * 1e-3
    for S in (2.0**-14, 3.0, 65536.0):
        D = d.cuda()
        A = torch.tensor(R.amp_init(S), dtype=torch.float32, device="cuda")
        _lib.check(lib.dmme_amp_scale(_lib.ptr(D), n, _lib.ptr(A), _lib.stream_ptr()), "dmme_amp_scale")
        want = d.clone()
        want[:n] = R.amp_scale(d[:n], R.amp_init(S))
        assert torch.equal(D.cpu().view(torch.int32), want.view(torch.int32)), (n, S)


# ---------------------------------------------------------------- exchange kernels
def _same_bits(a, b):
    """bit for bit, NaN compared as NaN"""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a.float())
    if not torch.equal(nan, torch.isnan(b.float())):
        return False
    ia = a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32)
    ib = b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)
    return torch.equal(ia[~nan], ib[~nan])


def _exchange(g, recv, world, scale):
    """pack g, reduce recv, unpack the packed g - each against the restatement"""
    _lib, lib = _L()
    st = _lib.stream_ptr()
    n = g.numel()
    per = (n + world - 1) // world
    pad = per * world
    assert recv.shape == (world, per)
    G, RV = g.cuda(), recv.cuda()
    send = torch.full((pad,), 7.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.dmme_grad_pack_bf16(_lib.ptr(G), n, _lib.ptr(send), pad, st), "pack")
    want_send = R.pack_bf16(g, pad)
    assert _same_bits(send, want_send), "pack"
    shard = torch.full((per,), 7.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.dmme_shard_reduce_bf16(_lib.ptr(RV), world, per, scale, _lib.ptr(shard), st), "reduce")
    assert _same_bits(shard, R.shard_reduce_bf16(recv, scale)), "reduce"
    out = torch.full((n,), 7.0, device="cuda")
    _lib.check(lib.dmme_grad_unpack_bf16(_lib.ptr(send), n, _lib.ptr(out), st), "unpack")
    assert _same_bits(out, R.unpack_bf16(want_send, n)), "unpack"


@pytest.mark.parametrize("n,world", [(1, 1), (5, 3), (1000, 2), (4097, 4), (4097, 7), (1 << 20, 8), (SWEEP + 3, 2), (8 * SWEEP + 24, 8)])
def test_bf16_exchange_kernels_bit_for_bit(n, world):
    """(2^20 + 3, 2): pack and unpack take a second sweep of the 4096 x 256 grid; (8 x 2^20 + 24, 8): `per` = 2^20 + 3, so does the reduce"""
    gen = torch.Generator().manual_seed(n + world)
    per = (n + world - 1) // world
    g = torch.randn(n, generator=gen) * 3
    recv = (torch.randn(world, per, generator=gen) * 3).to(torch.bfloat16)
    _exchange(g, recv, world, 1.0 / world)


def test_bf16_exchange_kernels_at_the_edges_of_the_format():
    """exact ties (both ways: to the even neighbour below and above), one float32 step either side of a tie, the largest float32 values
    that still round to bf16's maximum and the first that round to inf, float32 and bf16 subnormals, -0, +-inf, NaN"""
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000,
            0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007FFFFF, 0x80000001, 0x80018000, 0x00000000, 0x80000000, 0x7F800000,
            0xFF800000, 0x7FC00000, 0x3F800000, 0x40490FDB]
    g = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)
    n = g.numel()
    for world, scale in ((1, 1.0), (3, 1.0 / 3), (2, 0.5), (2, 1.0)):
        per = (n + world - 1) // world
        row = R.pack_bf16(g, per * world)
        # every special value meets every other kind of neighbour: the rows are rotations of the same list
        recv = torch.stack([torch.roll(row, 5 * j)[:per] for j in range(world)])
        _exchange(g, recv, world, scale)
    # the order is sum, THEN scale: max + max overflows the fp32 sum and stays inf under x 0.5 (scaling first would give max); two halves of
    # max sum to max exactly, and only the scale 2 takes them over the top
    top = torch.tensor([0x7F7F0000, 0x7EFF0000], dtype=torch.int32).view(torch.float32).to(torch.bfloat16)
    recv = torch.stack([top.repeat(2), top.repeat(2)])
    assert R.shard_reduce_bf16(recv, 0.5).view(torch.int16).tolist() == [0x7F80, 0x7EFF] * 2
    assert R.shard_reduce_bf16(recv, 1.0).view(torch.int16).tolist() == [0x7F80, 0x7F7F] * 2
    assert R.shard_reduce_bf16(recv, 2.0).view(torch.int16).tolist() == [0x7F80, 0x7F80] * 2
    for scale in (0.5, 1.0, 2.0):
        _exchange(g[:8], recv, 2, scale)


# ---------------------------------------------------------------- FusedAdam on the device
def _tiny(precision, device="cuda"):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks, cfg.attention_depths,
                        precision=precision)
    net.load_state_dict(O.make_state_dict(cfg, 5), strict=True)
    return net.cuda() if device == "cuda" else net


def _set_grads(net, step, scale=0.1):
    net.flat_grad()
    gen = torch.Generator().manual_seed(100 + step)
    for _, p in net.named_parameters():
        p.grad.copy_((torch.randn(p.shape, generator=gen) * scale).to(p.device))


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_fused_adam_grad_norm_is_what_clip_grad_norm_returns(grad_scale):
    from dmme_amd.optim import FusedAdam

    net = _tiny("fp32")
    opt = FusedAdam(net.parameters(), lr=LR, max_grad_norm=1.0, ema_decay=DECAY)
    _set_grads(net, 0)
    mean = [(p.grad.detach().double().cpu() * grad_scale).requires_grad_(False) for p in net.parameters()]
    holders = [torch.zeros_like(x).requires_grad_(True) for x in mean]
    for h, x in zip(holders, mean):
        h.grad = x
    want = float(torch.nn.utils.clip_grad_norm_(holders, 1.0))
    opt.grad_scale = grad_scale
    opt.step()
    got = opt.grad_norm()
    n = net.flat_grad().numel()
    assert abs(got - want) <= (norm_rel_bound(n) + 2 * U) * want, (got, want)  # (+ the host's product with grad_scale)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_optimiser_state_survives_load_on_cpu_then_cuda(precision):
    """four steps on the GPU, uninterrupted, against: three steps, state_dict(), a fresh model and optimiser built ON THE CPU,
    load_state_dict, .cuda(), the fourth step.  p, m, v, the EMA copy, the step count (and under fp16 the loss-scaling state: the second
    step is skipped, so steps-taken differs from the step count, and the scale has moved) are the same bits.  Before the state followed
    the model, the fourth step found its moments on another device and restarted them at zero, the EMA copy at the live weights, the scale
    at 65536 and the bias correction at t = 1 - and under fp16 the CPU-side load launched dmme_amp_init on a host pointer."""
    from dmme_amd.optim import FusedAdam

    def make(device):
        net = _tiny(precision, device)
        return net, FusedAdam(net.parameters(), lr=1e-3, max_grad_norm=1.0, ema_decay=0.99, init_scale=1024.0, growth_interval=3)

    def one_step(net, opt, k):
        _set_grads(net, k, scale=0.1 * (1024.0 if precision == "fp16" else 1.0))
        if k == 1 and precision == "fp16":
            net.flat_grad()[-1] = math.inf
        opt.step()

    net, opt = make("cuda")
    for k in range(3):
        one_step(net, opt, k)
    torch.cuda.synchronize()
    ck = copy.deepcopy({"model": net.state_dict(), "opt": opt.state_dict()})
    one_step(net, opt, 3)
    want = {"p": net.flat_parameters().clone(), **{k: opt._flat_state[id(net)][k].clone() for k in ("m", "v", "ema")}}
    assert not torch.equal(want["ema"], want["p"]) and float(want["m"].abs().max()) > 0

    net2, opt2 = make("cpu")
    net2.load_state_dict(ck["model"])
    opt2.load_state_dict(ck["opt"])
    assert not net2.flat_parameters().is_cuda and not opt2._flat_state[id(net2)]["m"].is_cuda
    net2.cuda()
    one_step(net2, opt2, 3)
    torch.cuda.synchronize()
    got = {"p": net2.flat_parameters(), **{k: opt2._flat_state[id(net2)][k] for k in ("m", "v", "ema")}}
    for k in want:
        assert got[k].is_cuda and torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    assert opt2._step_count == opt._step_count == 4
    if precision == "fp16":
        a, b = net.amp_state().cpu().tolist(), net2.amp_state().cpu().tolist()
        assert a == b and a[R.STEPS] == 3.0 and a[R.SKIPPED] == 1.0 and a[R.SCALE] == 512.0, (a, b)
        assert net2.amp_state().is_cuda
    else:
        assert net2.amp_state() is None
