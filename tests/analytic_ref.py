"""CPU restatement of Analytic-DPM as dmme_amd.AnalyticDPM states it (Bao et al., ICLR 2022), in float64 numpy: the variance table from the
closed form, the exact Gaussian problem it is checked on, the per-image moment with its ordered accumulation, the rows of the K-step
variational bound (Gaussian KL, discretised-Gaussian NLL), and plain-fp32 versions of the two rows in the device's order of operations.
The reference project has no such sampler: this file is the yardstick.

    a = abar_{tau_i}, p = abar_{tau_{i-1}},  lambda^2 = eta^2 (1 - p) / (1 - a) (1 - a / p)   (0 where p = 1)
    sigma^2 = lambda^2 + (sqrt((1 - a) p / a) - sqrt(1 - p - lambda^2))^2 (1 - G_{tau_i})
    k0 = sqrt(p / a),  k1 = sqrt(1 - p - lambda^2) - k0 sqrt(1 - a);   mu_theta = k0 x_t + k1 eps_theta,  mu~ = k0 x_t + k1 eps
    KL row  = 0.5 (log sigma^2 - log lambda^2 + (lambda^2 + mean (mu~ - mu_theta)^2) / sigma^2 - 1)
    NLL row = mean -log max(Phi((x0 + 1/255 - mu_theta) / sigma) - Phi((x0 - 1/255 - mu_theta) / sigma), 1e-12), the bins open at +-1

The bounds are derived from the unit roundoff of fp32, the kernels' order of operations and their summation shape, not measured.  The
device library's erf, exp and log are taken at the accuracy the OpenCL full profile demands of them (16, 3 and 3 ulp); division and square
root round correctly."""

from __future__ import annotations

import math

import numpy as np

from .ddim_ref import alpha_bar  # noqa: F401  (the linear schedule the package holds)

U = 2.0 ** -24  # unit roundoff of fp32; one ulp is at most 2 U of the value
ULP_ERF, ULP_EXP, ULP_LOG = 16, 3, 3
FLOOR = 1e-12
K0, K1, LOG_S2, LOG_L2, SA, S1 = range(6)
_erf = np.vectorize(math.erf, otypes=[np.float64])


# ------------------------------------------------------------------------------------------ the variance table
def table(ab, tau, eta, G):
    """dict of float64 [S+1] arrays k0, k1, lam2, sigma2, upper (entry 0: the identity step, zeros)"""
    ab, G = np.asarray(ab, dtype=np.float64), np.asarray(G, dtype=np.float64)
    S = len(tau) - 1
    out = {k: np.zeros(S + 1) for k in ("k0", "k1", "lam2", "sigma2", "upper")}
    out["k0"][0] = 1.0
    for i in range(1, S + 1):
        a, p = ab[tau[i]], ab[tau[i - 1]]
        lam2 = 0.0 if p == 1.0 else eta * eta * (1.0 - p) / (1.0 - a) * (1.0 - a / p)
        root = math.sqrt(max(1.0 - p - lam2, 0.0))
        c = math.sqrt((1.0 - a) * p / a) - root
        out["k0"][i] = math.sqrt(p / a)
        out["k1"][i] = root - math.sqrt(p / a) * math.sqrt(1.0 - a)
        out["lam2"][i], out["sigma2"][i], out["upper"][i] = lam2, lam2 + c * c * (1.0 - G[tau[i]]), lam2 + c * c
    return out


def gaussian_moments(ab, s2):
    """G_t of data N(0, s2 I) under the optimal predictor eps*(x_t) = sqrt(1 - a) x_t / (a s2 + 1 - a): E eps*^2 = (1 - a) / (a s2 + 1 - a)"""
    ab = np.asarray(ab, dtype=np.float64)
    return (1.0 - ab) / (ab * s2 + 1.0 - ab)


def gaussian_posterior_variance(a, p, lam2, s2):
    """Var(x_{tau_{i-1}} | x_{tau_i}) per dimension for data N(0, s2 I): x_prev = sqrt(p) x0 + sqrt(1 - p - lam2) eps + lam z with
    eps = (x_t - sqrt(a) x0) / sqrt(1 - a), so x_prev = c x0 + (...) x_t + lam z with c = sqrt(p) - sqrt(1 - p - lam2) sqrt(a / (1 - a)),
    and Var(x0 | x_t) = 1 / (1 / s2 + a / (1 - a))"""
    c = math.sqrt(p) - math.sqrt(max(1.0 - p - lam2, 0.0)) * math.sqrt(a / (1.0 - a))
    return lam2 + c * c / (1.0 / s2 + a / (1.0 - a))


# ------------------------------------------------------------------------------------------ the summation shape
def sum_depth(chw: int) -> int:
    """roundings on the longest path of a per-image fp32 sum in the kernels: a thread's elements one after the other, six butterfly steps in
    the wave, the block's four waves; the partial sums of the up to 32 workgroups are added in double"""
    parts = min(32, max(1, -(-chw // 1024)))
    return -(-chw // (parts * 256)) + 6 + 4


# ------------------------------------------------------------------------------------------ the moment
def moment(eps) -> np.ndarray:
    """float64 [B]: mean over the image of eps^2 (eps: (B, chw), the eps plane only)"""
    e = np.asarray(eps, dtype=np.float64)
    return (e * e).mean(axis=1)


def moment_bound(eps) -> np.ndarray:
    """|device - float64| per image, as pfode_ref.dot_bound: every product enters by one fma (one rounding of the running sum), `sum_depth`
    roundings on the longest path, one more for the fp32 row; all terms are positive, so the sum itself is the sum of magnitudes"""
    e = np.asarray(eps, dtype=np.float64)
    return (sum_depth(e.shape[1]) + 2) * U * (e * e).mean(axis=1)


def accumulate(sums, counts, t, m, T):
    """the batch added in index order, in place (sums float64[T+1], counts int64[T+1]); returns the status flag"""
    status = 0
    for tb, mb in zip(np.asarray(t).tolist(), np.asarray(m, dtype=np.float64)):
        if tb < 1 or tb > T:
            status = 1
            continue
        sums[tb] += mb
        counts[tb] += 1
    return status


# ------------------------------------------------------------------------------------------ the rows of the bound
def true_eps(x_t, x_0, row):
    """float64: the noise re-derived from x_t and x_0 with the row's fp32 sqrt(abar), sqrt(1 - abar)"""
    return (np.asarray(x_t, dtype=np.float64) - float(row[SA]) * np.asarray(x_0, dtype=np.float64)) / float(row[S1])


def kl_row(eps_theta, x_t, x_0, row) -> np.ndarray:
    """float64 [B]; inputs (B, chw); row: the 8 fp32 values of the device table, read as float64"""
    e, xt = np.asarray(eps_theta, dtype=np.float64), np.asarray(x_t, dtype=np.float64)
    k0, k1, ls, ll = (float(row[j]) for j in (K0, K1, LOG_S2, LOG_L2))
    mu_theta, mu_true = k0 * xt + k1 * e, k0 * xt + k1 * true_eps(x_t, x_0, row)
    return (0.5 * (ls - ll + (math.exp(ll) + (mu_true - mu_theta) ** 2) / math.exp(ls) - 1.0)).mean(axis=1)


def kl_row_f32(eps_theta, x_t, x_0, row) -> np.ndarray:
    """the device's order in plain fp32 numpy: eps = (x_t - sa x0) / s1, d = k1 (eps - eps_theta), fp32 sum of d d; the closing expression in
    float64, rounded once"""
    f = np.float32
    e, xt, x0 = (np.asarray(v, dtype=f) for v in (eps_theta, x_t, x_0))
    eps = (xt - f(row[SA]) * x0) / f(row[S1])
    d = f(row[K1]) * (eps - e)
    m = (d * d).sum(axis=1, dtype=f).astype(np.float64) / e.shape[1]
    ls, ll = float(row[LOG_S2]), float(row[LOG_L2])
    return (0.5 * (ls - ll + (math.exp(ll) + m) / math.exp(ls) - 1.0)).astype(f)


def kl_bound(eps_theta, x_t, x_0, row) -> np.ndarray:
    """|device - float64| per image.  Per element, with u the unit roundoff: the product sa x0, the difference, the quotient, the difference
    to eps_theta and the product with k1 round once each, so
        |delta d| <= |k1| (u (|sa x0| + |x_t - sa x0|) / s1 + u |eps| + u |eps - eps_theta|) + u |d|
    and |delta d^2| <= 2 |d| |delta d| + delta d^2.  The sum adds (sum_depth + 2) u sum d^2.  The closing expression is formed in double and
    rounded once: 0.5 delta m / sigma^2 + u |row|.  The factor 1.01 covers the second-order terms."""
    e, xt, x0 = (np.asarray(v, dtype=np.float64) for v in (eps_theta, x_t, x_0))
    k1, sa, s1, ls = float(row[K1]), float(row[SA]), float(row[S1]), float(row[LOG_S2])
    eps = (xt - sa * x0) / s1
    d = k1 * (eps - e)
    dd = abs(k1) * (U * (np.abs(sa * x0) + np.abs(xt - sa * x0)) / s1 + U * np.abs(eps) + U * np.abs(eps - e)) + U * np.abs(d)
    dm = (2.0 * np.abs(d) * dd + dd * dd).mean(axis=1) + (sum_depth(e.shape[1]) + 2) * U * (d * d).mean(axis=1)
    return 1.01 * (0.5 * dm / math.exp(ls) + U * np.abs(kl_row(eps_theta, x_t, x_0, row)))


def _nll_terms(mean, x_0, sd):
    """float64 per element: (nll, prob, a+, a-, up, lo)"""
    x0 = np.asarray(x_0, dtype=np.float64)
    ap, am = (x0 + 1.0 / 255.0 - mean) / sd, (x0 - 1.0 / 255.0 - mean) / sd
    up, lo = x0 < 1.0, x0 > -1.0
    Fp = np.where(up, 0.5 * (1.0 + _erf(ap / math.sqrt(2.0))), 1.0)
    Fm = np.where(lo, 0.5 * (1.0 + _erf(am / math.sqrt(2.0))), 0.0)
    prob = Fp - Fm
    return -np.log(np.maximum(prob, FLOOR)), prob, ap, am, up, lo


def nll_row(eps_theta, x_t, x_0, row) -> np.ndarray:
    """float64 [B]: the discretised-Gaussian NLL of x_0 under N(k0 x_t + k1 eps_theta, exp(log sigma^2))"""
    e, xt = np.asarray(eps_theta, dtype=np.float64), np.asarray(x_t, dtype=np.float64)
    mean = float(row[K0]) * xt + float(row[K1]) * e
    return _nll_terms(mean, x_0, math.sqrt(math.exp(float(row[LOG_S2]))))[0].mean(axis=1)


def nll_row_f32(eps_theta, x_t, x_0, row) -> np.ndarray:
    """the device's order in plain fp32 numpy (erf through float64 and rounded: at most half an ulp, inside the 16 the bound allows)"""
    f = np.float32
    e, xt, x0 = (np.asarray(v, dtype=f) for v in (eps_theta, x_t, x_0))
    mean = f(row[K0]) * xt + f(row[K1]) * e
    sd = np.sqrt(np.exp(f(row[LOG_S2])))
    c = f(1.0) / f(255.0)
    ap, am = (x0 + c - mean) / sd, (x0 - c - mean) / sd
    h = f(0.70710678118654752)
    Fp = np.where(x0 < 1, f(0.5) * (f(1.0) + _erf((ap * h).astype(np.float64)).astype(f)), f(1.0)).astype(f)
    Fm = np.where(x0 > -1, f(0.5) * (f(1.0) + _erf((am * h).astype(np.float64)).astype(f)), f(0.0)).astype(f)
    nll = -np.log(np.maximum(Fp - Fm, f(FLOOR)))
    return (nll.sum(axis=1, dtype=f).astype(np.float64) / e.shape[1]).astype(f)


def mean_error_analytic(eps_theta, x_t, row) -> np.ndarray:
    """|delta mean| per element of mean = (k0 x_t) + (k1 eps_theta): two products and a sum, one rounding each"""
    e, xt = np.asarray(eps_theta, dtype=np.float64), np.asarray(x_t, dtype=np.float64)
    k0, k1 = float(row[K0]), float(row[K1])
    return U * (np.abs(k0 * xt) + np.abs(k1 * e) + np.abs(k0 * xt + k1 * e))


def nll_bound(mean, dmean, x_0, log_s2: float) -> np.ndarray:
    """|device - float64| per image of the NLL row, for a device mean that is within `dmean` of `mean` (both per element, float64).
        sd = sqrt(exp(log s2)):  relative error (ULP_EXP 2u) / 2 + u
        a  = ((x0 + c) - mean) / sd:  |delta a| <= (u |x0 + c| + u c + dmean + u |x0 + c - mean|) / sd + |a| (rel(sd) + u)
        arg = a h, h the fp32 1/sqrt(2):  |delta arg| <= |delta a| / sqrt(2) + 2 u |arg|
        F  = 0.5 (1 + erf(arg)):  |delta F| <= (1 / sqrt(pi)) exp(-max(|arg| - |delta arg|, 0)^2) |delta arg| + ULP_ERF u |erf| + 2 u F
        prob = F+ - F-:  |delta prob| <= |delta F+| + |delta F-| + u prob  (an open bin's side is exact)
        nll = -log max(prob, 1e-12):  the device's prob lies in [prob - |delta prob|, prob + |delta prob|] and the floor is applied to it, so
             |delta nll| <= max(log(max(prob + dp, F) / max(prob, F)), log(max(prob, F) / max(prob - dp, F))) + ULP_LOG 2u |nll|
             (finite everywhere; wide where prob is within dp of the floor, as it must be)
    and the sum adds (sum_depth + 2) u sum |nll|, the fp32 row one more rounding.  The factor 1.01 covers the second-order terms."""
    x0 = np.asarray(x_0, dtype=np.float64)
    sd = math.sqrt(math.exp(log_s2))
    rel_sd = ULP_EXP * U + U
    c = 1.0 / 255.0
    nll, prob, ap, am, up, lo = _nll_terms(mean, x0, sd)

    def dF(a, sign, open_side):
        num = x0 + sign * c - mean
        da = (U * np.abs(x0 + sign * c) + U * c + dmean + U * np.abs(num)) / sd + np.abs(a) * (rel_sd + U)
        arg = a / math.sqrt(2.0)
        darg = da / math.sqrt(2.0) + 2.0 * U * np.abs(arg)
        slope = np.exp(-np.maximum(np.abs(arg) - darg, 0.0) ** 2) / math.sqrt(math.pi)
        F = 0.5 * (1.0 + _erf(arg))
        return np.where(open_side, slope * darg + ULP_ERF * U * np.abs(_erf(arg)) + 2.0 * U * F, 0.0)

    dprob = dF(ap, 1.0, up) + dF(am, -1.0, lo) + U * np.abs(prob)
    pc, lo_p, hi_p = np.maximum(prob, FLOOR), np.maximum(prob - dprob, FLOOR), np.maximum(prob + dprob, FLOOR)
    dnll = np.maximum(np.log(hi_p / pc), np.log(pc / lo_p)) + ULP_LOG * 2.0 * U * np.abs(nll)
    D = x0.shape[1]
    return 1.01 * (dnll.mean(axis=1) + (sum_depth(D) + 3) * U * np.abs(nll).mean(axis=1))


def nll_bound_analytic(eps_theta, x_t, x_0, row) -> np.ndarray:
    e, xt = np.asarray(eps_theta, dtype=np.float64), np.asarray(x_t, dtype=np.float64)
    mean = float(row[K0]) * xt + float(row[K1]) * e
    return nll_bound(mean, mean_error_analytic(eps_theta, x_t, row), x_0, float(row[LOG_S2]))


def nll_saturated_interval(eps_theta, x_t, x_0, row, margin: float = 8.0):
    """(lo [B], hi [B], decided-outside [B], undecided [B]) of the NLL row where the deviation is so small that the bins are all but decided
    (the floored variance 1e-12: sd = 1e-6 against bins of 2/255).  With |delta a| as in `nll_bound`, an element whose a+ and a- both lie
    further than `margin` from 0 after that error is decided: erf of an argument beyond 8 / sqrt(2) is +-1 to the last bit of fp32 (1 - erf(5.6)
    = 2e-15, and every erff saturates there by an explicit branch - the one thing assumed beyond the 16 ulp), so the element's probability is
    exactly 1 (x0's bin holds the mean: NLL 0) or exactly 0 (it does not: the floor, NLL log 1e12, good to the logarithm's 3 ulp and the
    rounding of the fp32 constant).  An undecided element lies anywhere between.  The sum adds (sum_depth + 3) u."""
    e, xt = np.asarray(eps_theta, dtype=np.float64), np.asarray(x_t, dtype=np.float64)
    x0 = np.asarray(x_0, dtype=np.float64)
    mean = float(row[K0]) * xt + float(row[K1]) * e
    dmean = mean_error_analytic(eps_theta, x_t, row)
    sd = math.sqrt(math.exp(float(row[LOG_S2])))
    c = 1.0 / 255.0
    _, _, ap, am, up, lo = _nll_terms(mean, x0, sd)

    def side(a, sign, open_side):  # +1: surely above the mean's side (F = 1), -1: surely below (F = 0), 0: undecided
        num = x0 + sign * c - mean
        da = (U * np.abs(x0 + sign * c) + U * c + dmean + U * np.abs(num)) / sd + np.abs(a) * (ULP_EXP * U + 2.0 * U)
        decided = np.abs(a) - da > margin
        return np.where(open_side, np.where(decided, np.sign(a), 0.0), sign)  # (a closed side: F+ = 1 at x0 = 1, F- = 0 at x0 = -1)

    sp, sm = side(ap, 1.0, up), side(am, -1.0, lo)
    undecided = (sp == 0) | (sm == 0)
    outside = ~undecided & (sp == sm)
    D = x0.shape[1]
    L, slack = -math.log(FLOOR), (1.0 + 2.0 * ULP_LOG * U + 2.0 * U) * (1.0 + (sum_depth(D) + 3) * U)
    n_out, n_und = outside.sum(axis=1), undecided.sum(axis=1)
    return n_out * L / slack / D, (n_out + n_und) * L * slack / D, n_out, n_und


def vlb_rows(eps_theta, x_t, x_0, idx, coef):
    """(rows float64 [B], bound [B], status) of a batch with per-image indices; coef: float32 [S+1][8]"""
    e, xt, x0 = (np.asarray(v, dtype=np.float64).reshape(len(idx), -1) for v in (eps_theta, x_t, x_0))
    S = coef.shape[0] - 1
    rows, bound, status = np.full(len(idx), np.nan), np.zeros(len(idx)), 0
    for b, i in enumerate(np.asarray(idx).tolist()):
        if i < 1 or i > S:
            status = 1
            continue
        args = (e[b:b + 1], xt[b:b + 1], x0[b:b + 1], coef[i])
        rows[b], bound[b] = (nll_row(*args)[0], nll_bound_analytic(*args)[0]) if i == 1 else (kl_row(*args)[0], kl_bound(*args)[0])
    return rows, bound, status


def prior_rows(x0, abar_T: float) -> np.ndarray:
    """KL(q(x_T | x_0) || N(0, I)) per image, nats/dim (tests/iddpm_paper_ref.py: prior_rows)"""
    a = float(abar_T)
    x = np.asarray(x0, dtype=np.float64).reshape(len(x0), -1)
    return (0.5 * ((-np.log1p(-a) - a) + a * x * x)).mean(axis=1)
