"""CPU restatement of progressive distillation (Salimans & Ho, ICLR 2022, Algorithm 2) on the discrete linear grid, as
dmme_amd.ProgressiveDistillation states it.  The reference project has no such method: this file is the yardstick.

- the grid and the tables [N+1][12] / [N+1][2] in float64 from an alpha_bar table (include/dmme_hip.h: dmme_distill_*);
- the three kernels in float32 numpy, every product and sum rounded on its own: what the device does, bit for bit;
- Algorithm 2 literally in float64, the paper's quotient x~ = (z_e - r z_t) / (alpha_e - r alpha_t) included;
- first-order forward bounds of the kernels' expressions as written, accumulated stage by stage in float64: every fp32 product or sum
  contributes 2^-24 of its result's magnitude, every rounded table entry 2^-24 of its term, inherited errors pass through the absolute
  coefficients (as tests/ilvr_ref.update_bound does it)."""

from __future__ import annotations

from typing import Callable, Union

import numpy as np

from .ddim_ref import alpha_bar  # noqa: F401  (the linear schedule the package holds)

P0, P1, P0M, P1M, M0, M1, W1, W2, Q0, Q1 = range(10)
ROW = 12
EPS = 2.0 ** -24  # the unit roundoff of float32
PREDICTIONS = ("eps", "x0", "v")
f32 = np.float32


def grid(T: int, N: int) -> np.ndarray:
    """int64 [2N+1]: equations.ddim.linear_tau(T, 2N) restated: round-half-even of the float32 product (T / 2N) i"""
    i = np.arange(0, 2 * N + 1).astype(np.float32)
    return np.round(f32(T / (2 * N)) * i).astype(np.int64)


def _pair(pred: str, alpha: float, sigma: float):
    return {"eps": (-sigma / alpha, 1.0 / alpha), "x0": (1.0, 0.0), "v": (-sigma, alpha)}[pred]


def tables(ab: np.ndarray, N: int, pred: str):
    """(rows float64 [N+1][12], tt int64 [N+1][2]); row 0 is NaN"""
    ab = np.asarray(ab, dtype=np.float64)
    tau = grid(ab.size - 1, N)
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    rows = np.zeros((N + 1, ROW))
    rows[0] = np.nan
    tt = np.zeros((N + 1, 2), dtype=np.int64)
    for i in range(1, N + 1):
        t, m, e = (int(tau[2 * i - k]) for k in range(3))
        r = rows[i]
        r[P0], r[P1] = _pair(pred, al[t], sg[t])
        r[P0M], r[P1M] = _pair(pred, al[m], sg[m])
        r[M1] = sg[m] / sg[t]
        r[M0] = al[m] - r[M1] * al[t]
        if e == 0:
            r[W1], r[W2] = 0.0, 1.0
        else:
            s_t, s_m, s_e = al[t] / sg[t], al[m] / sg[m], al[e] / sg[e]
            r[W1], r[W2] = (s_m - s_t) / (s_e - s_t), (s_e - s_m) / (s_e - s_t)
        r[Q0], r[Q1] = {"eps": (-al[t] / sg[t], 1.0 / sg[t]), "x0": (1.0, 0.0), "v": (-1.0 / sg[t], al[t] / sg[t])}[pred]
        tt[i] = (t, m)
    return rows, tt


# ------------------------------------------------------------------------------------------ the kernels in float32
def _per_image(v: np.ndarray, like: np.ndarray) -> np.ndarray:
    return np.asarray(v).reshape((-1,) + (1,) * (like.ndim - 1))


def _rows32(rows32: np.ndarray, idx: np.ndarray, N: int) -> np.ndarray:
    """[B][12] float32: the row of every image, NaN where the index lies outside 1..N (never used as an address)"""
    idx = np.asarray(idx, dtype=np.int64)
    bad = (idx < 1) | (idx > N)
    out = np.asarray(rows32, dtype=np.float32).reshape(-1, ROW)[np.where(bad, 0, idx)].copy()
    out[bad] = np.nan
    return out


def _axpby32(c0, c1, a, b):
    """(c0 a) + (c1 b) over float32 operands: two products and one sum, each rounded to float32 on its own"""
    return ((c0 * a).astype(np.float32) + (c1 * b).astype(np.float32)).astype(np.float32)


def _x0_32(p0, p1, o, z, clip):
    x = _axpby32(p0, p1, o, z)
    return np.where(x < f32(-1), f32(-1), np.where(x > f32(1), f32(1), x)).astype(np.float32) if clip else x


def noise32(x0, z, idx, tt, sqrt_abar32, sqrt_1m_abar32, N):
    """(z_t float32, t int64, m int64, status) of dmme_distill_noise"""
    x0, z = np.asarray(x0, dtype=np.float32), np.asarray(z, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    bad = (idx < 1) | (idx > N)
    safe = np.where(bad, 0, idx)
    tt = np.asarray(tt, dtype=np.int64).reshape(-1, 2)
    t, m = np.where(bad, 0, tt[safe, 0]), np.where(bad, 0, tt[safe, 1])
    sa = np.where(bad, f32(np.nan), np.asarray(sqrt_abar32, dtype=np.float32)[t]).astype(np.float32)
    sd = np.where(bad, f32(np.nan), np.asarray(sqrt_1m_abar32, dtype=np.float32)[t]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        z_t = _axpby32(_per_image(sa, x0), _per_image(sd, x0), x0, z)
    return z_t, t, m, int(bad.any())


def mid32(clip, z_t, out1, rows32, idx, N):
    """z_m of dmme_distill_mid"""
    z_t, out1 = np.asarray(z_t, dtype=np.float32), np.asarray(out1, dtype=np.float32)
    r = _rows32(rows32, idx, N)
    c = lambda k: _per_image(r[:, k], z_t)  # noqa: E731
    with np.errstate(invalid="ignore"):
        return _axpby32(c(M0), c(M1), _x0_32(c(P0), c(P1), out1, z_t, clip), z_t)


def target32(clip, z_t, out1, z_m, out2, rows32, idx, N):
    """the student's target of dmme_distill_target"""
    z_t, out1, z_m, out2 = (np.asarray(v, dtype=np.float32) for v in (z_t, out1, z_m, out2))
    r = _rows32(rows32, idx, N)
    c = lambda k: _per_image(r[:, k], z_t)  # noqa: E731
    with np.errstate(invalid="ignore"):
        x1 = _x0_32(c(P0), c(P1), out1, z_t, clip)
        x2 = _x0_32(c(P0M), c(P1M), out2, z_m, clip)
        return _axpby32(c(Q0), c(Q1), _axpby32(c(W1), c(W2), x1, x2), z_t)


# ------------------------------------------------------------------------------------------ Algorithm 2, literally, in float64
def _x0_of(pred: str, out, z, alpha, sigma):
    if pred == "eps":
        return (z - sigma * out) / alpha
    if pred == "x0":
        return out
    return alpha * z - sigma * out


def algorithm2(pred: str, clip: bool, ab: np.ndarray, N: int, idx, z_t, out1, out2: Union[np.ndarray, Callable], form: str = "quotient"):
    """float64 dict(x1, z_m, x2, x_tilde, target) of the paper's Algorithm 2 for images at the student indices `idx`: two DDIM steps of the
    teacher, t -> m -> e, then the x~ for which one DDIM step t -> e lands on z_e, as the paper's quotient (`form="quotient"`) or as the
    convex combination of the two x0 estimates (`form="convex"`, float64 weights); `out1`: the teacher's output at (z_t, t); `out2`: its
    output at (z_m, m), or a callable (z_m float64, m int64[B]) -> output"""
    ab = np.asarray(ab, dtype=np.float64)
    tau = grid(ab.size - 1, N)
    idx = np.asarray(idx, dtype=np.int64)
    z_t, out1 = np.asarray(z_t, dtype=np.float64), np.asarray(out1, dtype=np.float64)
    t, m, e = tau[2 * idx], tau[2 * idx - 1], tau[2 * idx - 2]
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    a_t, a_m, a_e, s_t, s_m, s_e = (_per_image(v, z_t) for v in (al[t], al[m], al[e], sg[t], sg[m], sg[e]))
    cl = (lambda x: np.clip(x, -1.0, 1.0)) if clip else (lambda x: x)
    x1 = cl(_x0_of(pred, out1, z_t, a_t, s_t))
    z_m = a_m * x1 + (s_m / s_t) * (z_t - a_t * x1)
    o2 = np.asarray(out2(z_m, m) if callable(out2) else out2, dtype=np.float64)
    x2 = cl(_x0_of(pred, o2, z_m, a_m, s_m))
    if form == "quotient":
        z_e = a_e * x2 + (s_e / s_m) * (z_m - a_m * x2)
        r = s_e / s_t
        x_tilde = (z_e - r * z_t) / (a_e - r * a_t)
    else:
        rows, _ = tables(ab, N, pred)
        x_tilde = _per_image(rows[idx, W1], z_t) * x1 + _per_image(rows[idx, W2], z_t) * x2
    eps_tilde = (z_t - a_t * x_tilde) / s_t
    target = {"eps": eps_tilde, "x0": x_tilde, "v": a_t * eps_tilde - s_t * x_tilde}[pred]
    return {"x1": x1, "z_m": z_m, "x2": x2, "x_tilde": x_tilde, "target": target, "t": t, "m": m}


def quotient32(ab: np.ndarray, N: int, idx, z_t, x1, x2):
    """the paper's quotient in float32 from float32 scalars: what the device would compute had it formed z_e - and why it does not"""
    ab = np.asarray(ab, dtype=np.float64)
    tau = grid(ab.size - 1, N)
    idx = np.asarray(idx, dtype=np.int64)
    t, m, e = tau[2 * idx], tau[2 * idx - 1], tau[2 * idx - 2]
    al, sg = np.sqrt(ab).astype(np.float32), np.sqrt(1.0 - ab).astype(np.float32)
    z_t, x1, x2 = (np.asarray(v, dtype=np.float32) for v in (z_t, x1, x2))
    a_t, a_m, a_e, s_t, s_m, s_e = (_per_image(v, z_t) for v in (al[t], al[m], al[e], sg[t], sg[m], sg[e]))
    z_m = a_m * x1 + (s_m / s_t) * (z_t - a_t * x1)
    z_e = a_e * x2 + (s_e / s_m) * (z_m - a_m * x2)
    r = s_e / s_t
    return ((z_e - r * z_t) / (a_e - r * a_t)).astype(np.float32)


# ------------------------------------------------------------------------------------------ the error bounds the GPU tests ask for
def _axpby_bound(c0, c1, a, b, da=0.0, db=0.0):
    """|fl(fl(c0' a') + fl(c1' b')) - (c0 a + c1 b)| to first order, c' the fp32-rounded float64 scalar, a', b' within da, db of a, b:
    |c0| da + |c1| db inherited, and for each term its scalar's rounding, its product's rounding and its share of the sum's rounding"""
    return np.abs(c0) * da + np.abs(c1) * db + 3.0 * EPS * (np.abs(c0 * a) + np.abs(c1 * b))


def bounds(clip: bool, rows64: np.ndarray, idx, z_t, out1, out2, d_out1=0.0, d_out2=0.0):
    """float64 dict(x1, z_m, x2, x_tilde, target) of elementwise bounds on the kernels' results against Algorithm 2 in float64 on the same
    float32 z_t, with the device's teacher outputs within `d_out1` / `d_out2` of `out1` / `out2` (0: the same arrays).  `d_out2` may be a
    callable (z_m, bound on z_m) -> bound: a teacher evaluated at the device's z_m instead of the exact one hands its own error in there.
    The clamp is 1-Lipschitz and rounds nothing."""
    idx = np.asarray(idx, dtype=np.int64)
    z_t, out1, out2 = (np.asarray(v, dtype=np.float64) for v in (z_t, out1, out2))
    r = np.asarray(rows64, dtype=np.float64).reshape(-1, ROW)[idx]
    c = lambda k: _per_image(r[:, k], z_t)  # noqa: E731
    cl = (lambda x: np.clip(x, -1.0, 1.0)) if clip else (lambda x: x)
    x1 = cl(c(P0) * out1 + c(P1) * z_t)
    b_x1 = _axpby_bound(c(P0), c(P1), out1, z_t, d_out1)
    z_m = c(M0) * x1 + c(M1) * z_t
    b_zm = _axpby_bound(c(M0), c(M1), x1, z_t, b_x1)
    x2 = cl(c(P0M) * out2 + c(P1M) * z_m)
    b_x2 = _axpby_bound(c(P0M), c(P1M), out2, z_m, d_out2(z_m, b_zm) if callable(d_out2) else d_out2, b_zm)
    xt = c(W1) * x1 + c(W2) * x2
    b_xt = _axpby_bound(c(W1), c(W2), x1, x2, b_x1, b_x2)
    b_t = _axpby_bound(c(Q0), c(Q1), xt, z_t, b_xt)
    return {"x1": b_x1, "z_m": b_zm, "x2": b_x2, "x_tilde": b_xt, "target": b_t}


def gddim_bound(k0: float, k1: float, a: float, b: float, x, out):
    """bound on GeneralizedDDIM's eager step x' = k0 x + k1 e, e = a out + b x (the x0 / v adapter; an eps network: a = 1, b = 0 and e = out
    exactly), against the same expression in float64 over the float64 scalars: the adapter's axpby, then the update's, plus 2^-24 |x'|
    for the update's third term (k2 z with k2 = 0, added or not)"""
    x, out = np.asarray(x, dtype=np.float64), np.asarray(out, dtype=np.float64)
    e = a * out + b * x
    b_e = 0.0 if (a, b) == (1.0, 0.0) else _axpby_bound(a, b, out, x)
    return _axpby_bound(k0, k1, x, e, 0.0, b_e) + EPS * np.abs(k0 * x + k1 * e)


def loss_bound(w: np.ndarray, out, target, d_target):
    """bound on the weighted MSE 1/(B chw) sum_b w_b sum_j (out - target)^2 in fp32 against float64, the device's target within d_target
    of the exact one: the first-order term 2 |out - target| d_target and the second-order one, the difference's and the square's rounding
    (3 x 2^-24 of each square), the weight's rounding and product (2 x 2^-24), and an fp32 sum of n non-negative terms in any order
    ((n + 2) 2^-24 of the sum, n = B chw)"""
    out, target, d_target = (np.asarray(v, dtype=np.float64) for v in (out, target, d_target))
    d = np.abs(out - target)
    wb = _per_image(np.asarray(w, dtype=np.float64), out)
    n = out.size
    exact = float((wb * d * d).sum() / n)
    inherited = float((wb * (2.0 * d * d_target + d_target * d_target)).sum() / n)
    return inherited + (n + 7.0) * EPS * (exact + inherited)
