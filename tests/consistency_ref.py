"""CPU restatement of consistency distillation (Song, Dhariwal, Chen & Sutskever 2023, Algorithm 2) on the discrete linear grid with the
boundary scalings of Latent Consistency Models, as dmme_amd.ConsistencyDistillation states it.  The reference project has no such
method: this file is the yardstick.

- the grid and the tables [N+1][12] / [N+1][2] in float64 from an alpha_bar table (include/dmme_hip.h: dmme_cm_*);
- the launches in float32 numpy, every product and sum rounded on its own, the per-image scalars in float64 rounded once: what the
  device does, bit for bit (the per-image sum of squares excepted: its order of summation is the device's own);
- Algorithm 2 literally in float64 (numpy for the target, torch autograd for the loss and its gradient), and multistep sampling
  x' = alpha_p f(x, a) + sigma_p z literally;
- first-order forward bounds of the expressions as written, accumulated stage by stage in float64 as tests/distill_ref.py does it: every
  fp32 product or sum contributes 2^-24 of its result's magnitude, every rounded table entry 2^-24 of its term, inherited errors pass
  through the absolute coefficients.

The first six slots of a row and `tt` have progressive distillation's layout, so distill_ref.noise32 and distill_ref.mid32 restate the
two launches this method shares with it."""

from __future__ import annotations

from typing import Callable, Union

import numpy as np

from .distill_ref import EPS, PREDICTIONS, _axpby32, _axpby_bound, _per_image, _rows32, _x0_32, _x0_of, alpha_bar, mid32, noise32  # noqa: F401

P0, P1, P0M, P1M, M0, M1, CS, CO, CSM, COM = range(10)
ROW = 12
f32 = np.float32
SIGMA_DATA, TIMESTEP_SCALING, HUBER_C = 0.5, 10.0, 0.00054
PSEUDO_HUBER, L2 = 0, 1


def grid(T: int, N: int) -> np.ndarray:
    """int64 [N+1]: equations.ddim.linear_tau(T, N) restated: round-half-even of the float32 product (T / N) i"""
    i = np.arange(0, N + 1).astype(np.float32)
    return np.round(f32(T / N) * i).astype(np.int64)


def scalings(t, sd: float = SIGMA_DATA, s: float = TIMESTEP_SCALING):
    """(cs(t), co(t)) in float64; t a number or an array"""
    st = s * np.asarray(t, dtype=np.float64)
    return sd * sd / (st * st + sd * sd), st / np.sqrt(st * st + sd * sd)


def _pair(pred: str, alpha: float, sigma: float):
    return {"eps": (-sigma / alpha, 1.0 / alpha), "x0": (1.0, 0.0), "v": (-sigma, alpha)}[pred]


def tables(ab: np.ndarray, N: int, pred: str, sd: float = SIGMA_DATA, s: float = TIMESTEP_SCALING):
    """(rows float64 [N+1][12], tt int64 [N+1][2]); row 0 is NaN"""
    ab = np.asarray(ab, dtype=np.float64)
    tau = grid(ab.size - 1, N)
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    rows = np.zeros((N + 1, ROW))
    rows[0] = np.nan
    tt = np.zeros((N + 1, 2), dtype=np.int64)
    for i in range(1, N + 1):
        t, m = int(tau[i]), int(tau[i - 1])
        r = rows[i]
        r[P0], r[P1] = _pair(pred, al[t], sg[t])
        r[P0M], r[P1M] = _pair(pred, al[m], sg[m])
        r[M1] = sg[m] / sg[t]
        r[M0] = al[m] - r[M1] * al[t]
        r[CS], r[CO] = scalings(t, sd, s)
        r[CSM], r[COM] = scalings(m, sd, s)
        tt[i] = (t, max(m, 1))
    return rows, tt


def sampler_rows(ab: np.ndarray, K: int, sd: float = SIGMA_DATA, s: float = TIMESTEP_SCALING) -> np.ndarray:
    """float64 [K+1][3]: (k0, k1, k2) of the step tau[i] -> tau[i-1] in the eps form"""
    ab = np.asarray(ab, dtype=np.float64)
    tau = grid(ab.size - 1, K)
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    out = np.zeros((K + 1, 3))
    out[0, 0] = 1.0
    for i in range(1, K + 1):
        a, p = int(tau[i]), int(tau[i - 1])
        cs, co = scalings(a, sd, s)
        out[i] = (al[p] * (cs + co / al[a]), -al[p] * co * sg[a] / al[a], sg[p] if p > 0 else 0.0)
    return out


# ------------------------------------------------------------------------------------------ the launches in float32
def f32_of(c0, c1, p0, p1, out, z, clip):
    """THE consistency function as the device evaluates it: (c0 z) + (c1 x0), x0 = (p0 out) + (p1 z) clamped iff clip"""
    return _axpby32(c0, c1, z, _x0_32(p0, p1, out, z, clip))


def target32(clip, z_m, out_m, rows32, idx, N):
    """f_target of dmme_cm_target"""
    z_m, out_m = np.asarray(z_m, dtype=np.float32), np.asarray(out_m, dtype=np.float32)
    r = _rows32(rows32, idx, N)
    c = lambda k: _per_image(r[:, k], z_m)  # noqa: E731
    with np.errstate(invalid="ignore"):
        return f32_of(c(CSM), c(COM), c(P0M), c(P1M), out_m, z_m, clip)


def diff32(z_t, out, f_target, rows32, idx, N):
    """f(z_t, t; out) - f_target, float32, as both loss launches form it (the student's x0 is never clamped)"""
    z_t, out, f_target = (np.asarray(v, dtype=np.float32) for v in (z_t, out, f_target))
    r = _rows32(rows32, idx, N)
    c = lambda k: _per_image(r[:, k], z_t)  # noqa: E731
    with np.errstate(invalid="ignore"):
        return (f32_of(c(CS), c(CO), c(P0), c(P1), out, z_t, False) - f_target).astype(np.float32)


def squares32(z_t, out, f_target, rows32, idx, N):
    """the float32 squares whose per-image sum is S_b"""
    d = diff32(z_t, out, f_target, rows32, idx, N)
    with np.errstate(invalid="ignore"):
        return (d * d).astype(np.float32)


def finish(metric: int, sumsq32, rows32, idx, N, chw: int, c32, grad_scale32):
    """(d_b float32 [B], g_b float32 [B]) from the per-image sums: in float64, each rounded once - the finishing launch of dmme_cm_loss.
    c32, grad_scale32: the float32 values the entry point receives."""
    S = np.asarray(sumsq32, dtype=np.float32).astype(np.float64)
    B = S.size
    r = _rows32(rows32, idx, N).astype(np.float64)
    c, gs = float(f32(c32)), float(f32(grad_scale32))
    with np.errstate(invalid="ignore"):
        num = (gs * r[:, CO]) * r[:, P0]
        if metric == PSEUDO_HUBER:
            root = np.sqrt(S + c * c)
            d, g = root - c, num / (float(B) * root)
        else:
            d, g = S / float(chw), (2.0 * num) / (float(B) * float(chw))
        return d.astype(np.float32), g.astype(np.float32)


def d_out32(g32, z_t, out, f_target, rows32, idx, N):
    """d_out of dmme_cm_loss: (g_b diff), one float32 product"""
    d = diff32(z_t, out, f_target, rows32, idx, N)
    with np.errstate(invalid="ignore"):
        return (_per_image(np.asarray(g32, dtype=np.float32), d) * d).astype(np.float32)


def ema32(dst, src, decay):
    """dst = (dst decay) + (src one_minus), one_minus = (float)(1.0 - (double)decay)"""
    dst, src = np.asarray(dst, dtype=np.float32), np.asarray(src, dtype=np.float32)
    d = f32(decay)
    return _axpby32(d, f32(1.0 - float(d)), dst, src)


# ------------------------------------------------------------------------------------------ Algorithm 2, literally, in float64
def _scal(ab, N, idx, like):
    ab = np.asarray(ab, dtype=np.float64)
    tau = grid(ab.size - 1, N)
    idx = np.asarray(idx, dtype=np.int64)
    t, m = tau[idx], tau[idx - 1]
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    return t, m, tuple(_per_image(v, like) for v in (al[t], al[m], sg[t], sg[m]))


def algorithm2(pred: str, clip: bool, ab: np.ndarray, N: int, idx, z_t, out1, out_m: Union[np.ndarray, Callable], sd: float = SIGMA_DATA,
               s: float = TIMESTEP_SCALING):
    """float64 dict(x1, z_m, x0_m, f_target, t, m): the teacher's x0 estimate at (z_t, t), one DDIM step to zh_m, the target network's
    consistency function at (zh_m, m).  `out1`: the teacher's output at (z_t, t); `out_m`: the target network's output at (zh_m, max(m, 1)),
    or a callable (zh_m float64, timesteps int64[B]) -> output"""
    z_t, out1 = np.asarray(z_t, dtype=np.float64), np.asarray(out1, dtype=np.float64)
    t, m, (a_t, a_m, s_t, s_m) = _scal(ab, N, idx, z_t)
    cl = (lambda x: np.clip(x, -1.0, 1.0)) if clip else (lambda x: x)
    x1 = cl(_x0_of(pred, out1, z_t, a_t, s_t))
    z_m = a_m * x1 + (s_m / s_t) * (z_t - a_t * x1)
    om = np.asarray(out_m(z_m, np.maximum(m, 1)) if callable(out_m) else out_m, dtype=np.float64)
    x0_m = cl(_x0_of(pred, om, z_m, a_m, s_m))
    cs_m, co_m = (_per_image(v, z_t) for v in scalings(m, sd, s))
    return {"x1": x1, "z_m": z_m, "x0_m": x0_m, "f_target": cs_m * z_m + co_m * x0_m, "t": t, "m": m}


def loss64(pred: str, metric: int, ab: np.ndarray, N: int, idx, z_t, out, f_target, c: float, sd: float = SIGMA_DATA, s: float = TIMESTEP_SCALING,
           grad_scale: float = 1.0):
    """(loss, d loss / d out times grad_scale, S_b, f - f_target) in float64 by torch autograd of the literal loss
    (1/B) sum_b d(f(z_t, t; out)_b, f_target_b) on the CPU"""
    import torch

    z = torch.from_numpy(np.asarray(z_t, dtype=np.float64))
    o = torch.from_numpy(np.asarray(out, dtype=np.float64).copy()).requires_grad_(True)
    ft = torch.from_numpy(np.asarray(f_target, dtype=np.float64))
    t, _, (a_t, _, s_t, _) = _scal(ab, N, idx, np.asarray(z_t))
    a_t, s_t = torch.from_numpy(np.ascontiguousarray(a_t)), torch.from_numpy(np.ascontiguousarray(s_t))
    cs, co = (torch.from_numpy(np.ascontiguousarray(_per_image(v, np.asarray(z_t)))) for v in scalings(t, sd, s))
    x0 = (z - s_t * o) / a_t if pred == "eps" else o if pred == "x0" else a_t * z - s_t * o
    e = cs * z + co * x0 - ft
    S = (e * e).reshape(e.shape[0], -1).sum(dim=1)
    d = torch.sqrt(S + c * c) - c if metric == PSEUDO_HUBER else S / e[0].numel()
    loss = d.mean()
    (loss * grad_scale).backward()
    return float(loss.detach()), o.grad.numpy(), S.detach().numpy(), e.detach().numpy()


def sample_step64(pred: str, ab: np.ndarray, K: int, i: int, x, out, z=None, sd: float = SIGMA_DATA, s: float = TIMESTEP_SCALING):
    """x' = alpha_p f(x, a) + sigma_p z for the step a = tau[i] -> p = tau[i-1] of the K-point grid, literally, in float64, from the
    network's raw output `out` at (x, a)"""
    ab = np.asarray(ab, dtype=np.float64)
    tau = grid(ab.size - 1, K)
    a, p = int(tau[i]), int(tau[i - 1])
    x, out = np.asarray(x, dtype=np.float64), np.asarray(out, dtype=np.float64)
    cs, co = scalings(a, sd, s)
    f = cs * x + co * _x0_of(pred, out, x, np.sqrt(ab[a]), np.sqrt(1.0 - ab[a]))
    return np.sqrt(ab[p]) * f + (np.sqrt(1.0 - ab[p]) * np.asarray(z, dtype=np.float64) if p > 0 else 0.0)


# ------------------------------------------------------------------------------------------ the error bounds the GPU tests ask for
def target_bounds(clip: bool, rows64: np.ndarray, idx, z_t, out1, out_m, d_out1=0.0, d_out_m=0.0):
    """float64 dict(x1, z_m, f_target) of elementwise bounds on dmme_distill_mid's and dmme_cm_target's results against `algorithm2` on
    the same float32 z_t, with the device's network outputs within d_out1 / d_out_m of out1 / out_m (0: the same arrays; d_out_m may be a
    callable (zh_m, bound on zh_m) -> bound).  The clamp is 1-Lipschitz and rounds nothing."""
    idx = np.asarray(idx, dtype=np.int64)
    z_t, out1, out_m = (np.asarray(v, dtype=np.float64) for v in (z_t, out1, out_m))
    r = np.asarray(rows64, dtype=np.float64).reshape(-1, ROW)[idx]
    c = lambda k: _per_image(r[:, k], z_t)  # noqa: E731
    cl = (lambda x: np.clip(x, -1.0, 1.0)) if clip else (lambda x: x)
    x1 = cl(c(P0) * out1 + c(P1) * z_t)
    b_x1 = _axpby_bound(c(P0), c(P1), out1, z_t, d_out1)
    z_m = c(M0) * x1 + c(M1) * z_t
    b_zm = _axpby_bound(c(M0), c(M1), x1, z_t, b_x1)
    x0m = cl(c(P0M) * out_m + c(P1M) * z_m)
    b_x0m = _axpby_bound(c(P0M), c(P1M), out_m, z_m, d_out_m(z_m, b_zm) if callable(d_out_m) else d_out_m, b_zm)
    b_ft = _axpby_bound(c(CSM), c(COM), z_m, x0m, b_zm, b_x0m)
    return {"x1": b_x1, "z_m": b_zm, "f_target": b_ft}


def loss_bounds(metric: int, rows64: np.ndarray, idx, z_t, out, f_target, d_f_target, c: float, grad_scale: float = 1.0):
    """dict(sumsq [B], loss, grad [B][chw]) of bounds on dmme_cm_loss against `loss64` at the exact f_target, the device's f_target
    within d_f_target of it, c and grad_scale being the float32 values both sides use:
      f           the student's axpby twice (x0, then f)
      e = f - ft  b_f + d_f_target, and 2^-24 |e| for the difference
      e^2         2 |e| b_e + b_e^2, and 2^-24 e^2 for the product
      S_b         the terms' bounds, and (chw + 1) 2^-24 of the sum: n non-negative float32 terms in any order
      d_b         pseudo-Huber: b_S / (2 sqrt(S + c^2)); L2: b_S / chw; and 2^-24 d_b for the one rounding of the float64 value
      loss        the mean of the b_d, and (B + 2) 2^-24 of the loss: B non-negative terms in any order, 1/B rounded, one product
      g_b         3 x 2^-24 |g_b| (co, p0 rounded in the table, g_b rounded once); pseudo-Huber: and |g_b| b_S / (2 (S + c^2))
      grad        |g_b| b_e + b_g |e| + b_g b_e, and 2^-24 |g_b e| for the product"""
    idx = np.asarray(idx, dtype=np.int64)
    z_t, out, f_target = (np.asarray(v, dtype=np.float64) for v in (z_t, out, f_target))
    r = np.asarray(rows64, dtype=np.float64).reshape(-1, ROW)[idx]
    c_ = lambda k: _per_image(r[:, k], z_t)  # noqa: E731
    B, chw = z_t.shape[0], z_t[0].size
    x0 = c_(P0) * out + c_(P1) * z_t
    b_x0 = _axpby_bound(c_(P0), c_(P1), out, z_t)
    f = c_(CS) * z_t + c_(CO) * x0
    b_f = _axpby_bound(c_(CS), c_(CO), z_t, x0, 0.0, b_x0)
    e = f - f_target
    b_e = b_f + d_f_target + EPS * np.abs(e)
    b_sq = 2.0 * np.abs(e) * b_e + b_e * b_e + EPS * e * e
    S = (e * e).reshape(B, -1).sum(axis=1)
    b_S = b_sq.reshape(B, -1).sum(axis=1)
    b_S = b_S + (chw + 1.0) * EPS * (S + b_S)
    num = grad_scale * r[:, CO] * r[:, P0]
    if metric == PSEUDO_HUBER:
        root = np.sqrt(S + c * c)
        d, g = root - c, num / (B * root)
        b_d = b_S / (2.0 * root) + EPS * d
        b_g = np.abs(g) * (3.0 * EPS + b_S / (2.0 * root * root))
    else:
        d, g = S / chw, 2.0 * num / (B * chw)
        b_d = b_S / chw + EPS * d
        b_g = np.abs(g) * 3.0 * EPS
    loss = float(d.mean())
    b_loss = float(b_d.mean()) + (B + 2.0) * EPS * (loss + float(b_d.mean()))
    g_, bg_ = _per_image(g, z_t), _per_image(b_g, z_t)
    b_grad = np.abs(g_) * b_e + bg_ * np.abs(e) + bg_ * b_e + EPS * np.abs(g_ * e)
    return {"sumsq": b_S, "loss": b_loss, "grad": b_grad}


def sample_step_bound(k, a: float, b: float, x, out, z=None):
    """bound on ConsistencySampler's eager step x' = (k0 x + k1 e) + k2 z, e = a out + b x (the x0 / v adapter; an eps network: a = 1, b = 0
    and e = out exactly), against `sample_step64`: the adapter's axpby, the update's axpby, then for the noise term k2's rounding, its
    product and the sum (3 x 2^-24 |k2 z|) and 2^-24 of the first two terms' sum for the last addition (made or not); 1e-13 of the
    magnitudes for the float64 evaluation of the eps form and of the literal form themselves (k0 and k1 nearly cancel for a v network)"""
    k0, k1, k2 = (float(v) for v in k)
    x, out = np.asarray(x, dtype=np.float64), np.asarray(out, dtype=np.float64)
    e = a * out + b * x
    b_e = 0.0 if (a, b) == (1.0, 0.0) else _axpby_bound(a, b, out, x)
    inner = k0 * x + k1 * e
    noise = 0.0 if k2 == 0.0 else np.abs(k2 * np.asarray(z, dtype=np.float64))
    return _axpby_bound(k0, k1, x, e, 0.0, b_e) + EPS * np.abs(inner) + 3.0 * EPS * noise + 1e-13 * (np.abs(k0 * x) + np.abs(k1 * e))
