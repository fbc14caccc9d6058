"""numpy restatement of the x0 / v prediction adapter and of the weighted loss (include/dmme_hip.h: dmme_pred_to_eps, dmme_q_sample_pred,
dmme_mse_loss_rows), written from the formulas and independent of the package:

- the adapter's tables [T+1][2] and the loss-weight tables [T+1] in float64 from an alpha_bar table;
- `to_eps` and `target` in float32 with the device's order of operations: numpy rounds every float32 product, sum and difference on
  its own, so the kernels are held to these bit for bit (the same functions run in float64 when handed float64 arrays);
- the weighted loss and its gradient in float64."""

import numpy as np

EPS, X0, V = "eps", "x0", "v"


def linear_alpha_bar(T=1000, start=1e-4, end=0.02):
    """float64 alpha_bar [T+1] of the linear beta schedule, alpha_bar[0] = 1"""
    beta = np.concatenate([[0.0], np.linspace(start, end, T, dtype=np.float64)])
    return np.cumprod(1.0 - beta)


def cosine_alpha_bar(T=1000, offset=0.008):
    """float64 alpha_bar [T+1] of Nichol & Dhariwal's cosine schedule with their clip beta <= 0.999 (which keeps alpha_bar_T above zero),
    alpha_bar[0] = 1 exactly"""
    f = np.cos((np.arange(T + 1, dtype=np.float64) / T + offset) / (1 + offset) * np.pi / 2) ** 2
    beta = np.concatenate([[0.0], np.clip(1.0 - f[1:] / f[:-1], 0.0, 0.999)])
    return np.cumprod(1.0 - beta)


def ab_table(alpha_bar, pred):
    """float64 [T+1][2]: eps = a_t * out + b_t * x_t.  x0: from x_t = sqrt(abar) x0 + sqrt(1-abar) eps; v: from v = sqrt(abar) eps -
    sqrt(1-abar) x0 and the same x_t, which give eps = sqrt(abar) v + sqrt(1-abar) x_t.  Row 0 of x0 (abar = 1) is NaN."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    out = np.empty((ab.size, 2), dtype=np.float64)
    if pred == X0:
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, 0] = -np.sqrt(ab) / np.sqrt(1 - ab)
            out[:, 1] = 1.0 / np.sqrt(1 - ab)
        out[ab >= 1.0] = np.nan
    elif pred == V:
        out[:, 0] = np.sqrt(ab)
        out[:, 1] = np.sqrt(1 - ab)
    else:
        raise ValueError(pred)
    return out


def weight_table(alpha_bar, pred, gamma=5.0):
    """float64 [T+1] min-SNR-gamma weights, snr = abar/(1-abar): eps min(snr, g)/snr, x0 min(snr, g), v min(snr, g)/(snr+1); index 0
    (snr infinite) holds the limits 0, g, 0"""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    w = np.empty_like(ab)
    for i, a in enumerate(ab):
        if a >= 1.0:
            w[i] = gamma if pred == X0 else 0.0
            continue
        snr = a / (1 - a)
        c = min(snr, gamma)
        w[i] = c / snr if pred == EPS else c if pred == X0 else c / (snr + 1)
    return w


def _rows(t, B):
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    return np.broadcast_to(t, (B,)) if t.size == 1 else t


def to_eps(table, out, x, t):
    """(a[t_b] * out_b) + (b[t_b] * x_b) in the dtype of `out` (float32: three separately rounded operations); table: [T+1][2] already
    in that dtype; out, x: (B, ...); t: one timestep or B"""
    out, x = np.asarray(out), np.asarray(x)
    tab = np.asarray(table, dtype=out.dtype)
    tt = _rows(t, out.shape[0])
    shape = (-1,) + (1,) * (out.ndim - 1)
    a, b = tab[tt, 0].reshape(shape), tab[tt, 1].reshape(shape)
    return (a * out) + (b * x)


def q_sample(sqrt_ab, sqrt_1m, x0, z, t):
    """x_t = (sa * x0) + (sd * z) in the dtype of x0, with the tables in that dtype"""
    x0, z = np.asarray(x0), np.asarray(z)
    tt = _rows(t, x0.shape[0])
    shape = (-1,) + (1,) * (x0.ndim - 1)
    sa, sd = np.asarray(sqrt_ab, dtype=x0.dtype)[tt].reshape(shape), np.asarray(sqrt_1m, dtype=x0.dtype)[tt].reshape(shape)
    return (sa * x0) + (sd * z)


def target(pred, sqrt_ab, sqrt_1m, x0, z, t):
    """the regression target in the dtype of x0: eps -> (x_t - sa x0)/sd (re-derived, as the eps loss has always done), x0 -> x0,
    v -> (sa * z) - (sd * x0)"""
    x0, z = np.asarray(x0), np.asarray(z)
    tt = _rows(t, x0.shape[0])
    shape = (-1,) + (1,) * (x0.ndim - 1)
    sa, sd = np.asarray(sqrt_ab, dtype=x0.dtype)[tt].reshape(shape), np.asarray(sqrt_1m, dtype=x0.dtype)[tt].reshape(shape)
    if pred == X0:
        return x0.copy()
    if pred == V:
        return (sa * z) - (sd * x0)
    mean = sa * x0
    return ((mean + sd * z) - mean) / sd


def weighted_loss(out, tgt, w_table, t, grad_scale=1.0):
    """float64 (loss, d_out): loss = 1/numel sum_b w[t_b] sum_j (out - tgt)^2, d_out = (out - tgt) 2 w[t_b] grad_scale / numel; the
    weights are the table's values as given (the fp32 device table, widened)"""
    o, g = np.asarray(out, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    w = np.asarray(w_table, dtype=np.float64)[_rows(t, o.shape[0])].reshape((-1,) + (1,) * (o.ndim - 1))
    d = o - g
    return float((w * d * d).sum() / o.size), d * (2.0 * w * grad_scale / o.size)
