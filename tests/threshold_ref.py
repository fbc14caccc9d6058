"""numpy restatement of x0 thresholding (include/dmme_hip.h: dmme_x0_threshold): the float32 form, every product, sum, difference and
quotient rounded on its own and the order statistics from np.sort, which the kernels reproduce bit for bit; and a float64 form of the
same arithmetic over numpy.quantile.  Nothing here imports the package."""

import numpy as np

NONE, STATIC, DYNAMIC = 0, 1, 2
MODES = {"none": NONE, "static": STATIC, "dynamic": DYNAMIC}


def table64(alpha_bar):
    """float64 [T+1][4] = (A, B, C, D): x0 = A x - B eps, eps = C x - D x0; NaN rows where abar = 1"""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    out = np.full((ab.size, 4), np.nan)
    m = ab < 1.0
    sa, sd = np.sqrt(ab[m]), np.sqrt(1.0 - ab[m])
    out[m] = np.stack([1.0 / sa, sd / sa, 1.0 / sd, sa / sd], axis=1)
    return out


def table32(alpha_bar):
    return table64(alpha_bar).astype(np.float32)


def rank(p, n):
    """(k, frac): the order statistic below the p-quantile of n values and the float32 weight of the next one"""
    pos = float(p) * (n - 1)
    k = min(int(np.floor(pos)), n - 1)
    frac = np.float32(pos - k)
    return k, (np.float32(0.0) if k == n - 1 else frac)


def quantile32(a, p):
    """the p-quantile of the float32 values a with linear interpolation, as the kernels form it: a_k + frac (a_{k+1} - a_k), three
    float32 roundings behind frac's own; a_{k+1} is not read where frac == 0.  Returns (q, a_k, a_{k+1} or None)"""
    a = np.sort(np.asarray(a, dtype=np.float32).reshape(-1))
    k, frac = rank(p, a.size)
    if frac == 0:
        return a[k], a[k], None
    gap = np.float32(a[k + 1] - a[k])
    return np.float32(a[k] + np.float32(frac * gap)), a[k], a[k + 1]


def _rows(table, t, B):
    T = table.shape[0] - 1
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    assert t.size in (1, B)
    out = np.full((B, 4), np.nan, dtype=table.dtype)
    for b in range(B):
        tn = int(t[0 if t.size == 1 else b])
        if 0 <= tn <= T:
            out[b] = table[tn]
    return out


def threshold(mode, e, x, table, t, p=None, planes=1, halves=1, sg=1.0, dtype=np.float32):
    """(e', info) for e: [halves * B][planes * chw], x: [B][chw] in `dtype` (float32: the kernels' bits; float64: the same formulas,
    the quantile from numpy.quantile).  info: per image s, the count of touched elements, whether the image is non-finite, and x0."""
    f = dtype
    e = np.array(e, dtype=f, copy=True)
    x = np.asarray(x, dtype=f)
    B, chw = x.shape
    assert e.shape == (halves * B, planes * chw) and mode in (STATIC, DYNAMIC) and (halves == 1 or planes == 1)
    rows = _rows(np.asarray(table, dtype=f), t, B)
    sg = f(sg)
    info = {"s": np.ones(B, dtype=f), "touched": np.zeros(B, dtype=np.int64), "nonfinite": np.zeros(B, dtype=bool), "x0": np.zeros((B, chw), dtype=f),
            "mask": np.zeros((B, chw), dtype=bool)}
    with np.errstate(all="ignore"):
        for b in range(B):
            A, Bc, C, D = (f(v) for v in rows[b])
            ec = e[b, :chw]
            if halves == 2:
                eu = e[B + b]
                em = (eu + (sg * (ec - eu).astype(f)).astype(f)).astype(f)
            else:
                em = ec
            x0 = ((A * x[b]).astype(f) - (Bc * em).astype(f)).astype(f)
            a = np.abs(x0)
            bad = ~np.isfinite(x0)
            info["x0"][b], info["nonfinite"][b] = x0, bad.any()
            s = f(1.0)
            if mode == DYNAMIC:
                if bad.any():
                    e[b, :chw] = np.nan
                    if halves == 2:
                        e[B + b] = np.nan
                    info["s"][b], info["touched"][b], info["mask"][b] = np.nan, chw, True
                    continue
                q = quantile32(a, p)[0] if f is np.float32 else np.quantile(a, p, method="linear")
                s = f(q) if q > 1.0 else f(1.0)
            touched = bad | ~((s == 1.0) & (a <= 1.0))
            c = np.minimum(np.maximum(x0, -s), s)
            new = ((C * x[b]).astype(f) - (D * (c / s).astype(f)).astype(f)).astype(f)
            new[bad] = np.nan
            e[b, :chw][touched] = new[touched]
            if halves == 2:
                e[B + b][touched] = new[touched]
            info["s"][b], info["touched"][b], info["mask"][b] = s, int(touched.sum()), touched
    return e, info
