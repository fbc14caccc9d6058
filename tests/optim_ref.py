"""float64 restatement of the optimiser tail (dmme_grad_norm, dmme_adam_step, dmme_adam_step_amp, dmme_amp_scale and the three bf16
exchange kernels), written from what the operations ARE - the comment blocks above the kernels (csrc/kernels_bwd.hip: "clip-by-global-
norm + Adam (+ EMA)", "dynamic loss scaling") and the reference's torch.optim.Adam + gradient_clip_val + EMA callback
(lit_modules/ddpm.py:127-141, callbacks/ema.py:169-176) - not from the kernels' code.  tests/test_optim_host.py pins it against
torch.optim.Adam / clip_grad_norm_ / GradScaler on the CPU; tests/test_gpu_optim.py holds the kernels against it.

One step, in this order:
    g  <- grad_scale * g                                        (1 / world of a sum-reducing exchange; grad_scale / S under loss scaling)
    g  <- g * c  where c = max_norm / (grad_scale * norm + 1e-6), applied only when c < 1 (and max_norm > 0 and a norm is given)
    m  <- b1 m + (1 - b1) g ;  v <- b2 v + (1 - b2) g^2
    p  <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    ema <- d ema + (1 - d) p
Everything is float64.  `round_scalars=True` rounds the scalar arguments to float32 first - the C ABI takes `float`, so the kernel never
sees 0.9 or 2e-4 but their float32 neighbours; without the switch they stay Python doubles, which is what torch.optim.Adam uses."""

from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

SCALE_FLOOR = 2.0**-14  # a loss scale never backs off below this (csrc/kernels_bwd.hip: "floor 2^-14")
SCALE, TRACKER, STEPS, FOUND_INF, SKIPPED = range(5)  # the first five of the scaler state's 8 floats


def f32(x: float) -> float:
    return float(np.float32(x))


def grad_norm(g: Tensor) -> float:
    """L2 norm of a buffer, accumulated in float64"""
    return float(g.detach().double().cpu().pow(2).sum().sqrt())


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, ema: Optional[Tensor], lr: float, b1: float, b2: float, eps: float, t: int,
              norm: Optional[float], max_norm: float, decay: float, grad_scale: float, round_scalars: bool = False,
              eps_placement: str = "adam") -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """-> (p, m, v, ema) after the step; inputs are not modified.  `eps_placement` other than "adam" selects one of the two mutants
    the sensitivity checks use: "inside_sqrt" (sqrt(v_hat + eps)) and "before_bias_correction" ((sqrt(v) + eps) / sqrt(1 - b2^t))."""
    tiny = 1e-6
    if round_scalars:
        lr, b1, b2, eps, max_norm, decay, grad_scale, tiny = (f32(x) for x in (lr, b1, b2, eps, max_norm, decay, grad_scale, tiny))
        norm = None if norm is None else f32(norm)
    p, g, m, v = (x.detach().double() for x in (p, g, m, v))
    g = g * grad_scale
    if norm is not None and max_norm > 0:
        c = max_norm / (grad_scale * norm + tiny)
        if c < 1.0:
            g = g * c
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1**t, 1.0 - b2**t
    if eps_placement == "adam":
        denom = v.sqrt() / math.sqrt(bc2) + eps
    elif eps_placement == "inside_sqrt":
        denom = (v / bc2 + eps).sqrt()
    elif eps_placement == "before_bias_correction":
        denom = (v.sqrt() + eps) / math.sqrt(bc2)
    else:
        raise ValueError(eps_placement)
    p = p - (lr / bc1) * m / denom
    if ema is not None:
        ema = decay * ema.detach().double() + (1.0 - decay) * p
    return p, m, v, ema


def adam_step_eps_inside_sqrt(*a, **kw):
    """mutant: eps under the square root"""
    return adam_step(*a, eps_placement="inside_sqrt", **kw)


def adam_step_eps_before_bias_correction(*a, **kw):
    """mutant: eps added to sqrt(v) before the bias correction divides"""
    return adam_step(*a, eps_placement="before_bias_correction", **kw)


def amp_init(init_scale: float) -> List[float]:
    return [float(init_scale), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def amp_scale(d: Tensor, state: List[float]) -> Tensor:
    """the loss gradient times S, in the tensor's own precision (one float32 product per element on the device)"""
    return d * torch.tensor(state[SCALE], dtype=d.dtype)


def amp_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, ema: Optional[Tensor], lr: float, b1: float, b2: float, eps: float,
             norm: float, max_norm: float, decay: float, grad_scale: float, state: List[float], growth: float, backoff: float,
             interval: int, round_scalars: bool = False):
    """adam_step inside torch.cuda.amp.GradScaler's state machine.  `g` is the SCALED gradient (S x gradient, times whatever
    `grad_scale` undoes), `norm` the L2 norm of that buffer.  -> (p, m, v, ema, new state); nothing is modified in place.
    The step is skipped when the scaled norm is not finite, or when 1 / S is not (a collapsed scale); a skip backs the scale off (never
    below 2^-14) and resets the growth tracker; a step taken counts towards the bias correction (t = steps taken + 1: skipped steps do
    not count, torch skips optimizer.step()) and `interval` of them in a row grow the scale."""
    st = list(state)
    S = st[SCALE]
    if round_scalars:
        with np.errstate(divide="ignore", over="ignore"):
            inv = float(np.float32(1.0) / np.float32(S))
    else:
        inv = 1.0 / S if S != 0 else math.inf
    if not (math.isfinite(norm) and math.isfinite(inv)):
        S = S * backoff
        st[SCALE] = S if S >= SCALE_FLOOR else SCALE_FLOOR  # (a NaN scale recovers to the floor as well)
        st[TRACKER] = 0.0
        st[FOUND_INF] = 1.0
        st[SKIPPED] += 1.0
        return p, m, v, ema, st
    if round_scalars:
        grad_scale = f32(grad_scale)
    # (the unscale factor is a float32 inside the fused pass; with a power-of-two S the quotient is exact either way)
    p, m, v, ema = adam_step(p, g, m, v, ema, lr, b1, b2, eps, int(st[STEPS]) + 1, norm, max_norm, decay, grad_scale / S, round_scalars=round_scalars)
    st[STEPS] += 1.0
    st[FOUND_INF] = 0.0
    st[TRACKER] += 1.0
    if st[TRACKER] >= interval:
        st[SCALE] = S * growth
        st[TRACKER] = 0.0
    return p, m, v, ema, st


# ---- gradient exchange with bf16 on the wire (distributed.Bf16ShardExchange): torch's own casts are the yardstick ----
def pack_bf16(g: Tensor, n_pad: int) -> Tensor:
    """fp32 slice -> bf16 (round to nearest even), zero padded to n_pad"""
    out = torch.zeros(n_pad, dtype=torch.bfloat16, device=g.device)
    out[: g.numel()] = g.to(torch.bfloat16)
    return out


def shard_reduce_bf16(recv: Tensor, scale: float) -> Tensor:
    """[world][per] bf16 -> fp32 sum in rank order (rank 0 first, starting from +0), ONE multiply by the float32 scale, ONE rounding"""
    acc = torch.zeros(recv.shape[1], dtype=torch.float32, device=recv.device)
    for j in range(recv.shape[0]):
        acc = acc + recv[j].float()
    return (acc * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16)


def unpack_bf16(src: Tensor, n: int) -> Tensor:
    return src[:n].float()


# ---- how far a correct float32 evaluation of ONE step may sit from the float64 one (first-order rounding analysis) ----
# u = 2^-24 is float32's unit roundoff; a product, sum or fused multiply-add carries (1 + d), |d| <= u.  Division, square root and powf
# are allowed one ulp (2u) each, so the bound holds whichever way the compiler lowers them.  Counts, per element:
#   clip factor   grad_scale / S (loss scaling only), grad_scale * norm, + 1e-6 (same sign), max_norm / ., c * grad_scale      <= 5 + 1 (the divide's second u)
#   g' = g * clip                                                                                                              K_G = 7
#   m  = b1 m + (1 - b1) g'   (1 - b1 is exact for b1 in [0.5, 1]); the two terms may cancel, so the error is ABSOLUTE:
#        <= K_M u (|b1 m| + |(1 - b1) g'|),  K_M = K_G + 2 (its product, the sum)                                              K_M = 9
#   v  = b2 v + ((1 - b2) g') g'   all terms >= 0, so the error is RELATIVE: 2 K_G + 2 products + the sum                      K_V = 17
#   bc = 1 - b^t: powf within 2u of b^t, the subtraction u  ->  relative error <= u (2 b^t / (1 - b^t) + 1) = u (2 (cond - 1) + 1),
#        cond = 1 / (1 - b^t): the conditioning of the bias correction (1000 for b2 = 0.999 at t = 1, 1.6 at t = 1000)
#   D  = sqrt(v) / sqrt(bc2) + eps:  K_V / 2 + 2 (sqrt)  +  (2 (cond2 - 1) + 1) / 2 + 2 (sqrt)  +  2 (divide)  +  1 (sum, same sign)
#   dp = (lr / bc1) * m / D:  2 (cond1 - 1) + 1 + 2 (divide)  +  1 (product)  +  2 (divide)  +  K_D,  relative to |dp|, PLUS m's absolute
#        error carried through:  K_M u (|b1 m| + |(1 - b1) g'|) * (lr / bc1) / D
#   p  = p - dp: one more rounding, <= one ulp of the larger of |p|, |p_new|  (nothing when p = 0: the precision cases start there)
#   ema = d ema + (1 - d) p  (1 - d exact): 2 u (|d ema| + |(1 - d) p|) + (1 - d) x p's error
U32 = 2.0**-24
K_G, K_M, K_V = 7, 9, 17


def gamma(k: float) -> float:
    return k * U32 / (1.0 - k * U32)  # (the usual gamma_k: the first-order count with its higher-order terms)


def update_rel_bound(b1: float, b2: float, t: int) -> float:
    """relative bound on the update dp (without the carried absolute error of m) at step t"""
    b1, b2 = f32(b1), f32(b2)
    c1, c2 = 1.0 / (1.0 - b1**t), 1.0 / (1.0 - b2**t)
    k_d = K_V / 2 + 2 + (2 * (c2 - 1) + 1) / 2 + 2 + 2 + 1
    return gamma(2 * (c1 - 1) + 1 + 2 + 1 + 2 + k_d)


def adam_step_bounds(p: Tensor, g: Tensor, m: Tensor, v: Tensor, ema: Optional[Tensor], lr: float, b1: float, b2: float, eps: float, t: int,
                     norm: Optional[float], max_norm: float, decay: float, grad_scale: float):
    """elementwise absolute bounds (float64 tensors) on |kernel - adam_step(..., round_scalars=True)| for m, v, p and ema"""
    pn, mn, vn, en = adam_step(p, g, m, v, ema, lr, b1, b2, eps, t, norm, max_norm, decay, grad_scale, round_scalars=True)
    lr, b1, b2, eps, max_norm, decay, grad_scale = (f32(x) for x in (lr, b1, b2, eps, max_norm, decay, grad_scale))
    p, g, m, v = (x.detach().double() for x in (p, g, m, v))
    gc = g * grad_scale
    if norm is not None and max_norm > 0:
        c = max_norm / (grad_scale * f32(norm) + f32(1e-6))
        if c < 1.0:
            gc = gc * c
    m_abs = (b1 * m).abs() + ((1.0 - b1) * gc).abs()
    bm = gamma(K_M) * m_abs
    bv = gamma(K_V) * vn
    denom = vn.sqrt() / math.sqrt(1.0 - b2**t) + eps
    step = lr / (1.0 - b1**t)
    dp = (pn - p).abs()
    bdp = update_rel_bound(b1, b2, t) * dp + bm * step / denom
    bp = bdp + 2.0 * U32 * torch.maximum(p.abs(), pn.abs()) * (p != 0)
    be = None
    if ema is not None:
        be = gamma(2) * ((decay * ema.detach().double()).abs() + ((1.0 - decay) * pn).abs()) + (1.0 - decay) * bp * (1 + 2 * U32)
    return {"m": bm, "v": bv, "p": bp, "ema": be}
