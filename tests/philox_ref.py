"""numpy reference of the library's device random streams (dmme_randn, dmme_dropout_masks, the noise of dmme_chain_update).

The stream contract, which this module states independently of the HIP source:

- Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), round multipliers
  0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85.
- A span is (seed, offset, numel); offset counts quads, each Philox call yields 4 words.  Quad q of the span uses the 64-bit
  counter offset + q (mod 2^64), laid out as the counter words {lo, hi, 0, 0}; the key is the seed as {lo, hi}.
- Uniform of a word x: u = ((x >> 8) + 1) / 2^24, on the grid {k / 2^24 : k = 1 .. 2^24}, so u lies in (0, 1] and is exact in fp32.
- Normals: per quad, words (x0, x1) and (x2, x3) each give one Box-Muller pair
      z0, z1 = r cos a, r sin a   with r = sqrt(-2 ln u(x0)),  a = fp32(fp32(2 pi) * u(x1)),
  and z2, z3 the same from (x2, x3).  The angle product is the one rounding the kernel makes that the reference must repeat
  (the device code is compiled without fma contraction); everything else is evaluated here in fp64.  u >= 2^-24 bounds every
  value: |z| <= sqrt(48 ln 2) = 5.768.
- Value order: quad q fills elements 4q .. 4q+3 (z0, z1, z2, z3, or the four uniforms); the last quad is cut off at numel and the
  rest of its words are discarded.  A span therefore consumes ceil(numel / 4) counters.
- Dropout2d multipliers (p in fp32): element i is 0 if u_i <= p, else fp32(1) / fp32(1 - p); drop probability
  floor(p * 2^24) / 2^24.  The dropout draws key the generator with seed ^ DROPOUT_KEY_XOR (models/ddpm.py).
"""

from __future__ import annotations

import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
TWO_PI_F32 = np.float32(2.0 * math.pi)
MAX_ABS_Z = math.sqrt(48.0 * math.log(2.0))  # r at u = 2^-24
DROPOUT_KEY_XOR = 0x5DEECE66D

# a word whose uniform is exactly 0.5 (x >> 8 == 2^23 - 1) under the dropout key of seed 1337, found by scanning counters from
# 2^32 + 1000 with this module: (key, counter, word index).  Tests of the drop rule u <= p at p = 0.5 place a span over it.
HALF_KEY, HALF_CTR, HALF_WORD = 1337 ^ DROPOUT_KEY_XOR, 4298399573, 1


def philox4x32_10(seed: int, counters) -> np.ndarray:
    """uint32[n, 4] outputs of Philox4x32-10 under the key {seed_lo, seed_hi}.

    `counters` is either a 1-D array of 64-bit counters (words {lo, hi, 0, 0}, the library's layout) or an [n, 4] array of full
    counter words (for published known-answer vectors)."""
    ctr = np.asarray(counters, dtype=np.uint64)
    if ctr.ndim == 2:
        assert ctr.shape[1] == 4
        c = [ctr[:, j] & np.uint64(MASK32) for j in range(4)]
    else:
        ctr = ctr.reshape(-1)
        zero = np.zeros_like(ctr)
        c = [ctr & np.uint64(MASK32), ctr >> np.uint64(32), zero, zero.copy()]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & MASK32, seed >> 32
    m0, m1, lo, sh = np.uint64(M0), np.uint64(M1), np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = c[0] * m0  # 32 x 32 -> 64 bits: exact in uint64
        p1 = c[2] * m1
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, axis=1).astype(np.uint32)


def _span_words(seed: int, offset: int, numel: int) -> np.ndarray:
    """uint32[ceil(numel / 4), 4]: the words of the span's quads"""
    quads = (int(numel) + 3) // 4
    ctr = np.arange(quads, dtype=np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF)  # wraps mod 2^64 like the device counter
    return philox4x32_10(seed, ctr)


def to_uniform(words) -> np.ndarray:
    """u = ((x >> 8) + 1) / 2^24 in float64 (exact; the same value in fp32)"""
    w = np.asarray(words, dtype=np.uint32)
    return ((w >> np.uint32(8)).astype(np.float64) + 1.0) * (1.0 / 16777216.0)


def uniforms(seed: int, offset: int, numel: int) -> np.ndarray:
    """float64[numel] uniforms of the span, in element order"""
    return to_uniform(_span_words(seed, offset, numel)).reshape(-1)[: int(numel)]


def normals(seed: int, offset: int, numel: int, with_radius: bool = False):
    """float64[numel] standard normals of the span (and, with_radius, the Box-Muller radius r of each element's pair)"""
    u = to_uniform(_span_words(seed, offset, numel))
    r = np.sqrt(-2.0 * np.log(u[:, 0::2]))  # [quads, 2]: radius of pair (x0, x1) and of pair (x2, x3)
    a = (TWO_PI_F32 * u[:, 1::2].astype(np.float32)).astype(np.float64)  # fp32 product, as on the device
    z = np.empty_like(u)
    z[:, 0::2] = r * np.cos(a)
    z[:, 1::2] = r * np.sin(a)
    z = z.reshape(-1)[: int(numel)]
    if with_radius:
        return z, np.repeat(r, 2, axis=1).reshape(-1)[: int(numel)]
    return z


def dropout_masks(seed: int, offset: int, numel: int, p: float) -> np.ndarray:
    """float32[numel] Dropout2d multipliers of the span: 0 where u <= p, else fp32(1) / fp32(1 - p)"""
    p32 = np.float32(p)
    keep = np.float32(1.0) / (np.float32(1.0) - p32)
    u = uniforms(seed, offset, numel).astype(np.float32)
    return np.where(u <= p32, np.float32(0.0), keep).astype(np.float32)
