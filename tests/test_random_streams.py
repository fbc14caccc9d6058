"""The numpy reference of the device random streams (tests/philox_ref.py) on its own, no GPU: Random123's published known-answer
vectors, the span arithmetic (counters, carries, the cut last quad), a statistics battery on the normals, the Dropout2d drop rate,
and distinct keys across ranks.  tests/test_gpu_random.py holds the kernels to this reference."""

import math

import numpy as np
import pytest
import torch

from tests import philox_ref as P

# Random123 kat_vectors, philox4x32 10: counter words, key words -> output words
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

# (seed, offset in quads) of the statistics battery: fixed once, never re-picked to make a bound pass.  A seed >= 2^32 (the key's
# high word in use), offsets >= 2^32 (the counter's high word), and one span that crosses the low word's carry.
BATTERY = [(0, 0), (1337, 2**32 - 2**19), (2**63 + 12345, 2**40 + 7), (0xDEADBEEFCAFEF00D, 3 * 2**32 + 11)]
N_BATTERY = 2**22

@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    seed = key[0] | key[1] << 32
    got = P.philox4x32_10(seed, np.array([ctr], dtype=np.uint64))
    assert [int(v) for v in got[0]] == list(want)


def test_counter_layout_is_lo_hi_zero_zero():
    """a 64-bit counter is the counter words {lo, hi, 0, 0}"""
    seed = 0x0123456789ABCDEF
    ctrs = np.array([0, 1, 2**32 - 1, 2**32, 2**32 + 1, 2**40 + 7, 2**64 - 1], dtype=np.uint64)
    words = np.stack([ctrs & np.uint64(0xFFFFFFFF), ctrs >> np.uint64(32), 0 * ctrs, 0 * ctrs], axis=1)
    assert np.array_equal(P.philox4x32_10(seed, ctrs), P.philox4x32_10(seed, words))
    # the high words matter: counters 2^32 apart, and keys 2^32 apart, give different outputs
    assert not np.array_equal(P.philox4x32_10(seed, [5]), P.philox4x32_10(seed, [5 + 2**32]))
    assert not np.array_equal(P.philox4x32_10(seed, [5]), P.philox4x32_10(seed ^ 2**32, [5]))


def test_uniform_grid_and_bounds():
    w = np.array([0, 0xFF, 0x100, 0x7FFFFF00, 0x7FFFFFFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32)
    u = P.to_uniform(w)
    assert list(u) == [2.0**-24, 2.0**-24, 2.0**-23, 0.5, 0.5, 1.0, 1.0]
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)  # exact in fp32
    # the structural bound of the normals: r = sqrt(-2 ln 2^-24)
    assert math.isclose(math.sqrt(-2.0 * math.log(2.0**-24)), P.MAX_ABS_Z) and 5.768 < P.MAX_ABS_Z < 5.7683


@pytest.mark.parametrize("seed,offset", [(1337, 2**32 - 7), (2**63 + 12345, 0), (7, 2**40 + 7)])
def test_split_on_a_quad_boundary_leaves_the_stream_unchanged(seed, offset):
    """a span cut anywhere on a quad boundary, the second part starting k quads on, is the same values; spans that carry from
    the counter's low word into its high word included"""
    n = 4 * 12 + 3
    z = P.normals(seed, offset, n)
    u = P.uniforms(seed, offset, n)
    m = P.dropout_masks(seed, offset, n, 0.3)
    for k in range(0, n // 4 + 1):
        assert np.array_equal(np.concatenate([P.normals(seed, offset, 4 * k), P.normals(seed, offset + k, n - 4 * k)]), z), k
        assert np.array_equal(np.concatenate([P.uniforms(seed, offset, 4 * k), P.uniforms(seed, offset + k, n - 4 * k)]), u), k
        parts = [P.dropout_masks(seed, offset, 4 * k, 0.3), P.dropout_masks(seed, offset + k, n - 4 * k, 0.3)]
        assert np.array_equal(np.concatenate(parts), m), k
    # a prefix is the start of the longer span (the last quad is cut, never shifted)
    for short in range(1, n):
        assert np.array_equal(P.normals(seed, offset, short), z[:short])
    # element order: quad q holds z0..z3 of counter offset + q
    zq, rq = P.normals(seed, offset + 5, 4, with_radius=True)
    assert np.array_equal(zq, z[20:24])
    assert rq[0] == rq[1] and rq[2] == rq[3] and math.isclose(zq[0] ** 2 + zq[1] ** 2, rq[0] ** 2, rel_tol=1e-12)


def test_box_muller_matches_the_words():
    """the transform of one quad, spelled out from its four words"""
    seed, ctr = 99, 2**32 + 3
    x = P.philox4x32_10(seed, [ctr])[0]
    u = [((int(w) >> 8) + 1) / 2.0**24 for w in x]
    want = []
    for ur, ua in ((u[0], u[1]), (u[2], u[3])):
        r = math.sqrt(-2.0 * math.log(ur))
        a = float(np.float32(np.float32(2 * math.pi) * np.float32(ua)))
        want += [r * math.cos(a), r * math.sin(a)]
    assert np.array_equal(P.normals(seed, ctr, 4), np.array(want))


def _corr(a, b):
    a = a - a.mean()
    b = b - b.mean()
    return float(a @ b / math.sqrt((a @ a) * (b @ b)))


@pytest.mark.parametrize("seed,offset", BATTERY)
def test_normal_statistics(seed, offset):
    """moments, Kolmogorov-Smirnov distance to Phi, tail counts, the structural maximum and cross-correlations of 2^22 normals;
    every bound is 5 sigma of the statistic's sampling distribution (KS: 1.95 / sqrt(N), the 0.1 % point)"""
    N = N_BATTERY
    z = P.normals(seed, offset, N)
    mean = z.mean()
    d = z - mean
    m2, m3, m4 = (d**2).mean(), (d**3).mean(), (d**4).mean()
    assert abs(mean) <= 5 / math.sqrt(N), mean
    assert abs(m2 - 1) <= 5 * math.sqrt(2 / N), m2
    assert abs(m3 / m2**1.5) <= 5 * math.sqrt(6 / N), m3 / m2**1.5
    assert abs(m4 / m2**2 - 3) <= 5 * math.sqrt(24 / N), m4 / m2**2 - 3

    zs = torch.from_numpy(np.sort(z))
    cdf = torch.special.ndtr(zs).numpy()
    i = np.arange(1, N + 1, dtype=np.float64)
    ks = max((i / N - cdf).max(), (cdf - (i - 1) / N).max())
    assert ks <= 1.95 / math.sqrt(N), ks

    for k in (3.0, 4.0):
        p = math.erfc(k / math.sqrt(2))
        count = int((np.abs(z) > k).sum())
        assert abs(count - N * p) <= 5 * math.sqrt(N * p * (1 - p)), (k, count, N * p)
    assert np.abs(z).max() <= P.MAX_ABS_Z

    q = z.reshape(-1, 4)
    pairs = {
        "z0 with z1 (shared radius)": (q[:, 0::2].ravel(), q[:, 1::2].ravel()),
        "z0^2 with z1^2": (q[:, 0::2].ravel() ** 2, q[:, 1::2].ravel() ** 2),
        "z0 with z2 (same counter)": (q[:, 0:2].ravel(), q[:, 2:4].ravel()),
        "lag one quad": (z[:-4], z[4:]),
        "seed + 1": (z, P.normals(seed + 1, offset, N)),
        "the dropout key's stream": (z, P.normals(seed ^ P.DROPOUT_KEY_XOR, offset, N)),
    }
    for name, (a, b) in pairs.items():
        rho = _corr(a, b)
        assert abs(rho) <= 5 / math.sqrt(a.size), (name, rho)


def test_dropout_drop_rate():
    """p = 0.1 in fp32: the count of drops in 2^24 draws sits within 5 sigma of N floor(p 2^24) / 2^24"""
    N, p = 2**24, 0.1
    m = P.dropout_masks(P.HALF_KEY, 2**32 + 12345, N, p)
    q = math.floor(float(np.float32(p)) * 2**24) / 2**24
    drops = int((m == 0).sum())
    assert abs(drops - N * q) <= 5 * math.sqrt(N * q * (1 - q)), (drops, N * q)
    keep = np.float32(1) / (np.float32(1) - np.float32(p))
    assert set(np.unique(m).tolist()) == {0.0, float(keep)}


def test_a_uniform_equal_to_p_is_dropped():
    """u <= p, not u < p: the word at P.HALF_CTR has u == 0.5 exactly, and p = 0.5 drops it"""
    u = P.uniforms(P.HALF_KEY, P.HALF_CTR, 4)
    assert u[P.HALF_WORD] == 0.5
    m = P.dropout_masks(P.HALF_KEY, P.HALF_CTR, 4, 0.5)
    assert m[P.HALF_WORD] == 0.0
    assert all(m[j] == (0.0 if u[j] <= 0.5 else 2.0) for j in range(4))


def test_rank_keys_do_not_collide():
    """every rank's noise key and dropout key (key ^ 0x5DEECE66D) are distinct over a set of base seeds and 64 ranks"""
    from dmme_amd import distributed

    keys = []
    for s in (0, 1, 42, 1337, 2**31 - 1, 2**32 + 5):
        for r in range(64):
            k = distributed.rank_seed(s, r)
            keys += [k, k ^ P.DROPOUT_KEY_XOR]
    assert len(set(keys)) == len(keys)
