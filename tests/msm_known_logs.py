"""TEST INFRASTRUCTURE - an expectation for LARGE multi-scalar multiplications that shares no code with the MSM routes (CPU:
tests/test_msm_known_logs.py, GPU: tests/test_gpu_msm_default_route.py).

For points with known logarithms, P_i = [a_i] G, the sum is one scalar multiplication: sum_i [k_i] P_i = [sum_i a_i k_i mod r] G.  The
left side is the call under test; the right side is a sum of Python integers and ONE multiplication by the oracle, normalised - exact bytes,
since every MSM output is normalised.  Logs and scalars are drawn on the host as canonical integers below 2^253 < r: (n, 4) uint64 words,
least significant first, the top word masked to 61 bits.  The library receives them as Montgomery rows through its own wire decoder
(Engine.fr_decode_batch of the 32-byte big-endian records wire() makes); the host sum reads the same words.

Special terms are spliced in at fixed positions.  A cluster of eight terms at every index a call may start from (Logs.starts), s = the start:
    s + 0   k = r - 1                                 s + 1   a = 0: the point at infinity as the device's own chain leaves it
    s + 2, s + 3   the same a: one point twice        s + 4, s + 5   a and r - a under ONE k: P and -P meet in every bucket
    s + 6   k = 0                                     s + 7   k = 1
the last three terms of a call carry k = 1, 0, r - 1 (the last index: r - 1), and at every seam t of Logs.seams - the first index of a
call's second chunk - a[t] = r - a[t - 1] and k[t] = k[t - 1]: P goes into the buckets in one pass and -P in the next."""
import operator

import numpy as np

import bn_model as M
from bn_oracle import FR
from conftest import canon_infinity

R = M.R_ORD
CHUNK = 1 << 20                                        # the default BN254_OPT_MSM_CHUNK
CLUSTER = 8
_M64 = (1 << 64) - 1


def draw(rng, n):
    """n canonical integers below 2^253 as (n, 4) uint64 words"""
    w = np.frombuffer(rng.bytes(32 * n), np.uint64).reshape(n, 4).copy()
    w[:, 3] &= np.uint64((1 << 61) - 1)
    return w


def to_words(values):
    return np.array([[(v >> (64 * j)) & _M64 for j in range(4)] for v in values], np.uint64).reshape(-1, 4)


def to_ints(words):
    b = np.ascontiguousarray(words, "<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def wire(words):
    """(n, 4) words -> (n, 32) uint8: the big-endian canonical records of BN254_FR_WIRE_BYTES"""
    return np.ascontiguousarray(words[:, ::-1]).astype(">u8").view(np.uint8).reshape(-1, 32)


def _neg(row):
    return to_words([R - to_ints(row[None])[0]])[0]


class Logs:
    """the logarithms a_i of a point set: .words (n, 4), .ints, the call starts and chunk seams the special terms were placed for"""

    def __init__(self, rng, n, starts=(0,), seams=()):
        a = draw(rng, n)
        for s in starts:
            assert s + CLUSTER <= n
            a[s + 1] = 0
            a[s + 3] = a[s + 2]
            a[s + 5] = _neg(a[s + 4])
        for t in seams:
            assert 0 < t < n and all(not (s <= t - 1 < s + CLUSTER or s <= t < s + CLUSTER) for s in starts)
            a[t] = _neg(a[t - 1])
        self.words, self.ints, self.starts, self.seams = a, to_ints(a), tuple(starts), tuple(seams)
        assert all(0 < v < R for i, v in enumerate(self.ints) if i - 1 not in starts)


def draw_scalars(rng, logs, lo, n, chunk=CHUNK):
    """(k, special): the scalars of the call over terms [lo, lo + n) of `logs` as (n, 4) words, and the indices (relative to lo) of its special terms"""
    assert lo in logs.starts and n >= CLUSTER + 3
    k = draw(rng, n)
    k[0], k[6], k[7] = to_words([R - 1, 0, 1])
    k[n - 3], k[n - 2], k[n - 1] = to_words([1, 0, R - 1])
    k[5] = k[4]
    special = list(range(CLUSTER)) + [n - 3, n - 2, n - 1]
    for t in logs.seams:
        if lo < t < lo + n:
            assert t - lo == chunk and t - lo + 1 < n - 3          # the seam of THIS call, clear of the last three terms
            k[t - lo] = k[t - lo - 1]
            special += [t - lo - 1, t - lo]
    assert n <= chunk or {chunk - 1, chunk} <= set(special)
    assert {0, n - 1} <= set(special)
    return k, sorted(special)


def host_sum(logs, lo, k):
    """sum a_i k_i mod r over terms [lo, lo + len(k)) in Python integers"""
    return sum(map(operator.mul, logs.ints[lo:lo + len(k)], to_ints(k))) % R


def expected(oracle, g, s):
    """normalize([s] G) by the oracle, the point at infinity as G::zero()"""
    one, mul, norm = (oracle.g1_one, oracle.g1_mul, oracle.g1_normalize) if g == 1 else (oracle.g2_one, oracle.g2_mul, oracle.g2_normalize)
    return canon_infinity(norm(mul(one(), oracle.fp_from_int(FR, s % R)))[None])[0]


def montgomery(eng, words):
    """(n, 4) canonical words -> (n, 4) Montgomery rows by the library's wire decoder; every record must be accepted"""
    rows, st = eng.fr_decode_batch(wire(words))
    assert not st.any()
    return rows
