"""The per-lane bodies of the group kernels (bn_amd/csrc/group_ops.hpp) on the CPU: the segmented fold, the accumulation levels and the
reduction of the bucket method, the fixed-base chain and the 80-byte table record, each run by the host simulation over host arrays (G2 on
simulated lane pairs) with every limb / value bound enforced, against the oracle.  The shapes are the smallest that reach each branch."""
import ctypes as C

import numpy as np
import pytest

import bn_model as M
import hostsim_lib
from bn_oracle import FR
from conftest import canon_infinity

R = M.R_ORD
U32 = C.POINTER(C.c_uint32)
GROUPS = (1, 2)


@pytest.fixture(scope="module")
def hs():
    return hostsim_lib.HostSim(bounds=True)


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(U32)


class Group:
    """the oracle's side of one group: points are rows of 12 (G1) / 24 (G2) uint64"""
    def __init__(self, oracle, g):
        self.g, self.o, self.w = g, oracle, 12 * g
        for name in ("one", "zero", "add", "mul", "neg", "normalize", "eq"):
            setattr(self, name, getattr(oracle, f"g{g}_{name}"))

    def times(self, p, k):
        return self.mul(p, self.o.fp_from_int(FR, k % R))

    def sum(self, pts):
        acc = self.zero()
        for p in pts:
            acc = self.add(acc, p)
        return acc

    def same(self, a, b):
        return self.eq(np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64))


@pytest.fixture(scope="module")
def groups(oracle):
    return {g: Group(oracle, g) for g in GROUPS}


@pytest.fixture(scope="module")
def points(groups):
    """{g: 8 distinct finite points with z != 1}, computed once"""
    rng = np.random.default_rng(1207)
    return {g: np.stack([G.times(G.one(), int.from_bytes(rng.bytes(40), "little")) for _ in range(8)]) for g, G in groups.items()}


@pytest.mark.parametrize("g", GROUPS)
def test_segmented_fold(hs, groups, points, g):
    """pieces of 0, 1 and 4 points, two equal points (the doubling branch), P, -P, Q (an accumulator at infinity as the left operand),
    each as an inner piece (raw Jacobian sum) and as the last one of its segment (normalised)"""
    G, P = groups[g], points[g]
    shapes = [[], [P[0]], [P[1], P[2], P[3], P[4]], [P[5], P[5]], [P[6], G.neg(P[6]), P[7]], [P[2], G.neg(P[2])]]
    src = np.ascontiguousarray(np.stack([p for s in shapes for p in s]), np.uint64)
    pieces, off = [], 0
    for last in (0, 1):
        off = 0
        for s in shapes:
            pieces.append((off, len(s), last)); off += len(s)
    pc = np.array(pieces, np.uint32)
    out = np.zeros((len(pieces), G.w), np.uint64)
    hs.lib.hs_msm_fold(g, _p(src), _p(pc), len(pieces), _p(out))
    for (o, cnt, last), got in zip(pieces, out):
        want = G.zero() if cnt == 0 else src[o]
        for q in src[o + 1:o + cnt]:
            want = G.add(want, q)                                      # the serial chain, in index order
        if last:
            want = G.normalize(want)
        assert np.array_equal(canon_infinity(got), canon_infinity(want)), (o, cnt, last)


def _accumulate(hs, G, pts, entries, nkeys, buckets=None):
    """entries: (term index, key) in key order -> the buckets after every level"""
    idx = np.array([e[0] for e in entries], np.uint32)
    keys = np.array([e[1] for e in entries], np.uint32)
    if buckets is None:
        buckets = np.zeros((nkeys, G.w), np.uint64)                   # z = 0: every bucket starts at infinity
    levels = C.c_uint32(0)
    hs.lib.hs_msm_acc(G.g, _p(pts), _p(idx), _p(keys), len(entries), _p(buckets), C.byref(levels))
    return buckets, levels.value


def _check_buckets(G, pts, chunks, buckets):
    for key in range(len(buckets)):
        want = G.sum([pts[i] for entries in chunks for i, k in entries if k == key])
        assert G.same(buckets[key], want), key


@pytest.mark.parametrize("g", GROUPS)
def test_bucket_accumulation_levels(hs, groups, points, g):
    """MSM_PIECE = 16 entries per lane.  Entry counts 1, 16, 17 and 33; one key over all 33 entries (its run began earlier AND goes on in
    the middle lane: slot 2i and the MSM_SKIP marker) and over 257 (three levels); a run that starts inside a lane and continues into the
    next; a lane whose entries are 16 different keys; a short last lane; the points gathered through idx at level 0 (repeated indices: equal
    points meet in a bucket) and taken in place above; a second chunk adds into the buckets of the first"""
    assert hs.lib.hs_msm_piece() == 16
    G, P = groups[g], np.ascontiguousarray(points[g])
    rng = np.random.default_rng(5)
    term = lambda: int(rng.integers(0, len(P)))
    for n, want_levels in ((1, 1), (16, 1), (17, 2), (33, 2)):
        keys = sorted(int(k) for k in rng.integers(1, 6, n))
        entries = [(term(), k) for k in keys]
        buckets, levels = _accumulate(hs, G, P, entries, 6)
        assert levels == want_levels
        _check_buckets(G, P, [entries], buckets)
    for n, want_levels in ((33, 2), (257, 3)):
        entries = [(term(), 3) for _ in range(n)]
        buckets, levels = _accumulate(hs, G, P, entries, 4)
        assert levels == want_levels
        _check_buckets(G, P, [entries], buckets)
    keys = [1] * 3 + [2] * 2 + [3] * 5 + [4] * 6 + [4] * 4 + list(range(5, 17)) + list(range(20, 36)) + [36] * 2
    assert len(keys) == 50 and keys[10:20] == [4] * 10 and len(set(keys[32:48])) == 16
    first = [(term(), k) for k in keys]
    buckets, _ = _accumulate(hs, G, P, first, 40)
    _check_buckets(G, P, [first], buckets)
    second = [(term(), k) for k in sorted(int(k) for k in rng.integers(1, 40, 20))]
    buckets, _ = _accumulate(hs, G, P, second, 40, buckets)
    _check_buckets(G, P, [first, second], buckets)


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("ngroups", (1, 2))
def test_bucket_reduction(hs, groups, points, g, ngroups):
    """G = 16 buckets per lane, two windows of 16 * ngroups buckets, some of them at infinity: S = sum B_b and T = sum (b - base) B_b"""
    G, P = groups[g], points[g]
    Gn, W, log2b = 16, 2, 4 + (ngroups - 1)
    rng = np.random.default_rng(11)
    buckets = np.zeros((W << log2b, G.w), np.uint64)
    for b in range(len(buckets)):
        if rng.integers(0, 4):                                        # one in four stays at infinity (z = 0)
            buckets[b] = P[int(rng.integers(0, len(P)))]
    buckets[5] = G.zero()                                             # infinity as the reference writes it
    count = W * ngroups
    terms = np.zeros((2 * count, G.w), np.uint64)
    hs.lib.hs_msm_reduce(g, _p(buckets), Gn, ngroups, log2b, count, _p(terms))
    for t in range(count):
        base = ((t // ngroups) << log2b) + (t % ngroups) * Gn
        assert G.same(terms[t], G.sum(buckets[base:base + Gn])), t
        assert G.same(terms[count + t], G.sum([G.times(buckets[base + b], b) for b in range(Gn)])), t


def _recode(k, c):
    """the signed digits of group_ops.hpp base_mul_body: (window, |digit|) of every non-zero digit"""
    W, half, carry, out = (254 + c - 1) // c, 1 << (c - 1), 0, []
    for w in range(W):
        v = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if v > half else 0
        ad = (1 << c) - v if carry else v
        if ad:
            out.append((w, ad))
    assert carry == 0
    return out


def _edge_scalars(c):
    """tests/test_gpu_mul_base.py::_edge_values without its sweep over every bit position"""
    W = (254 + c - 1) // c
    vals = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
    for d in ((1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1):          # a digit exactly 2^(c-1), runs of carries
        vals.append(sum(d << (c * w) for w in range(W)) & ((1 << 253) - 1))
    vals.append(1 << (c - 1))
    for cc in (8, 10, 12):                                                                   # the top window wraps mod r: a doubling
        vals.append(R - 2 * (R % (1 << (cc * ((254 + cc - 1) // cc - 1)))))
    rng = np.random.default_rng(2024)
    return vals + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(4)]


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("c", (8, 10, 12))
def test_fixed_base_chain(hs, oracle, groups, points, g, c):
    """widths 8, 10 and 12 over a table whose entries d 2^(c w) B the oracle computed (only those the scalars' digits name; any other
    record is zero, so a wrong index cannot pass), and over the table of a base at infinity (every record flagged)"""
    G, B = groups[g], points[g][0]
    W, half = (254 + c - 1) // c, 1 << (c - 1)
    vals = _edge_scalars(c)
    table = np.zeros((W * half * g, 20), np.uint32)
    flagged = np.zeros_like(table)
    zero4 = np.zeros(4, np.uint64)
    for w, d in sorted({e for k in vals for e in _recode(k, c)}):
        e = w * half + d - 1
        q = G.normalize(G.times(B, d << (c * w)))
        assert q[2 * 4 * g:].any()
        for comp in range(g):                                         # G2: component c0 of (x, y) in record 2e, c1 in record 2e + 1
            x, y = q[4 * comp:4 * comp + 4], q[4 * g + 4 * comp:4 * g + 4 * comp + 4]
            hs.lib.hs_base_record(_p(np.ascontiguousarray(x)), _p(np.ascontiguousarray(y)), 0, _p(table), e * g + comp)
            hs.lib.hs_base_record(_p(zero4), _p(zero4), 1, _p(flagged), e * g + comp)
    K = np.stack([oracle.fp_from_int(FR, k) for k in vals])
    out = np.zeros((len(vals), G.w), np.uint64)
    hs.lib.hs_mul_base(g, _p(table), c, _p(K), len(vals), _p(out))
    for k, got in zip(vals, out):
        assert np.array_equal(canon_infinity(got), canon_infinity(G.normalize(G.times(B, k)))), hex(k)
    hs.lib.hs_mul_base(g, _p(flagged), c, _p(K), len(vals), _p(out))
    assert np.array_equal(canon_infinity(out), canon_infinity(np.stack([G.zero()] * len(vals))))


def test_table_record_round_trip(hs):
    """18 limbs and the flag word through the five 16-byte groups and back; the record is the limbs in order, word 18 the flag, word 19 zero"""
    rng = np.random.default_rng(3)
    for flag in (0, 1, 0xdeadbeef):
        limbs = rng.integers(0, 1 << 29, 18).astype(np.uint32)
        limbs[8] = limbs[17] = 1 << 20                                # below q: what a record holds is a product
        rec = np.full(20, 0xffffffff, np.uint32)
        out = np.zeros(19, np.uint32)
        hs.lib.hs_aff_record_roundtrip(_p(limbs), C.c_uint32(flag), _p(rec), _p(out))
        assert np.array_equal(rec[:18], limbs) and rec[18] == flag and rec[19] == 0
        assert np.array_equal(out[:18], limbs) and out[18] == flag


def test_scalar_digits(hs):
    """msm_digit: the c-bit digit of every window, across word boundaries"""
    rng = np.random.default_rng(8)
    for k in (R - 1, int.from_bytes(rng.bytes(31), "little")):
        raw = np.frombuffer(k.to_bytes(32, "little"), np.uint32).copy()
        for c in (3, 8, 10, 12, 13, 16):
            for w in range((254 + c - 1) // c):
                assert hs.lib.hs_msm_digit(_p(raw), w, c) == (k >> (c * w)) & ((1 << c) - 1), (c, w)
