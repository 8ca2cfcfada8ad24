"""The multi-scalar multiplication against prepared bases on the CPU: the signed recoding, the window step of a table build, level 0 of the
accumulation over the records and the whole route, each run by the host simulation (tests/hostsim/hostsim_msm_prepared.cpp: the bodies of
bn_amd/csrc/group_ops.hpp over host arrays, G2 on simulated lane pairs) with every limb / value bound enforced, against the oracle."""
import ctypes as C

import numpy as np
import pytest

import bn_model as M
import hostsim_msm_prepared_lib as L
from bn_oracle import FR
from conftest import canon_infinity
from test_hostsim_group_ops import Group

R = M.R_ORD
GROUPS = (1, 2)
NEG = 1 << 31
p32 = L.p32


@pytest.fixture(scope="module")
def hs():
    return L.lib()


@pytest.fixture(scope="module")
def groups(oracle):
    return {g: Group(oracle, g) for g in GROUPS}


@pytest.fixture(scope="module")
def points(groups):
    """{g: 8 distinct finite points with z != 1}, computed once"""
    rng = np.random.default_rng(2901)
    out = {}
    for g, G in groups.items():
        P = np.stack([G.times(G.one(), int.from_bytes(rng.bytes(40), "little")) for _ in range(8)])
        assert not np.array_equal(P[0, 8 * g:], G.one()[8 * g:])                                 # really z != 1
        out[g] = np.ascontiguousarray(P)
    return out


# ---------------------------------------------------------------------------------------------------------------- signed recoding
def _model(k, c):
    """signed digits in [-2^(c-1), 2^(c-1)], low window first: v > 2^(c-1) carries"""
    W, half, carry, out = L.windows(c), 1 << (c - 1), 0, []
    for w in range(W):
        v = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if v > half else 0
        out.append(v - (1 << c) if carry else v)
    return out, carry


def _crafted(c):
    W, half = L.windows(c), 1 << (c - 1)
    below_r = lambda d: sum(d << (c * w) for w in range(W)) & ((1 << 253) - 1)                    # every digit d, cut below 2^253 < r
    return [0, 1, R - 1, 1 << 253, below_r(half), below_r(half + 1), (1 << (c * (W - 1))) - 1]


@pytest.mark.parametrize("c", (3, 5, 8, 13, 16))
def test_signed_recoding(c):
    """0, 1, r - 1, 2^253, every digit exactly 2^(c-1) (the edge that does NOT carry), every digit 2^(c-1) + 1 (a run of carries), every
    window but the top one full - and a few random scalars: the device's digits are the model's, the model reconstructs k, every |d| is at
    most 2^(c-1) and the top window leaves no carry"""
    rng = np.random.default_rng(c)
    half = 1 << (c - 1)
    for k in _crafted(c) + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(8)]:
        assert 0 <= k < R
        want, carry = _model(k, c)
        assert carry == 0 and sum(d << (c * w) for w, d in enumerate(want)) == k and all(abs(d) <= half for d in want), hex(k)
        got, got_carry = L.signed_digits(k, c)
        assert got_carry == 0
        assert [(-m if neg else m) for m, neg in got] == want, hex(k)
        # (a window of 2^c - 1 under a carry is the digit zero WITH the sign flag - v = 2^c carries on -: nothing is entered for it)
    k = _crafted(c)[4]
    assert all(d == half for d in _model(k, c)[0][:-1])                                           # exactly 2^(c-1): kept, no carry
    k = _crafted(c)[5]
    assert _model(k, c)[0][0] == half + 1 - (1 << c) and _model(k, c)[0][1] == half + 2 - (1 << c)


# ---------------------------------------------------------------------------------------------------------------- the table
def _records(G, q, flag=None):
    """the g records (20 words each) of the normalised point q"""
    g = G.g
    rec = np.zeros((g, 20), np.uint32)
    inf = not q[8 * g:].any() if flag is None else flag
    for comp in range(g):
        x, y = np.ascontiguousarray(q[4 * comp:4 * comp + 4]), np.ascontiguousarray(q[4 * g + 4 * comp:4 * g + 4 * comp + 4])
        L.lib().hsp_record(p32(x), p32(y), 1 if inf else 0, p32(rec), comp)
    return rec


@pytest.mark.parametrize("g", GROUPS)
def test_window_step_and_table_of_one_point(hs, groups, points, g):
    """c = 13, W = 20: msm_prep_double_body takes 2^(13 w) P to 2^(13 (w + 1)) P, and the build (normalise, repack, double) gives the
    records of normalize(2^(13 w) P) for every window - for a finite point with z != 1 and, beside it, a point at infinity with stale x, y
    (flagged records in every window); the kept points are the normalised inputs"""
    G, c = groups[g], 13
    W = L.windows(c)
    P = points[g][0]
    run = np.ascontiguousarray(np.stack([P, P]))
    hs.hsp_double(g, p32(run), 2, c)
    assert G.same(run[0], G.times(P, 1 << c)) and np.array_equal(run[0], run[1])
    stale = P.copy(); stale[8 * g:] = 0                                                           # z == 0, x and y whatever
    src = np.ascontiguousarray(np.stack([P, stale]))
    table = np.full((W, 2, g, 20), 0xffffffff, np.uint32)
    kept = np.zeros_like(src)
    hs.hsp_table(g, p32(src), 2, c, p32(table), p32(kept))
    assert np.array_equal(kept[0], G.normalize(P)) and np.array_equal(kept[1], G.zero())
    for w in range(W):
        q = G.normalize(G.times(P, 1 << (c * w)))
        assert q[8 * g:].any()
        assert np.array_equal(table[w, 0], _records(G, q)), w
        assert (table[w, 1, :, 18] != 0).all() and (table[w, 1, :, 19] == 0).all(), w


# ---------------------------------------------------------------------------------------------------------------- level 0
def _table_of(G, pts):
    """records of the normalised points, then one flagged record (index len(pts)) whose x, y are those of pts[0]"""
    recs = [_records(G, G.normalize(p)) for p in pts] + [_records(G, G.normalize(pts[0]), flag=True)]
    return np.ascontiguousarray(np.stack(recs))


def _accumulate(hs, G, table, entries, nkeys, buckets=None):
    """entries: (table index, negative, key) in key order -> (buckets, levels)"""
    idx = np.array([e[0] | (NEG if e[1] else 0) for e in entries] + [0xdeadbeef], np.uint32)
    keys = np.array([e[2] for e in entries] + [0x7fffffff], np.uint32)
    if buckets is None:
        buckets = np.zeros((nkeys, G.w), np.uint64)                                               # z = 0: every bucket starts at infinity
    levels = C.c_uint32(0)
    hs.hsp_acc(G.g, p32(table), p32(idx), p32(keys), len(entries), p32(buckets), C.byref(levels))
    return buckets, levels.value


def _check_buckets(G, pts, chunks, buckets):
    flagged = len(pts)
    for key in range(len(buckets)):
        terms = [G.neg(pts[i]) if neg else pts[i] for entries in chunks for i, neg, k in entries if k == key and i != flagged]
        assert G.same(buckets[key], G.sum(terms)), key


@pytest.mark.parametrize("g", GROUPS)
def test_level_zero_over_records(hs, groups, points, g):
    """MSM_PIECE = 16 entries per lane.  Entry counts 1, 16, 17 and 33 with random keys, signs and records, flagged records among them;
    one key over all 33 entries (slot 2i and the MSM_SKIP marker in the middle lane; the levels above are msm_acc_body) and over 257 (three
    levels); the same record twice in a bucket (the doubling branch of the mixed addition), three times, P with -P (an accumulator back
    at infinity, then a further entry), only flagged records; a run that crosses a lane seam; a second chunk into the same buckets"""
    assert hs.hsp_piece() == 16
    G, P = groups[g], points[g]
    table = _table_of(G, P)
    flagged = len(P)
    rng = np.random.default_rng(50 + g)
    entry = lambda k: (int(rng.integers(0, len(P) + 1)), bool(rng.integers(0, 2)), k)
    for n, want_levels in ((1, 1), (16, 1), (17, 2), (33, 2)):
        entries = [entry(k) for k in sorted(int(k) for k in rng.integers(0, 6, n))]
        buckets, levels = _accumulate(hs, G, table, entries, 6)
        assert levels == want_levels
        _check_buckets(G, P, [entries], buckets)
    for n, want_levels in ((33, 2), (257, 3)):
        entries = [entry(3) for _ in range(n)]
        assert any(e[1] for e in entries) and any(e[0] == flagged for e in entries)
        buckets, levels = _accumulate(hs, G, table, entries, 4)
        assert levels == want_levels
        _check_buckets(G, P, [entries], buckets)
    crafted = ([(0, False, 0)] * 2 + [(1, True, 1)] * 3 + [(2, False, 2), (2, True, 2)] + [(3, False, 3), (3, True, 3), (4, False, 3)] +
               [(flagged, False, 4), (flagged, True, 4)] + [(5, True, 5), (flagged, False, 5), (5, True, 5)] +
               [(6, False, 6)] * 2 + [(7, False, 7)] * 4)                                         # bucket 6 .. 7: entries 14 .. 19 cross the seam at 16
    assert len(crafted) == 21 and [e[2] for e in crafted] == sorted(e[2] for e in crafted)
    buckets, _ = _accumulate(hs, G, table, crafted, 9)
    _check_buckets(G, P, [crafted], buckets)
    assert G.same(buckets[0], G.times(P[0], 2)) and G.same(buckets[1], G.times(G.neg(P[1]), 3))
    for empty in (2, 4, 8):
        assert not buckets[empty][8 * g:].any(), empty                                            # cancelled, only flagged records, never named
    second = [entry(k) for k in sorted(int(k) for k in rng.integers(0, 9, 20))]
    buckets, _ = _accumulate(hs, G, table, second, 9, buckets)
    _check_buckets(G, P, [crafted, second], buckets)


# ---------------------------------------------------------------------------------------------------------------- the whole route
@pytest.mark.parametrize("chunk", (40, 16))
@pytest.mark.parametrize("g", GROUPS)
def test_whole_route_on_40_terms(hs, oracle, groups, points, g, chunk):
    """c = 5 (W = 51 windows, 16 buckets, one reduction lane): a handle of 43 points - raw, z != 1, repeated points, a point at infinity -
    built by the simulated table build, 40 scalars (random, and the crafted ones of the recoding test) against points [3, 43), in one
    chunk and in chunks of 16; the tail - the reduction's 2 terms times the host's tail scalars - is folded by the oracle and compared
    with the oracle fold of the terms"""
    G, c, count, first, n = groups[g], 5, 43, 3, 40
    rng = np.random.default_rng(77 + g)
    pts = points[g][rng.integers(0, 8, count)].copy()
    pts[first + 7, 8 * g:] = 0                                                                    # a point at infinity in the range
    pts = np.ascontiguousarray(pts)
    W = L.windows(c)
    table = np.zeros((W, count, g, 20), np.uint32)
    kept = np.zeros_like(pts)
    hs.hsp_table(g, p32(pts), count, c, p32(table), p32(kept))
    ks = _crafted(c) + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n - 7)]
    ks[9] = ks[8]; pts_same = np.array_equal(pts[first + 8], pts[first + 9])                      # equal scalars side by side
    K = np.ascontiguousarray(np.stack([oracle.fp_from_int(FR, k) for k in ks]))
    p = L.plan(c, chunk, 96 * g)
    assert (p["K"], p["G"], p["groups"]) == (16, 16, 1)
    buckets = np.zeros((p["K"], G.w), np.uint64)
    terms = np.zeros((2 * p["count"], G.w), np.uint64)
    hs.hsp_route(g, p32(table), count, first, p32(K), n, c, chunk, p32(buckets), p32(terms))
    scal = L.tail_scalars(c)
    mont = pow(1 << 256, -1, R)
    tail = [G.times(t, sum(int(x) << (64 * i) for i, x in enumerate(s)) * mont % R) for t, s in zip(terms, scal)]
    got = G.normalize(G.sum(tail))
    want = G.normalize(G.sum([G.times(pts[first + i], k) for i, k in enumerate(ks)]))
    assert want[8 * g:].any()
    assert np.array_equal(canon_infinity(got), canon_infinity(want)), pts_same
    # every bucket is what the signed digits say: sum over (term, window) of +- 2^(5 w) P_i with |d| - 1 == bucket
    digits = [_model(k, c)[0] for k in ks]
    for b in (0, 7, 15):
        members = [G.times(pts[first + i], ((1 << (c * w)) if d > 0 else R - (1 << (c * w))) % R) for i, ds in enumerate(digits) for w, d in enumerate(ds) if abs(d) == b + 1]
        assert G.same(buckets[b], G.sum(members)), b
