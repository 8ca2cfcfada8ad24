"""CPU tests of the host planners (bn_amd/csrc/host_plan.hpp, exported by tests/hostsim/hostsim.cpp): the work lists of the segmented folds
are replayed symbolically, the cutting of a prepared batch into Miller pieces and the workspace of the bucket method are checked against
their rules.  No GPU: the planners are host arithmetic over sizes and offsets."""
import ctypes as C
import random

import numpy as np
import pytest

import hostsim_lib

P61 = (1 << 61) - 1
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b97091_43e1f593f0000001
SEGMENTS = {"ragged": [0, 1, 17, 300, 0, 65, 64, 5, 0], "all_empty": [0, 0, 0], "one_long": None}      # one_long: one segment of 4 * chunk + 1
_U64P, _SZP = C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)


@pytest.fixture(scope="module")
def lib():
    l = hostsim_lib.HostSim(bounds=True).lib
    for f in (l.hs_seg_partials_max, l.hs_seg_tail_max, l.hs_msm_tail_scalars):
        f.restype = C.c_size_t
    return l


def _u64(n):
    return np.zeros(max(n, 1), np.uint64)


def _ptr(a, t=_U64P):
    return a.ctypes.data_as(t)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def seg_plan(lib, off, chunk, small, V, fold, snap):
    m, cap = len(off) - 1, 4 * (int(off[-1]) + len(off)) + 64
    pieces, launches, chunks, counts = _u64(5 * cap), _u64(4 * cap), _u64(3 * cap), _u64(4)
    ok = lib.hs_seg_plan(_ptr(off, _SZP), C.c_size_t(m), C.c_size_t(chunk), int(small), C.c_size_t(V), C.c_size_t(fold), int(snap), _ptr(pieces), _ptr(launches), _ptr(chunks),
                         C.c_size_t(cap), _ptr(counts))
    assert ok == 1, counts
    assert counts[3] == 1, "seg_plan returned false"
    n = [int(x) for x in counts[:3]]
    return pieces[:5 * n[0]].reshape(-1, 5).tolist(), launches[:4 * n[1]].reshape(-1, 4).tolist(), chunks[:3 * n[2]].reshape(-1, 3).tolist()


def _levels(L, fold, cap):
    """fold launches a run of L values needs before at most `cap` are left"""
    k = 0
    while L > cap:
        L = -(-L // fold); k += 1
    return k


@pytest.mark.parametrize("fold,snap,small,V", [(16, True, False, 384), (16, True, True, 384), (4, False, False, 96)])
@pytest.mark.parametrize("chunk", [8, 64])
@pytest.mark.parametrize("shape", sorted(SEGMENTS))
def test_segmented_plan_replayed_symbolically(lib, shape, chunk, fold, snap, small, V):
    lengths = SEGMENTS[shape] or [4 * chunk + 1]
    off = _offsets(lengths)
    m, n = len(lengths), int(off[-1])
    rng = random.Random(chunk * 1000 + fold)
    w = [rng.getrandbits(61) % P61 for _ in range(n)]
    pieces, launches, chunks = seg_plan(lib, off, chunk, small, V, fold, snap)
    pb, tail_max = lib.hs_seg_partials_max(C.c_size_t(chunk), C.c_size_t(fold)), lib.hs_seg_tail_max()
    first_partial, carry_slot = chunk + 1, chunk + 1 + pb
    out, carried, j = {}, None, 0                    # j: the first segment the next chunk works on
    covered = 0
    assert sum(l[3] for l in launches) == len(pieces)
    for ci, (lo, hi, carry_out) in enumerate(chunks):
        assert lo == covered and lo <= hi <= min(n, lo + chunk) and (hi > lo or n == 0)
        if not snap and hi < n:
            assert hi - lo == chunk                  # fixed cuts: every chunk but the last is full
        covered = hi
        slots = {1 + i: w[lo + i] for i in range(hi - lo)}
        if carried is not None:
            slots[0] = carried
        # what the chunk has to do, from the offsets alone: the runs of values of its segments, the deepest run's levels
        jend = m if hi == n else next(jj for jj in range(j, m + 1) if jj == m or off[jj] >= hi)
        runs = [(min(int(off[jj + 1]), hi) - max(int(off[jj]), lo)) + (1 if carried is not None and jj == j else 0) for jj in range(j, jend)]
        last_cap = tail_max if small else fold
        want_fold = max([_levels(L, fold, last_cap) + (0 if small else 1) for L in runs], default=0)
        mine = [l for l in launches if l[0] == ci]
        assert [l[1] for l in mine] == [0] * want_fold + ([1] if small and runs else []), (ci, mine, runs)
        written_here = set()
        for _, tail, first, count in mine:
            results = []
            for src, to_out, dst, cnt, last in pieces[first:first + count]:
                assert src % V == 0 and dst % V == 0
                assert cnt <= (tail_max if tail else fold)
                a = src // V
                for k in range(a, a + cnt):
                    assert k in slots, f"chunk {ci}: slot {k} read before it was written"
                val = sum(slots[k] for k in range(a, a + cnt)) % P61
                if to_out:
                    assert last == 1 and dst // V not in out and dst // V < m
                    results.append(("out", dst // V, val))
                else:
                    d = dst // V
                    assert last == 0 and (first_partial <= d < first_partial + pb or d == carry_slot), d
                    assert d not in written_here, f"chunk {ci}: slot {d} written twice"
                    written_here.add(d)
                    results.append(("ws", d, val))
            for kind, d, val in results:             # the pieces of one launch run side by side: their results are visible to the next launch only
                if kind == "out":
                    out[d] = val
                else:
                    slots[d] = val
        assert bool(carry_out) == (carry_slot in written_here)
        carried = slots[carry_slot] if carry_out else None
        j = jend - 1 if carry_out else jend
    assert covered == n and carried is None
    assert out == {jj: sum(w[int(off[jj]):int(off[jj + 1])]) % P61 for jj in range(m)}


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("round_pairs", [8, 64])
def test_miller_pieces_cover_the_segments_in_sub_launches_inside_chunks(lib, direct, round_pairs):
    lengths = [0, 1, 4, 3, 0, 2, 4, 4, 1] * 9 if direct else SEGMENTS["ragged"]
    off = _offsets(lengths)
    m = len(lengths)
    want_voff = _offsets([-(-L // 4) for L in lengths])
    if direct:
        ranges = [(0, m)]
    else:                                            # the chunks of the fold over the derived offsets, as the prepared batch plans them
        ranges = [(lo, hi) for lo, hi, _ in seg_plan(lib, want_voff, round_pairs, False, 384, 16, True)[2]]
    cap = int(off[-1]) + m + 8
    voff, pieces, subs, counts = _u64(m + 1), _u64(2 * cap), _u64(4 * cap), _u64(2)
    cr = np.array(ranges, np.uint64).reshape(-1)
    assert lib.hs_miller_cut(_ptr(off, _SZP), C.c_size_t(m), int(direct), _ptr(cr, _SZP), C.c_size_t(len(ranges)), C.c_size_t(round_pairs), _ptr(voff), _ptr(pieces), _ptr(subs),
                             C.c_size_t(cap), _ptr(counts)) == 1
    assert np.array_equal(voff, want_voff)
    pieces = pieces[:2 * int(counts[0])].reshape(-1, 2).tolist()
    subs = subs[:4 * int(counts[1])].reshape(-1, 4).tolist()
    # the pieces each segment is cut into, from the offsets alone: (first pair, pairs), absolute
    want = []
    for a, b in zip(off[:-1].tolist(), off[1:].tolist()):
        want += [(a, b - a)] if direct else [(k, min(4, b - k)) for k in range(a, b, 4)]
    assert len(pieces) == len(want) and all(c <= 4 for _, c in want)
    seen = 0
    for ci, lo, cnt, base in subs:
        clo, chi = ranges[ci]
        assert lo == seen and clo <= lo and lo + cnt <= chi and 1 <= cnt <= -(-round_pairs // 32) * 32        # in order, inside its chunk, at most one round (in whole waves of 32 lane pairs)
        assert base == want[lo][0]
        assert [(base + f, c) for f, c in pieces[lo:lo + cnt]] == want[lo:lo + cnt]            # `first` is relative to the sub-launch
        seen = lo + cnt
    assert seen == len(want)


@pytest.mark.parametrize("chunk", [1, 64, 1 << 20])
@pytest.mark.parametrize("cb", [1, 8, 16])
@pytest.mark.parametrize("V", [96, 192])
def test_bucket_workspace_layout(lib, cb, chunk, V):
    L = 8                                            # bn254_msm_piece_M(): entries per lane and level, passed in
    head, levels = _u64(15), _u64(3 * 64)
    assert lib.hs_msm_bucket_plan(cb, C.c_size_t(chunk), C.c_size_t(V), C.c_size_t(L), _ptr(head), _ptr(levels), C.c_size_t(64)) == 1
    W, G, groups, K, count, n0max, o_counts, o_tiles, o_n0, o_idx, o_keys, o_buckets, o_terms, total, nlev = (int(x) for x in head)
    assert W == -(-254 // cb) and G == min(16, 1 << cb) and G * groups == 1 << cb and K == W << cb and count == W * groups and n0max == W * chunk
    levels = levels[:3 * nlev].reshape(-1, 3).tolist()
    want_slots, N = [], n0max
    while True:
        M = 2 * -(-N // L)
        want_slots.append(M)
        if N <= L:
            break
        N = M
    assert [l[0] for l in levels] == want_slots
    regions = [(o_counts, K * 4), (o_tiles, 4096), (o_n0, 4), (o_idx, n0max * 4), (o_keys, n0max * 4), (o_buckets, K * V)]
    for M, o_pts, o_k in levels:
        regions += [(o_pts, M * V), (o_k, M * 4)]
    regions.append((o_terms, 2 * count * V))
    at = 0
    for o, size in regions:                          # in this order, 256-byte aligned, none into the next, all inside the workspace
        assert o % 256 == 0 and o >= at
        at = o + size
    assert at <= total


@pytest.mark.parametrize("cb", [1, 8, 16])
def test_tail_scalar_table(lib, cb):
    W, G = -(-254 // cb), min(16, 1 << cb)
    groups = (1 << cb) // G
    count = W * groups
    buf = _u64(8 * count)
    assert lib.hs_msm_tail_scalars(cb, _ptr(buf), C.c_size_t(8 * count)) == 8 * count
    got = [int.from_bytes(buf[4 * i:4 * i + 4].tobytes(), "little") for i in range(2 * count)]
    mont = 1 << 256
    want_s = [(q * G << (cb * w)) * mont % R_MOD for w in range(W) for q in range(groups)]       # base * 2^(c w) for the S term of (window, group)
    want_t = [(1 << (cb * w)) * mont % R_MOD for w in range(W) for _ in range(groups)]           # 2^(c w) for its T term
    assert got == want_s + want_t


def test_window_width_by_size(lib):
    assert [lib.hs_msm_window_bits(C.c_long(-1), C.c_size_t(1 << lg)) for lg in (0, 14, 15, 17, 18, 19, 20, 24)] == [8, 8, 9, 11, 12, 11, 14, 14]
    assert lib.hs_msm_window_bits(C.c_long(5), C.c_size_t(1 << 20)) == 5
    # the sizes of tests/test_gpu_msm_default_route.py, which reads the widths it ran from this rule
    assert [lib.hs_msm_window_bits(C.c_long(-1), C.c_size_t(n)) for n in (1 << 16, (1 << 18) - 1, (1 << 19) - 1, (1 << 20) + 1000)] == [11, 11, 12, 14]
