"""The bodies of bn254_fr_dot_batch (bn_amd/csrc/dot_ops.hpp) and its planner (host_plan.hpp bn_dot_plan) on the CPU:
tests/hostsim/hostsim_dot.cpp runs the kernels' own code over host arrays along the planner's own work list, for every piece length the
sweep times and fans of 2, 4 and 16, against Python integers (tests/dot_cases.py over tests/fr_cases.py).  The simulation also checks every
piece against the arrays before its lane runs, so a plan that reads or writes outside them fails here and never on a device."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import dot_cases as DC
import fr_cases as FC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
PIECES = (4, 8, 16, 32)
FANS = (2, 4, 16)
BAD_ARG = -2
_U32P, _U64P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)


@pytest.fixture(scope="module")
def sim():
    """compiled the way hostsim_lib.py compiles its library: g++, rebuilt when a source is newer"""
    out = HERE / "libhostsim_dot.so"
    srcs = [HERE / "hostsim_dot.cpp"] + sorted(CSRC.glob("*.hpp"))
    if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_dot.cpp")])
    lib = C.CDLL(str(out))
    lib.hsd_shipped_piece.restype = C.c_uint32; lib.hsd_shipped_fan.restype = C.c_uint32
    lib.hsd_plan.restype = C.c_size_t
    lib.hsd_plan.argtypes = [_SZP, C.c_size_t, C.c_size_t, C.c_size_t, _U64P, C.c_size_t, _U64P, C.c_size_t, _SZP, _SZP]
    lib.hsd_dot.argtypes = [_U32P, _U64P, _U32P, C.c_uint64, _SZP, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _U32P, _SZP]
    lib.hsd_check.argtypes = [C.c_void_p, _U64P, C.c_int, C.c_void_p, C.c_size_t, _SZP, C.c_size_t, C.c_void_p, C.c_int]
    return lib


def _dot(sim, coeff, x, offsets, index, P, F, step=1 << 22):
    """the device form over integer lists -> ((m, 4) uint64, (product launches, fold launches))"""
    Cf, X = FC.rows(coeff), FC.rows(x)
    o = np.ascontiguousarray(offsets, np.uint64)
    m = o.size - 1
    idx = None if index is None else np.ascontiguousarray(index, np.uint64)
    out = np.full((m, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
    launches = (C.c_size_t * 2)()
    rc = sim.hsd_dot(Cf.ctypes.data_as(_U32P), None if idx is None else idx.ctypes.data_as(_U64P), X.ctypes.data_as(_U32P), len(x), o.ctypes.data_as(_SZP), m, P, F, step,
                     out.ctypes.data_as(_U32P), launches)
    assert rc == 0, rc
    return out, (launches[0], launches[1])


def _plan(sim, offsets, P, F):
    """(pieces as (first, len, to_out, dst) rows, levels as (first, count) rows, slots)"""
    o = np.ascontiguousarray(offsets, np.uint64)
    nl, slots = C.c_size_t(), C.c_size_t()
    count = sim.hsd_plan(o.ctypes.data_as(_SZP), o.size - 1, P, F, None, 0, None, 0, C.byref(nl), C.byref(slots))
    pieces = np.zeros((count, 4), np.uint64); levels = np.zeros((nl.value, 2), np.uint64)
    assert sim.hsd_plan(o.ctypes.data_as(_SZP), o.size - 1, P, F, pieces.ctypes.data_as(_U64P), count, levels.ctypes.data_as(_U64P), nl.value, C.byref(nl), C.byref(slots)) == count
    return pieces.astype(np.int64), levels.astype(np.int64), slots.value


def test_the_shipped_choices_are_covered(sim):
    assert sim.hsd_shipped_piece() in PIECES and sim.hsd_shipped_fan() in FANS


@pytest.mark.parametrize("F", FANS)
@pytest.mark.parametrize("P", PIECES)
def test_every_length_in_one_call_and_alone(sim, P, F):
    lens = DC.lengths(P, F)
    n = sum(lens)
    coeff, xval = DC.terms(n, seed=P * 100 + F)
    x, index = DC.gathered(xval, seed=7)
    offsets = DC.offsets_of(lens)
    want = FC.rows(DC.model(coeff, x, offsets, index))
    got, _ = _dot(sim, coeff, x, offsets, index, P, F)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0]
    assert not got[0].any()                                                     # the empty segment is Fr::zero()
    got, _ = _dot(sim, coeff, xval, offsets, None, P, F)                        # index == NULL: x[t]
    assert np.array_equal(got, want)
    at = 0
    for L, w in zip(lens, want):                                                # every segment as a call of its own
        got, _ = _dot(sim, coeff[at:at + L], xval[at:at + L], [0, L], None, P, F)
        assert np.array_equal(got[0], w), L
        at += L


def test_the_bytes_do_not_depend_on_the_plan(sim):
    lens = [0, 1, 5, 37, 300, 0, 64]
    coeff, xval = DC.terms(sum(lens), seed=3)
    x, index = DC.gathered(xval, seed=4)
    offsets = DC.offsets_of(lens)
    want = FC.rows(DC.model(coeff, x, offsets, index))
    for P in PIECES + (1, 3, 64):
        for F in FANS + (3,):
            for step in (1 << 22, 7, 1):
                got, _ = _dot(sim, coeff, x, offsets, index, P, F, step)
                assert np.array_equal(got, want), (P, F, step)


@pytest.mark.parametrize("m", [1, 255, 256, 257])
def test_segment_counts_around_a_workgroup(sim, m):
    P, F = sim.hsd_shipped_piece(), sim.hsd_shipped_fan()
    cyc = [L for L in DC.lengths(P, F) if L <= F * P + 1]
    lens = [cyc[j % len(cyc)] for j in range(m)]
    coeff, xval = DC.terms(sum(lens), seed=m)
    x, index = DC.gathered(xval, seed=m + 1)
    offsets = DC.offsets_of(lens)
    got, _ = _dot(sim, coeff, x, offsets, index, P, F)
    assert np.array_equal(got, FC.rows(DC.model(coeff, x, offsets, index)))


def test_all_indices_equal_and_repeated(sim):
    P, F = sim.hsd_shipped_piece(), sim.hsd_shipped_fan()
    lens = [3, P + 1, F * P + 1]
    n = sum(lens)
    coeff, _ = DC.terms(n, seed=11)
    x = FC.values(5, seed=12)
    for index in ([4] * n, [0] * n, [t % 5 for t in range(n)], [4 - t % 5 for t in range(n)]):
        got, _ = _dot(sim, coeff, x, DC.offsets_of(lens), index, P, F)
        assert np.array_equal(got, FC.rows(DC.model(coeff, x, DC.offsets_of(lens), index)))
    got, _ = _dot(sim, coeff, [FC.R - 1], DC.offsets_of(lens), [0] * n, P, F)                    # nx = 1
    assert np.array_equal(got, FC.rows(DC.model(coeff, [FC.R - 1], DC.offsets_of(lens), [0] * n)))


def test_empty_segments_first_last_and_adjacent(sim):
    P, F = sim.hsd_shipped_piece(), sim.hsd_shipped_fan()
    for lens in ([0, 3], [3, 0], [0, 0, 3, 0, 0, P + 2, 0], [0], [0, 0, 0]):
        coeff, xval = DC.terms(sum(lens), seed=5)
        got, _ = _dot(sim, coeff, xval, DC.offsets_of(lens), None, P, F)
        assert np.array_equal(got, FC.rows(DC.model(coeff, xval, DC.offsets_of(lens))))
        assert all(not got[j].any() for j, L in enumerate(lens) if L == 0)


def test_an_index_out_of_range_contributes_zero_in_the_device_form(sim):
    """the _dev entry point cannot read its index: an entry >= nx is outside its contract but memory safe - the body compares before it
    loads.  (The host-buffer entry point rejects such an index: tests/test_dot_abi.py.)  Run here only, never on a device."""
    P, F = sim.hsd_shipped_piece(), sim.hsd_shipped_fan()
    lens = [4, P + 3]
    n = sum(lens)
    coeff, _ = DC.terms(n, seed=21)
    x = FC.values(6, seed=22)
    index = [t % 6 for t in range(n)]
    for bad in (6, 1 << 63, (1 << 64) - 1):
        idx = list(index); idx[1] = bad; idx[6] = bad; idx[n - 1] = bad
        got, _ = _dot(sim, coeff, x, DC.offsets_of(lens), idx, P, F)
        kept = [0 if t in (1, 6, n - 1) else c for t, c in enumerate(coeff)]
        assert np.array_equal(got, FC.rows(DC.model(kept, x, DC.offsets_of(lens), index))), bad


@pytest.mark.parametrize("F", FANS)
@pytest.mark.parametrize("P", PIECES)
def test_the_invariants_of_the_plan(sim, P, F):
    lens = DC.lengths(P, F) + [0, 0, 3 * F * P + 5]
    offsets = DC.offsets_of(lens)
    pieces, levels, slots = _plan(sim, offsets, P, F)
    m = len(lens)
    assert int(levels[:, 1].sum()) == len(pieces) and list(levels[:, 0]) == list(np.concatenate([[0], np.cumsum(levels[:, 1])[:-1]]))
    assert len(levels) == 1 + max(DC.plan_levels(L, P, F) for L in lens)
    lo, cnt = levels[0]
    product = pieces[lo:lo + cnt]
    covered = np.zeros(int(offsets[-1]), np.int64)
    for first, ln, to_out, dst in product:
        assert 0 <= ln <= P
        covered[first:first + ln] += 1
    assert (covered == 1).all()                                                 # every term in exactly one piece
    assert len(product) == sum(max(1, -(-L // P)) for L in lens)
    assert sorted(int(d) for _, _, t, d in pieces if t) == list(range(m))       # every out[j] written exactly once
    written = sorted(int(d) for _, _, t, d in pieces if not t)
    assert written == list(range(slots))                                        # every slot written exactly once
    read = np.zeros(slots, np.int64)
    for l in range(1, len(levels)):
        lo, cnt = levels[l]
        for first, ln, to_out, dst in pieces[lo:lo + cnt]:
            assert 1 <= ln <= F                                                 # no fold lane takes more than F
            read[first:first + ln] += 1
    assert (read == 1).all()                                                    # every partial sum is folded exactly once
    # per segment: the level its result is written on is the stated count
    level_of = {}
    for l, (lo, cnt) in enumerate(levels):
        for first, ln, to_out, dst in pieces[lo:lo + cnt]:
            if to_out: level_of[int(dst)] = l
    assert [level_of[j] for j in range(m)] == [DC.plan_levels(L, P, F) for L in lens]
    assert slots < 2 * int(offsets[-1]) // P + 64 * m


def test_sub_launches_cut_every_level(sim):
    P, F = 8, 16
    lens = [P] * 25 + [P * 20]                                                  # 25 + 20 = 45 pieces, then 2 fold pieces and 1
    coeff, xval = DC.terms(sum(lens), seed=9)
    got, launches = _dot(sim, coeff, xval, DC.offsets_of(lens), None, P, F, step=20)
    assert launches == (3, 2)
    assert np.array_equal(got, FC.rows(DC.model(coeff, xval, DC.offsets_of(lens))))


def test_the_argument_checks(sim):
    D = C.c_void_p(0x1000)
    off = lambda *v: (C.c_size_t * len(v))(*v)
    idx = lambda *v: (C.c_uint64 * len(v))(*v)
    ok = lambda *a: sim.hsd_check(*a)
    assert ok(D, None, 0, D, 3, off(0, 1, 3), 2, D, 1) == 0
    assert ok(D, idx(0, 1, 1), 1, D, 2, off(0, 1, 3), 2, D, 1) == 0
    assert ok(D, None, 0, D, 3, None, 2, D, 1) == BAD_ARG                       # offsets == NULL with m > 0
    assert ok(D, None, 0, D, 3, off(1, 1, 3), 2, D, 1) == BAD_ARG               # offsets[0] != 0
    assert ok(D, None, 0, D, 3, off(0, 4, 3), 2, D, 1) == BAD_ARG               # decreasing
    assert ok(D, None, 0, D, (1 << 40) + 1, off(0, (1 << 40) + 1), 1, D, 0) == BAD_ARG
    assert ok(None, None, 0, D, 3, off(0, 1, 3), 2, D, 1) == BAD_ARG and ok(D, None, 0, None, 3, off(0, 1, 3), 2, D, 1) == BAD_ARG
    assert ok(D, None, 0, D, 3, off(0, 1, 3), 2, None, 1) == BAD_ARG
    assert ok(D, None, 0, D, 4, off(0, 1, 3), 2, D, 1) == BAD_ARG               # index == NULL with nx != n
    assert ok(D, idx(0, 2, 1), 1, D, 2, off(0, 1, 3), 2, D, 1) == BAD_ARG       # index out of range: the host-buffer form only
    assert ok(D, idx(0, 2, 1), 1, D, 2, off(0, 1, 3), 2, D, 0) == 0
    assert ok(None, None, 0, None, 0, off(0, 0, 0), 2, D, 1) == 0               # only empty segments: no term is read
