"""Segmented scans over Fr on an MI355X (run with -m gpu): bn254_fr_scan_batch, its _dev entry point, the Python faces and bn_amd.poly's
powers / divide_linear / evaluate.  The model is Python integers (tests/scan_cases.py over tests/fr_cases.py): the expected bytes are the
limbs of v * 2^256 mod r, and they do not depend on how the plan cuts a segment.  The shapes are the smallest that reach every seam of the plan
for the shipped piece length P and fan F, read from the library's internal hooks: around one piece, one down lane, a first and a second up
level, two workgroups of lanes, two sub-launches of a level."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as FC
import scan_cases as SC

pytestmark = pytest.mark.gpu
SCOPES = ("fr_scan_reduce", "fr_scan_up", "fr_scan_down", "fr_scan")


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_scan_piece.argtypes = []; l.bn254_fr_scan_piece.restype = C.c_uint
    l.bn254_fr_scan_fan.argtypes = []; l.bn254_fr_scan_fan.restype = C.c_uint
    l.bn254_fr_scan_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def PF(lib):
    return int(lib.bn254_fr_scan_piece()), int(lib.bn254_fr_scan_fan())


@pytest.fixture(scope="module")
def every_length(PF):
    """one call over the whole length list, empty segments first, last and adjacent: (lens, offsets, a per term, a per segment, b, init) as
    integers and the same as limb rows - computed once, never changed"""
    lens = [0] + SC.lengths(*PF) + [0, 0, 3, 0]
    n = sum(lens)
    ints = (SC.values(n, 1), SC.values(len(lens), 2), SC.values(n, 3), SC.values(len(lens), 4))
    return (lens, SC.offsets_of(lens)) + ints + tuple(FC.rows(v) for v in ints)


def _diff(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8]


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    assert got.tobytes() == want.tobytes(), _diff(got, want)


FLAGS = [dict(), dict(reverse=True), dict(exclusive=True), dict(a_per_segment=True), dict(reverse=True, exclusive=True, a_per_segment=True)]


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "+".join(f) or "none")
def test_the_general_recurrence_with_every_flag(eng, every_length, flags):
    lens, offsets, a, a_seg, b, init, A, A_seg, B, I = every_length
    per = flags.get("a_per_segment", False)
    got = eng.fr_scan_batch(A_seg if per else A, B, offsets, I, **flags)
    _same(got, FC.rows(SC.model(a_seg if per else a, b, offsets, init, **flags)))


def test_prefix_sums_and_products_with_both_defaults_of_init(eng, every_length):
    lens, offsets, a, a_seg, b, init, A, A_seg, B, I = every_length
    _same(eng.fr_scan_batch(None, B, offsets), FC.rows(SC.model(None, b, offsets)))                         # sums from zero
    _same(eng.fr_scan_batch(A, None, offsets), FC.rows(SC.model(a, None, offsets)))                         # products from one
    _same(eng.fr_scan_batch(A, B, offsets), FC.rows(SC.model(a, b, offsets)))                               # the recurrence from zero
    _same(eng.fr_scan_batch(None, B, offsets, I), FC.rows(SC.model(None, b, offsets, init)))                # an explicit init
    _same(eng.fr_scan_batch(A, None, offsets, I, reverse=True), FC.rows(SC.model(a, None, offsets, init, reverse=True)))
    _same(eng.fr_scan_batch(A_seg, None, offsets, exclusive=True, a_per_segment=True), FC.rows(SC.model(a_seg, None, offsets, exclusive=True, a_per_segment=True)))


def test_257_segments_that_cycle_through_the_lengths(eng, PF):
    """two workgroups of direct lanes, folded segments among them; empty segments first, last and adjacent"""
    P, F = PF
    cyc = [L for L in SC.lengths(P, F) if L <= F * P + 1]
    lens = [0, 0] + [cyc[j % len(cyc)] for j in range(254)] + [0]
    assert len(lens) == 257
    n = sum(lens)
    a, b, init = SC.values(n, 5), SC.values(n, 6), SC.values(257, 7)
    offsets = SC.offsets_of(lens)
    _same(eng.fr_scan_batch(FC.rows(a), FC.rows(b), offsets, FC.rows(init)), FC.rows(SC.model(a, b, offsets, init)))


@pytest.mark.parametrize("reverse", [False, True])
def test_one_segment_of_two_up_levels_alone(eng, every_length, PF, reverse):
    P, F = PF
    lens, offsets, a, a_seg, b, init, A, A_seg, B, I = every_length
    L = F * F * P + 1
    j = lens.index(L)
    assert SC.up_levels(L, P, F) == 2 and SC.plan_levels(L, P, F) == 7
    lo = int(offsets[j])
    got = eng.fr_scan_batch(A[lo:lo + L], B[lo:lo + L], [0, L], I[j:j + 1], reverse=reverse)
    _same(got, FC.rows(SC.model(a[lo:lo + L], b[lo:lo + L], [0, L], init[j:j + 1], reverse=reverse)))


def test_the_seam_between_sub_launches(eng, lib, PF):
    """45 lanes in sub-launches of 20: the launches of the four scopes are those of the plan"""
    P, F = PF
    lens = [P] * 25 + [20 * P]
    n = sum(lens)
    a, b, init = SC.values(n, 9), SC.values(n, 10), SC.values(len(lens), 11)
    offsets = SC.offsets_of(lens)
    eng.profile(True); eng.profile_reset()
    assert lib.bn254_fr_scan_set_launch_max(20) == 0
    try:
        got = eng.fr_scan_batch(FC.rows(a), FC.rows(b), offsets, FC.rows(init))
        launches = tuple(eng.kernel_stats(s)[1] for s in SCOPES)
    finally:
        assert lib.bn254_fr_scan_set_launch_max(0) == 0
        eng.profile(False)
    assert launches == SC.launches(lens, P, F, 20)
    _same(got, FC.rows(SC.model(a, b, offsets, init)))


def test_the_dev_form_in_place_and_on_a_stream(eng, every_length):
    """device-resident operands on a stream that is not the default one; out is b, then out is a; the host offsets are overwritten as soon
    as the call has returned (the launches were planned from them)"""
    import torch
    lens, offsets, a, a_seg, b, init, A, A_seg, B, I = every_length
    m, n = len(lens), int(offsets[-1])
    stream = torch.cuda.Stream()
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")
    da, db, di, da2, db2 = dev(A), dev(B), dev(I), dev(A), dev(B)
    out = torch.zeros(n * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    off = [offsets.copy() for _ in range(3)]
    with torch.cuda.stream(stream):
        eng.fr_scan_batch_dev(da.data_ptr(), db.data_ptr(), di.data_ptr(), off[0], m, out.data_ptr(), reverse=True, stream=stream.cuda_stream)
        off[0][:] = 1 << 63
        eng.fr_scan_batch_dev(da.data_ptr(), db.data_ptr(), di.data_ptr(), off[1], m, db.data_ptr(), stream=stream.cuda_stream)             # out is b
        off[1][:] = 1 << 63
        eng.fr_scan_batch_dev(da2.data_ptr(), db2.data_ptr(), None, off[2], m, da2.data_ptr(), exclusive=True, stream=stream.cuda_stream)   # out is a
        off[2][:] = 1 << 63
    stream.synchronize()
    host = lambda t: t.cpu().numpy().view(np.uint64).reshape(n, 4)
    _same(host(out), FC.rows(SC.model(a, b, offsets, init, reverse=True)))
    _same(host(db), FC.rows(SC.model(a, b, offsets, init)))
    _same(host(da2), FC.rows(SC.model(a, b, offsets, None, exclusive=True)))
    assert host(da).tobytes() == A.tobytes()                                                    # an input that is not out is left alone


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr
    rng = np.random.default_rng(5)
    a = [Fr.random(rng) for _ in range(7)]
    b = [Fr.random(rng) for _ in range(6)] + [Fr.zero()]
    offsets = [0, 0, 3, 7, 7]
    init = [Fr.random(rng) for _ in range(4)]
    ints = lambda v: [x.v for x in v]
    want = [Fr(v) for v in SC.model(ints(a), ints(b), offsets, ints(init))]
    assert bn_amd.fr_scan_batch(a, b, offsets, init) == want
    assert bn_amd.fr_scan_batch(np.stack([c.limbs for c in a]), np.stack([c.limbs for c in b]), np.array(offsets), np.stack([c.limbs for c in init])) == want
    assert bn_amd.fr_scan_batch(None, b, offsets) == [Fr(v) for v in SC.model(None, ints(b), offsets)]
    prod = 1
    for x in a:
        prod = prod * x.v % FC.R
    assert bn_amd.fr_scan_batch(a, None, [0, 7], reverse=True)[0] == Fr(prod)                   # the last output of a product scan is the product
    assert bn_amd.fr_scan_batch([], None, [0]) == [] and bn_amd.fr_scan_batch(None, [], [0, 0]) == []


@pytest.mark.parametrize("which", [1, 2, 3])
def test_poly_powers_against_pow(eng, PF, which):
    from bn_amd import Fr, poly
    P, F = PF
    n = [1, P + 1, F * P + 1][which - 1]
    x = SC.values(8, 40 + which)[-1]
    assert poly.powers(Fr(x), n, engine=eng) == [Fr(pow(x, i, FC.R)) for i in range(n)]


def test_poly_divide_linear_and_evaluate(eng, PF):
    """degree F * P at a random z, at z = 0 and at a root of p: q * (X - z) + y == p in Python integers, and y == evaluate(p, z)"""
    from bn_amd import Fr, poly
    P, F = PF
    rng = np.random.default_rng(50)
    root = FC.rand(rng)
    g = [FC.rand(rng) for _ in range(F * P)]                                                    # p = g * (X - root): degree F * P, p(root) = 0
    p = [0] * (F * P + 1)
    for i, c in enumerate(g):
        p[i + 1] = (p[i + 1] + c) % FC.R
        p[i] = (p[i] - c * root) % FC.R
    for z in (FC.rand(rng), 0, root):
        q, y = poly.divide_linear([Fr(c) for c in p], Fr(z), engine=eng)
        assert len(q) == F * P
        assert y == Fr(sum(c * pow(z, i, FC.R) for i, c in enumerate(p))) == poly.evaluate(FC.rows(p), Fr(z), engine=eng)
        back = [0] * (F * P + 1)
        for i, c in enumerate(q):
            back[i + 1] = (back[i + 1] + c.v) % FC.R
            back[i] = (back[i] - c.v * z) % FC.R
        back[0] = (back[0] + y.v) % FC.R
        assert back == p, z
    assert y == Fr.zero() and [c.v for c in q] == g                                             # at the root the quotient is g itself
