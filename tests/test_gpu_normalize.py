"""Batched normalize and projective equality on an MI355X (run with -m gpu): bn254_g{1,2}_normalize_batch, bn254_g{1,2}_eq_batch, their
_dev entry points and the Python faces.  The inputs (tests/normalize_cases.py) are built on the CPU from known affine points, re-represented
as (l^2 x, l^3 y, l z) with l random, l = 1 and l = q - 1, with points at infinity - (0, 1, 0) and z = 0 under arbitrary x, y - at every
position of a run.  normalize is compared bytewise with bn254_g{1,2}_mul_batch by Fr::one() on the same input (the parity definition) and
with bn_model's (x/z^2, y/z^3, 1); eq with the crate's function restated over bn_model, and with the bytes of the two normalized points.
Sizes, with K the shipped run length: 1, K - 1, K, K + 1, 2 K + 3, 256 K + 1 (the first point of a second workgroup of G1), and the seam
between sub-launches through the library's internal test hook (three sub-launches of 20, 20 and 5 points)."""
import ctypes as C

import numpy as np
import pytest

import bn_model as M
import normalize_cases as NC

pytestmark = pytest.mark.gpu

FR_ONE = np.array(M.to_mont_limbs(1, M.R_ORD), np.uint64)


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_normalize_run.argtypes = []; l.bn254_normalize_run.restype = C.c_uint
    l.bn254_normalize_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def K(lib):
    return int(lib.bn254_normalize_run())


def _sizes(K):
    return sorted({1, max(1, K - 1), K, K + 1, 2 * K + 3, 256 * K + 1})


@pytest.fixture(scope="module")
def cases(K):
    """{g: [(n, phase, model points, rows)]}: every phase of the pattern at the small sizes, one at the large one; built once"""
    out = {}
    for g in (1, 2):
        out[g] = []
        for n in _sizes(K):
            for phase in (range(6) if n <= 2 * K + 3 else (0,)):
                pts = NC.points(g, n, K, phase, seed=1000 * g + 10 * n + phase)
                out[g].append((n, phase, pts, NC.rows(g, pts)))
    return out


def _normalize(eng, g):
    return eng.g1_normalize if g == 1 else eng.g2_normalize


def _mul_by_one(eng, g, P):
    """how a point was normalized before: the general kernel with every scalar Fr::one()"""
    return (eng.g1_mul_batch if g == 1 else eng.g2_mul_batch)(P, np.tile(FR_ONE, (P.shape[0], 1)))


def _model_rows(g, pts, idx):
    return NC.rows(g, [NC.model_normalize(g, pts[i]) for i in idx])


@pytest.mark.parametrize("g", [1, 2])
def test_normalize_is_mul_by_one_and_the_model(eng, cases, K, g):
    seen = set()
    for n, phase, pts, P in cases[g]:
        got = _normalize(eng, g)(P)
        assert got.shape == P.shape and got.dtype == np.uint64
        assert got.tobytes() == _mul_by_one(eng, g, P).tobytes(), (g, n, phase)
        idx = range(n) if n <= 2 * K + 3 else sorted({0, K - 1, K, n - 1, n - 2, 64 * K - 1, 64 * K} | set(np.random.default_rng(n).choice(n, 57, replace=False).tolist()))
        assert got[list(idx)].tobytes() == _model_rows(g, pts, idx).tobytes(), (g, n, phase)
        seen.add(n)
    assert seen == set(_sizes(K))


@pytest.mark.parametrize("g", [1, 2])
def test_normalize_in_place_and_on_a_stream(eng, cases, K, g):
    """out == p through the host call and the _dev call, the latter on a stream that is not the default one"""
    import torch
    words = NC.WORDS[g]
    stream = torch.cuda.Stream()
    for n, phase, pts, P in cases[g]:
        if phase not in (0, 3):
            continue
        want = _normalize(eng, g)(P)
        buf = P.copy()
        fn = eng._lib.bn254_g1_normalize_batch if g == 1 else eng._lib.bn254_g2_normalize_batch
        assert fn(eng._h, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), n) == 0
        assert buf.tobytes() == want.tobytes(), ("host in place", g, n, phase)
        d = torch.from_numpy(P.view(np.int64)).to("cuda:0")
        o = torch.empty_like(d)
        torch.cuda.synchronize()
        dev = eng.g1_normalize_dev if g == 1 else eng.g2_normalize_dev
        with torch.cuda.stream(stream):
            dev(d.data_ptr(), o.data_ptr(), n, stream.cuda_stream)            # out of place ...
            dev(d.data_ptr(), d.data_ptr(), n, stream.cuda_stream)            # ... and in place
        stream.synchronize()
        assert o.cpu().numpy().view(np.uint64).reshape(n, words).tobytes() == want.tobytes(), ("dev", g, n, phase)
        assert d.cpu().numpy().view(np.uint64).reshape(n, words).tobytes() == want.tobytes(), ("dev in place", g, n, phase)


@pytest.mark.parametrize("g", [1, 2])
def test_normalize_across_sub_launches(eng, lib, K, g):
    """three sub-launches (20, 20, 5 points) through the internal hook: every one cuts its own runs, the last run of each is short"""
    pts = NC.points(g, 45, K, 1, seed=45 + g)
    P = NC.rows(g, pts)
    want = _model_rows(g, pts, range(45))
    assert lib.bn254_normalize_set_launch_max(20) == 0
    try:
        got = _normalize(eng, g)(P)
    finally:
        assert lib.bn254_normalize_set_launch_max(0) == 0
    assert got.tobytes() == want.tobytes()
    assert _normalize(eng, g)(P).tobytes() == want.tobytes()


@pytest.mark.parametrize("g", [1, 2])
def test_eq_against_the_model_and_the_normalized_bytes(eng, K, g):
    import torch
    eq = eng.g1_eq if g == 1 else eng.g2_eq
    seen = []
    for n in _sizes(K):
        a, b = NC.pairs(g, n, seed=7 * n + g)
        A, B = NC.rows(g, a), NC.rows(g, b)
        want = np.array([NC.model_eq(g, x, y) for x, y in zip(a, b)], bool)
        got = eq(A, B)
        assert got.dtype == np.bool_ and got.shape == (n,)
        assert np.array_equal(got, want), (g, n, np.nonzero(got != want)[0][:8])
        assert np.array_equal(eq(B, A), want), (g, n)
        na, nb = _normalize(eng, g)(A), _normalize(eng, g)(B)
        assert np.array_equal(got, (na == nb).all(axis=1)), (g, n)               # eq(a, b) == (normalize(a) == normalize(b) bytewise)
        assert eq(A, A).all()
        seen += want.tolist()
    assert True in seen and False in seen
    # the raw 1 / 0 of the _dev call, on a stream that is not the default one
    stream = torch.cuda.Stream()
    da, db = (torch.from_numpy(x.view(np.int64)).to("cuda:0") for x in (A, B))
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        (eng.g1_eq_dev if g == 1 else eng.g2_eq_dev)(da.data_ptr(), db.data_ptr(), out.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert out.cpu().numpy().tolist() == want.astype(np.int32).tolist()


def test_eq_covers_every_kind_of_pair():
    """the expected values of the six kinds, from the model alone (no case of the list above is vacuous)"""
    for g in (1, 2):
        a, b = NC.pairs(g, 12, seed=3)
        assert [NC.model_eq(g, x, y) for x, y in zip(a, b)] == [True, False, False, True, False, False] * 2
        assert a[1][0] != b[1][0] and NC.model_normalize(g, a[1])[0] == NC.model_normalize(g, b[1])[0]      # P, -P: x agrees, y does not


def test_the_python_faces(eng):
    import bn_amd
    from bn_amd import Fr, G1, G2
    rng = np.random.default_rng(11)
    for cls, norm_batch, eq_batch in ((G1, bn_amd.g1_normalize_batch, bn_amd.g1_eq_batch), (G2, bn_amd.g2_normalize_batch, bn_amd.g2_eq_batch)):
        p = cls.random(rng)
        s = p + cls.zero()
        assert (s == p) is True and (p == s) is True
        d = p + p                                                              # raw Jacobian limbs, z != 1
        assert not np.array_equal(d.limbs, (d * Fr.one()).limbs)
        assert np.array_equal(d.normalize().limbs, (d * Fr.one()).limbs)
        assert (d == p) is False and (d == d.normalize()) is True and (cls.zero() == p - p) is True
        assert (p == 5) is False
        assert [np.array_equal(x.limbs, y.limbs) for x, y in zip(norm_batch([d, p, cls.zero()]), [d * Fr.one(), p, cls.zero()])] == [True] * 3
        assert eq_batch([d, p, cls.zero()], [d.normalize(), d, p - p]) == [True, False, True]
