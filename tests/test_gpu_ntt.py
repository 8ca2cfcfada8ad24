"""Number-theoretic transforms over Fr on an MI355X (run with -m gpu): bn254_fr_ntt_batch, its _dev entry point, the Python faces and
bn_amd.poly.  The model is Python integers (tests/ntt_cases.py): the expected bytes are the limbs of v * 2^256 mod r.  With the tile log
forced to 2 through the library's internal hook a transform of 2^7 elements takes four passes; with the shipped tile log T the sizes are
those around one tile (T - 1, T, T + 1) and one of three passes (min(2 T + 1, 21)), which is checked by the round trip and by few-term
sums."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as FC
import ntt_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_ntt_tile_log.argtypes = []; l.bn254_ntt_tile_log.restype = C.c_uint
    l.bn254_ntt_set_tile_log.argtypes = [C.c_uint]
    l.bn254_ntt_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def T(lib):
    return int(lib.bn254_ntt_tile_log())


def _shift(sh):
    return None if sh is None else FC.rows([sh])[0]


def _diff(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8]


def test_four_passes_of_a_tile_of_four_against_the_model(eng, lib):
    """tile log 2: log_n 0..7 is one to four passes, the last one ragged at odd log_n; count 1 and 3, both directions, the three shifts"""
    assert lib.bn254_ntt_set_tile_log(2) == 0
    try:
        for log_n in range(8):
            for count in (1, 3):
                vals = NC.batch(log_n, count, seed=100 + 10 * log_n + count)
                rows = FC.rows(vals)
                for inverse in (False, True):
                    for sh in NC.SHIFTS:
                        got = eng.fr_ntt_batch(rows, log_n, inverse, _shift(sh))
                        want = FC.rows(NC.ntt_batch(vals, log_n, inverse, sh))
                        assert got.shape == rows.shape and got.dtype == np.uint64
                        assert got.tobytes() == want.tobytes(), (log_n, count, inverse, sh, _diff(got, want))
    finally:
        assert lib.bn254_ntt_set_tile_log(0) == 0


def test_sizes_around_the_shipped_tile_against_the_model(eng, T):
    for log_n in (T - 1, T, T + 1):
        vals = NC.batch(log_n, 1, seed=200 + log_n)
        rows = FC.rows(vals)
        for inverse in (False, True):
            got = eng.fr_ntt_batch(rows, log_n, inverse, _shift(5))
            want = FC.rows(NC.ntt(vals, inverse, 5))
            assert got.tobytes() == want.tobytes(), (log_n, inverse, _diff(got, want))


@pytest.fixture(scope="module")
def three_passes(T):
    """log_n, dense random rows (Montgomery images drawn directly: canonical values) and the sparse input of six non-zeros"""
    log_n = min(2 * T + 1, 21)
    n = 1 << log_n
    rng = np.random.default_rng(300)
    dense = rng.integers(0, 1 << 64, (n, 4), dtype=np.uint64)
    dense[:, 3] >>= np.uint64(3)                                                 # every value below 2^253 < r: canonical
    assert int(dense[:, 3].max()) < (FC.R >> 192)
    pos = [0, 1, n // 2 - 1, n // 2, n - 1, int(rng.integers(2, n // 2 - 1))]
    terms = [(j, FC.rand(rng)) for j in pos]
    ks = sorted(set([0, 1, n // 2, n - 1] + [int(k) for k in np.random.default_rng(301).integers(0, n, 64)]))
    return log_n, dense, terms, ks


def test_three_passes_of_the_shipped_tile_round_trip(eng, three_passes):
    log_n, dense, _, _ = three_passes
    for sh in (None, 5):
        fwd = eng.fr_ntt_batch(dense, log_n, False, _shift(sh))
        assert not np.array_equal(fwd, dense)
        back = eng.fr_ntt_batch(fwd, log_n, True, _shift(sh))
        assert back.tobytes() == dense.tobytes(), (sh, _diff(back, dense))


def test_three_passes_of_the_shipped_tile_against_few_term_sums(eng, three_passes):
    log_n, _, terms, ks = three_passes
    rows = np.zeros((1 << log_n, 4), np.uint64)
    for j, v in terms:
        rows[j] = FC.rows([v])[0]
    for inverse, sh in ((False, None), (False, 5), (True, None), (True, 5)):
        got = eng.fr_ntt_batch(rows, log_n, inverse, _shift(sh))
        want = FC.rows(NC.sparse_outputs(terms, log_n, ks, inverse, sh))
        assert got[ks].tobytes() == want.tobytes(), (inverse, sh, [ks[i] for i in _diff(got[ks], want)])


def test_the_seams_between_sub_launches(eng, lib):
    """45 transforms of 8 in sub-launches of 64 elements: six launches of the one pass"""
    log_n, count = 3, 45
    vals = NC.batch(log_n, count, seed=400)
    rows = FC.rows(vals)
    want = FC.rows(NC.ntt_batch(vals, log_n, False, 5))
    assert lib.bn254_ntt_set_launch_max(64) == 0
    try:
        eng.profile(True); eng.profile_reset()
        got = eng.fr_ntt_batch(rows, log_n, False, _shift(5))
        launches = eng.kernel_stats("ntt")[1]
    finally:
        eng.profile(False)
        assert lib.bn254_ntt_set_launch_max(0) == 0
    assert got.tobytes() == want.tobytes(), _diff(got, want)
    passes = 1
    assert launches == passes * 6
    assert lib.bn254_ntt_set_tile_log(2) == 0                                    # two passes of a tile of four: (2 + 1 stages) x 6 sub-launches
    assert lib.bn254_ntt_set_launch_max(64) == 0
    try:
        eng.profile(True); eng.profile_reset()
        got = eng.fr_ntt_batch(rows, log_n, False, _shift(5))
        launches = eng.kernel_stats("ntt")[1]
    finally:
        eng.profile(False)
        assert lib.bn254_ntt_set_launch_max(0) == 0 and lib.bn254_ntt_set_tile_log(0) == 0
    assert got.tobytes() == want.tobytes(), _diff(got, want)
    assert launches == 2 * 6


def test_in_place_on_the_host_and_on_a_stream(eng, T):
    """out == in through the host call; through the _dev call on a stream that is not the default one, out of place and in place, with the
    host `shift` overwritten as soon as the call has returned"""
    import torch
    for log_n, count in ((5, 3), (T + 2, 1)):                                  # one pass; two passes
        vals = NC.batch(log_n, count, seed=500 + log_n)
        rows = FC.rows(vals)
        want = FC.rows(NC.ntt_batch(vals, log_n, True, NC.SHIFT_RANDOM))
        buf = rows.copy()
        p = buf.ctypes.data_as(C.c_void_p)
        sh = _shift(NC.SHIFT_RANDOM).copy()
        from bn_amd import _native
        _native.check(eng._lib.bn254_fr_ntt_batch(eng._h, p, p, log_n, count, 1, sh.ctypes.data_as(C.c_void_p)))
        assert buf.tobytes() == want.tobytes(), ("host, in place", log_n, _diff(buf, want))
        stream = torch.cuda.Stream()
        d_in = torch.from_numpy(rows.view(np.int64)).cuda()
        d_out = torch.zeros_like(d_in)
        d_io = d_in.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            eng.fr_ntt_batch_dev(d_in.data_ptr(), d_out.data_ptr(), log_n, count, True, sh, stream.cuda_stream)
            sh[:] = 7                                                            # read before the call returned
            sh2 = _shift(NC.SHIFT_RANDOM).copy()
            eng.fr_ntt_batch_dev(d_io.data_ptr(), d_io.data_ptr(), log_n, count, True, sh2, stream.cuda_stream)
            sh2[:] = 0
        stream.synchronize()
        assert d_out.cpu().numpy().view(np.uint64).tobytes() == want.tobytes(), ("stream, out of place", log_n)
        assert d_io.cpu().numpy().view(np.uint64).tobytes() == want.tobytes(), ("stream, in place", log_n)
        assert d_in.cpu().numpy().view(np.uint64).tobytes() == rows.tobytes(), "the input was written"


def test_three_passes_in_place_on_the_device(eng, lib):
    """an odd number of passes in place: the first pass may not write what the others still read (tile log 2, log_n 5: passes of 2, 2, 1)"""
    import torch
    log_n, count = 5, 3
    vals = NC.batch(log_n, count, seed=550)
    want = FC.rows(NC.ntt_batch(vals, log_n, False, None))
    d_io = torch.from_numpy(FC.rows(vals).view(np.int64)).cuda()
    assert lib.bn254_ntt_set_tile_log(2) == 0
    try:
        eng.fr_ntt_batch_dev(d_io.data_ptr(), d_io.data_ptr(), log_n, count, False, None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        assert lib.bn254_ntt_set_tile_log(0) == 0
    assert d_io.cpu().numpy().view(np.uint64).tobytes() == want.tobytes()


def test_the_tables_are_built_once_and_reused():
    import bn_amd
    e = bn_amd.Engine(0)                                                         # a context of its own: its tables are not built yet
    e.profile(True); e.profile_reset()
    try:
        a5, a12 = NC.batch(5, 1, seed=600), NC.batch(12, 1, seed=601)
        first = e.fr_ntt_batch(FC.rows(a5), 5)
        ms, launches = e.kernel_stats("ntt_table")
        assert launches >= 1 and ms > 0
        mid = e.fr_ntt_batch(FC.rows(a12), 12)
        third = e.fr_ntt_batch(FC.rows(a5), 5)
        assert first.tobytes() == third.tobytes() == FC.rows(NC.ntt(a5)).tobytes()
        assert mid.tobytes() == FC.rows(NC.ntt(a12)).tobytes()
        before = e.kernel_stats("ntt_table")[1]
        assert e.fr_ntt_batch(FC.rows(a5), 5).tobytes() == first.tobytes()
        assert e.kernel_stats("ntt_table")[1] == before == launches              # neither another size nor a repeat builds anything
        coset = e.fr_ntt_batch(FC.rows(a5), 5, False, _shift(5))
        built = e.kernel_stats("ntt_table")[1]
        assert built == before + 1 and coset.tobytes() == FC.rows(NC.ntt(a5, False, 5)).tobytes()
        assert e.fr_ntt_batch(FC.rows(a5), 5, False, _shift(5)).tobytes() == coset.tobytes() and e.kernel_stats("ntt_table")[1] == built
        # a forward pair holds s^i whatever the size: another size with the same shift builds nothing; an inverse pair carries n^-1
        assert e.fr_ntt_batch(FC.rows(a12), 12, False, _shift(5)).tobytes() == FC.rows(NC.ntt(a12, False, 5)).tobytes()
        assert e.fr_ntt_batch(FC.rows(a5), 5, False, _shift(5)).tobytes() == coset.tobytes() and e.kernel_stats("ntt_table")[1] == built
        assert e.fr_ntt_batch(coset, 5, True, _shift(5)).tobytes() == FC.rows(a5).tobytes() and e.kernel_stats("ntt_table")[1] == built + 1
        assert e.fr_ntt_batch(FC.rows(a12), 12, True, _shift(5)).tobytes() == FC.rows(NC.ntt(a12, True, 5)).tobytes() and e.kernel_stats("ntt_table")[1] == built + 2
    finally:
        e.profile(False)


def test_python_faces(eng):
    import bn_amd
    from bn_amd import Fr
    vals = NC.batch(4, 1, seed=700)
    want = NC.ntt(vals, False, 5)
    assert [x.v for x in bn_amd.fr_ntt([Fr(v) for v in vals], shift=5, engine=eng)] == want
    assert [x.v for x in bn_amd.fr_ntt(FC.rows(vals), shift=Fr(5), engine=eng)] == want
    assert [x.v for x in bn_amd.fr_ntt([Fr(v) for v in want], inverse=True, shift=5, engine=eng)] == vals
    two = NC.batch(3, 2, seed=701)
    got = bn_amd.fr_ntt_batch([[Fr(v) for v in two[:8]], [Fr(v) for v in two[8:]]], inverse=True, engine=eng)
    assert [[x.v for x in row] for row in got] == [NC.ntt(two[:8], True), NC.ntt(two[8:], True)]
    got = bn_amd.fr_ntt_batch(FC.rows(two).reshape(2, 8, 4), engine=eng)
    assert [[x.v for x in row] for row in got] == [NC.ntt(two[:8]), NC.ntt(two[8:])]
    assert bn_amd.fr_ntt([Fr(9)], engine=eng) == [Fr(9)]                          # n = 1


def _poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % FC.R
    return out


def _poly_divmod_zh(p, n):
    """(quotient, remainder) of p by X^n - 1"""
    p = list(p)
    q = [0] * max(len(p) - n, 0)
    for i in range(len(p) - 1, n - 1, -1):
        q[i - n] = p[i]
        p[i - n] = (p[i - n] + p[i]) % FC.R
        p[i] = 0
    return q, p[:n]


def test_poly_mul_and_quotient(eng):
    from bn_amd import Fr, poly
    rng = np.random.default_rng(800)
    a = [FC.rand(rng) for _ in range(6)]; b = [FC.rand(rng) for _ in range(8)]      # degrees 5 and 7: 13 coefficients, padded to 16
    assert [x.v for x in poly.mul([Fr(v) for v in a], [Fr(v) for v in b], engine=eng)] == _poly_mul(a, b)
    assert [x.v for x in poly.mul([Fr(a[0])], [Fr(b[0])], engine=eng)] == [a[0] * b[0] % FC.R]
    for n in (8, 16):
        log_n = n.bit_length() - 1
        A = [FC.rand(rng) for _ in range(n)]; B = [FC.rand(rng) for _ in range(n)]     # degree < n
        h, Cc = _poly_divmod_zh(_poly_mul(A, B), n)                                     # A B = h Z_H + C with C = A B mod Z_H
        ev = [NC.ntt(p) for p in (A, B, Cc)]
        got = poly.quotient(*[[Fr(v) for v in e] for e in ev], engine=eng)
        assert [x.v for x in got] == h + [0] * (n - len(h)), n
