"""The wire format on an MI355X (run with -m gpu): bn254_{fr,g1,g2}_{encode,decode}_batch and bn254_g{1,2}_{encode,decode}_stream against the
integer model of wire_cases.py and the oracle - records that fail several checks at once, the 512-bit extremes of the Fq2 split, the sizes around
a wave with guard records behind `out` and `status`, and the ends of the byte stream: cut records, lone tags, max_points, a `cap` that is
exactly enough and one byte short.  Every comparison is of exact bytes."""
import ctypes as C

import numpy as np
import pytest

import wire_cases as W

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257]
PATTERN = 0x5a5a5a5a5a5a5a5a
BAD_ARG = -2


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    e = bn_amd.Engine(0)
    yield e
    e.close()


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _decode_fns(eng, oracle):
    return {1: (eng.g1_decode_batch, oracle.g1_decode), 2: (eng.g2_decode_batch, oracle.g2_decode)}


@pytest.mark.parametrize("g", [1, 2])
def test_collisions_and_extremes_in_one_call(oracle, eng, g):
    """every record of the collision list - several failed checks at once, tag 0 over all of them, the 512-bit extremes - in ONE batch: status and
    output equal the model's and the oracle's"""
    from conftest import canon_infinity
    cases = W.collision_cases(g)
    dec, ref = _decode_fns(eng, oracle)[g]
    out, st = dec(np.stack([np.frombuffer(c.rec, np.uint8) for c in cases]))
    assert st.dtype == np.int32 and st.tolist() == [c.status for c in cases], [(c.name, int(s), c.status) for c, s in zip(cases, st) if s != c.status][:8]
    for i, c in enumerate(cases):
        assert out[i].tobytes() == W.words(g, c.point).tobytes(), c.name                  # rejected records and tag 0: G::zero()
        rc, want = ref(np.frombuffer(c.rec, np.uint8))
        assert rc == st[i] and (rc != 0 or canon_infinity(want).tobytes() == out[i].tobytes()), c.name
    assert set(st.tolist()) == ({0, 1, 3, 4} if g == 1 else {0, 2, 3, 4, 5})


def test_fr_cases_in_one_call(oracle, eng):
    cases = W.fr_cases()
    out, st = eng.fr_decode_batch(np.stack([np.frombuffer(rec, np.uint8) for _, rec, _, _ in cases]))
    assert st.tolist() == [c[2] for c in cases]
    for i, (name, rec, status, v) in enumerate(cases):
        assert out[i].tobytes() == W.fr_words(v).tobytes(), name                          # a rejected record is Fr::zero()
        rc, want = oracle.fr_decode(np.frombuffer(rec, np.uint8))
        assert rc == status and (rc != 0 or want.tobytes() == out[i].tobytes()), name
    ok = [i for i, c in enumerate(cases) if c[2] == 0]
    assert eng.fr_encode_batch(out[ok]).tobytes() == b"".join(cases[i][1] for i in ok)


def _guarded(lib, eng, name, inp, n, out_shape, out_dtype, with_status):
    """the C entry point on buffers one record longer than n, filled with a pattern -> (out[:n], status[:n] or None); the guard record and the
    input must come back as they went in"""
    inp = np.ascontiguousarray(inp)
    keep = inp.copy()
    fill = PATTERN if out_dtype == np.uint64 else 0x5a
    out = np.full((n + 1,) + out_shape, fill, out_dtype)
    st = np.full(n + 1, -7, np.int32)
    rc = getattr(lib, name)(eng._h, _p(inp), _p(out), _p(st), n) if with_status else getattr(lib, name)(eng._h, _p(inp), _p(out), n)
    assert rc == 0, (name, n, rc)
    assert (out[n] == fill).all() and st[n] == -7, (name, n, "the guard record was written")
    assert inp.tobytes() == keep.tobytes(), (name, n, "the input was written")
    if not with_status:
        assert (st == -7).all()
    return out[:n], st[:n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("g", [1, 2])
def test_point_batches_around_a_wave_with_guards(eng, g, n):
    """65- and 129-byte records: every lane reads and writes at another misalignment; the last lane of the last block is the one next to the guard"""
    lib = eng._lib
    b, want_st, want_p = W.decode_batch(g, n, start=3 * n)
    out, st = _guarded(lib, eng, f"bn254_g{g}_decode_batch", b, n, (W.WORDS[g],), np.uint64, True)
    assert st.tolist() == want_st.tolist() and out.tobytes() == want_p.tobytes(), (np.flatnonzero(st != want_st)[:8], np.flatnonzero((out != want_p).any(axis=1))[:8])
    if n >= 63:
        assert any(r[0] == 0 and r[1:].any() for r in b) and len(set(want_st.tolist())) >= 4        # tag 0 with padding that is not zero, most statuses
    P, want_b, normal = W.encode_batch(g, n, start=n)
    enc, _ = _guarded(lib, eng, f"bn254_g{g}_encode_batch", P, n, (W.RS[g],), np.uint8, False)
    assert enc.tobytes() == want_b.tobytes(), np.flatnonzero((enc != want_b).any(axis=1))[:8]
    if n >= 63:
        z = P[:, 2 * W.WORDS[g] // 3:]
        assert (z != normal[:, 2 * W.WORDS[g] // 3:]).any(axis=1).sum() >= n // 3                    # Jacobian inputs that are not normalised
        assert any(not z[i].any() and P[i, :W.WORDS[g] // 3].any() for i in range(n))               # infinity with x != 0
    back, st = _guarded(lib, eng, f"bn254_g{g}_decode_batch", enc, n, (W.WORDS[g],), np.uint64, True)
    assert not st.any() and back.tobytes() == normal.tobytes()                                      # decode(encode(P)) == normalize(P)
    if n == 65:
        norm = eng.g1_normalize(P) if g == 1 else eng.g2_normalize(P)
        assert norm.tobytes() == back.tobytes()                                                     # ... and the library's own normalize


@pytest.mark.parametrize("n", SIZES)
def test_fr_batches_around_a_wave_with_guards(eng, n):
    lib = eng._lib
    b, want_st, want_k = W.fr_batch(n, start=n)
    out, st = _guarded(lib, eng, "bn254_fr_decode_batch", b, n, (4,), np.uint64, True)
    assert st.tolist() == want_st.tolist() and out.tobytes() == want_k.tobytes()
    want_b = b.copy(); want_b[want_st != 0] = 0                                 # a rejected record came back as Fr::zero(): 32 zero bytes
    enc, _ = _guarded(lib, eng, "bn254_fr_encode_batch", want_k, n, (32,), np.uint8, False)
    assert enc.tobytes() == want_b.tobytes()
    back, st = _guarded(lib, eng, "bn254_fr_decode_batch", enc, n, (4,), np.uint64, True)
    assert not st.any() and back.tobytes() == want_k.tobytes()


def _stream_fns(eng, g):
    return (eng.g1_encode_stream, eng.g1_decode_stream) if g == 1 else (eng.g2_encode_stream, eng.g2_decode_stream)


@pytest.mark.parametrize("stop", [0, 1])
@pytest.mark.parametrize("g", [1, 2])
def test_every_stream_case(eng, g, stop):
    """count, statuses, consumed and the decoded prefix of every case of the list, as the decoder of all records and as the one that stops with
    the first bad record"""
    dec = _stream_fns(eng, g)[1]
    cases = W.stream_cases(g)
    with eng.options(stream_stop_at_error=stop):
        got = [dec(np.frombuffer(c.data, np.uint8), max_points=c.max_points) for c in cases]
    for c, (out, st, used) in zip(cases, got):
        count, statuses, consumed, points = c.stop if stop else c.default
        assert (out.shape[0], st.tolist(), used) == (count, statuses, consumed), (c.name, stop, out.shape[0], st.tolist(), used)
        assert out.tobytes() == b"".join(W.words(g, p).tobytes() for p in points), (c.name, stop)
    assert any(c.stop != c.default for c in cases) and sum(c.default[0] == 0 for c in cases) >= 4


def _forty(g):
    """40 points with infinities at both ends and two neighbours in the middle, as Jacobian inputs -> (uint64 words, the model's points)"""
    P, _, _ = W.encode_batch(g, 40, start=2)                 # start = 2: the first point is an infinity, and every sixth after it
    pts = [W.normalize(g, _coords(g, row)) for row in P]
    assert pts[0] is None
    P[39] = W.words(g, None); pts[39] = None
    P[19] = P[18]; pts[19] = pts[18]
    return P, pts


def _coords(g, row):
    """ABI words -> the model's Jacobian coordinates"""
    vals = [sum(int(x) << (64 * j) for j, x in enumerate(row[4 * i:4 * i + 4])) * pow(W.MONT, -1, W.Q) % W.Q for i in range(len(row) // 4)]
    return tuple(vals) if g == 1 else ((vals[0], vals[1]), (vals[2], vals[3]), (vals[4], vals[5]))


@pytest.mark.parametrize("g", [1, 2])
def test_the_encoded_stream_and_its_tail(eng, g):
    """encode == the model's concatenation; the stream minus 5 bytes stops on the boundary in front of the cut record"""
    enc, dec = _stream_fns(eng, g)
    rs = W.RS[g]
    P, pts = _forty(g)
    got = enc(P)
    want = W.stream_encode(g, pts)
    assert got.tobytes() == want and got[0] == 0 and got[-1] == 0
    out, st, used = dec(got)
    assert used == len(want) and out.shape[0] == 40 and not st.any() and out.tobytes() == b"".join(W.words(g, p).tobytes() for p in pts)
    # a list that ends with a finite point: five bytes less is one record less; the list above ends with an infinity, so five bytes less
    # take that infinity and the finite record in front of it
    finite = enc(P[:39])
    for data, n_want, used_want in ((finite[:-5], 38, finite.size - rs), (got[:-5], 38, got.size - 1 - rs)):
        out, st, used = dec(data)
        count, statuses, consumed, points = W.stream_decode(g, data.tobytes())
        assert (out.shape[0], used) == (n_want, used_want) == (count, consumed) and not st.any()
        assert out.tobytes() == b"".join(W.words(g, p).tobytes() for p in points)
        assert data[used] == 4                                              # `consumed` sits on the tag of the cut record


@pytest.mark.parametrize("g", [1, 2])
def test_encode_stream_cap_exact_and_one_byte_short(eng, g):
    """what include/bn254_hip.h says of `cap`: the length of the stream is enough; one byte less is BN254_E_BAD_ARG, `*written` is left as it was
    and `out` holds the leading whole records that fit - nothing behind them is written"""
    fn = getattr(eng._lib, f"bn254_g{g}_encode_stream")
    P, pts = _forty(g)
    P, pts = P[:8], pts[:8]
    want = W.stream_encode(g, pts)
    need = len(want)
    out = np.full(need + 64, 0xa5, np.uint8); w = C.c_size_t(12345)
    assert fn(eng._h, _p(P), 8, _p(out), need, C.byref(w)) == 0
    assert w.value == need and out[:need].tobytes() == want and (out[need:] == 0xa5).all()
    for last, pts_l in ((8, pts), (7, pts[:7])):             # the list ends with a finite record (8) / with an infinity (7: pts[6] is None)
        want_l = W.stream_encode(g, pts_l)
        fits = len(W.stream_encode(g, pts_l[:-1]))           # the records in front of the last one still fit
        out = np.full(len(want_l) + 64, 0xa5, np.uint8); w = C.c_size_t(12345)
        assert fn(eng._h, _p(P), last, _p(out), len(want_l) - 1, C.byref(w)) == BAD_ARG
        assert w.value == 12345
        assert out[:fits].tobytes() == want_l[:fits] and (out[fits:] == 0xa5).all()
    assert pts[6] is None and pts[7] is not None
    out = np.full(8, 0xa5, np.uint8); w = C.c_size_t(12345)
    assert fn(eng._h, _p(P), 8, _p(out), 0, C.byref(w)) == BAD_ARG and w.value == 12345 and (out == 0xa5).all()          # cap 0: nothing at all
