"""Hash-to-curve for G1 on an MI355X (run with -m gpu): bn254_g1_map_to_curve_batch, bn254_g1_hash_to_curve_uniform_batch,
bn254_g1_hash_to_curve_batch and their _dev twins against the integer model of hash_cases.py - every case, the sizes around a wave, the seam
between sub-launches, every padding seam of SHA-256 - against the existing group calls, and through the wire format's on-curve check."""
import ctypes as C
import threading

import numpy as np
import pytest

import hash_cases as HC

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_hash_set_launch_max.argtypes = [C.c_size_t]
    return l


def _dev(fn, rows, stream=None, **kw):
    """a _dev form: records up, points stay on the device until the call is over"""
    import torch
    n = rows.shape[0]
    flat = np.ascontiguousarray(rows, np.uint8).reshape(-1)
    d_in = torch.from_numpy(flat.copy() if flat.size else np.zeros(1, np.uint8)).to("cuda:0")
    d_out = torch.full((n * 12,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    if stream is None:
        fn(d_in.data_ptr(), d_out.data_ptr(), n, **kw)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            fn(d_in.data_ptr(), d_out.data_ptr(), n, stream=stream.cuda_stream, **kw)
        stream.synchronize()
    return d_out.cpu().numpy().view(np.uint64).reshape(n, 12)


def _dev_map(eng, u, stream=None):
    return _dev(eng.g1_map_to_curve_batch_dev, u, stream)


def _dev_uniform(eng, b, stream=None):
    return _dev(eng.g1_hash_to_curve_uniform_batch_dev, b, stream)


def _dev_msgs(eng, msgs, dst, stream=None):
    fn = lambda d_in, d_out, n, stream=0: eng.g1_hash_to_curve_batch_dev(d_in, msgs.shape[1], dst, d_out, n, stream=stream)
    return _dev(fn, msgs, stream)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint64 and got.tobytes() == want.tobytes(), (what, np.flatnonzero((got != want).any(axis=1))[:8])


def _on_curve(eng, pts):
    """independent of the model: the wire format's decoder checks y^2 = x^3 + 3 on what its encoder wrote"""
    back, st = eng.g1_decode_batch(eng.g1_encode_batch(pts))
    assert not st.any() and back.tobytes() == pts.tobytes()


def test_every_map_case_through_both_forms(eng):
    n = len(HC.u_cases())
    u, want = HC.map_batch(n)
    got = eng.g1_map_to_curve_batch(u)
    _same(got, want, "host buffers"); _same(_dev_map(eng, u), want, "_dev")
    _on_curve(eng, got)
    assert (got[:, 8:] == want[0, 8:]).all()                                     # z == 1 everywhere: never the point at infinity


def test_every_uniform_case_through_both_forms(eng):
    n = len(HC.uniform_cases())
    b, want = HC.uniform_batch(n)
    got = eng.g1_hash_to_curve_uniform_batch(b)
    _same(got, want, "host buffers"); _same(_dev_uniform(eng, b), want, "_dev")
    _on_curve(eng, got)
    names = [c[0] for c in HC.uniform_cases()]
    zero = HC.words(None)
    assert [nm for nm, r in zip(names, got) if (r == zero).all()] == ["cancel", "cancel-small"]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_wave(eng, n):
    u, want = HC.map_batch(n, start=n)
    _same(eng.g1_map_to_curve_batch(u), want, ("map", n))
    b, want = HC.uniform_batch(n, start=n)
    _same(eng.g1_hash_to_curve_uniform_batch(b), want, ("uniform", n))
    msgs = HC.messages(n, 32, seed=n)
    got = eng.g1_hash_to_curve_batch(msgs, HC.BLS_DST)
    _same(got, eng.g1_hash_to_curve_uniform_batch(_expanded(msgs, HC.BLS_DST)), ("messages", n))
    _on_curve(eng, got)


def _expanded(msgs, dst):
    rows = [np.frombuffer(HC.expand_message_xmd(m.tobytes(), dst, HC.UNIFORM), np.uint8) for m in msgs]
    return np.stack(rows)


def test_the_seam_between_sub_launches(eng, lib):
    u, want_u = HC.map_batch(150, start=7)                                       # sub-launches of 64, 64 and 22 records
    b, want_b = HC.uniform_batch(150, start=5)
    msgs = HC.messages(150, 9, seed=1)
    exp = _expanded(msgs, b"seam")
    try:
        assert lib.bn254_hash_set_launch_max(64) == 0
        got = (eng.g1_map_to_curve_batch(u), _dev_map(eng, u), eng.g1_hash_to_curve_uniform_batch(b), _dev_uniform(eng, b),
               eng.g1_hash_to_curve_batch(msgs, b"seam"), _dev_msgs(eng, msgs, b"seam"))
    finally:
        assert lib.bn254_hash_set_launch_max(0) == 0
    _same(got[0], want_u, "map"); _same(got[1], want_u, "map _dev")
    _same(got[2], want_b, "uniform"); _same(got[3], want_b, "uniform _dev")
    want_m = eng.g1_hash_to_curve_uniform_batch(exp)
    _same(got[4], want_m, "messages"); _same(got[5], want_m, "messages _dev")
    _same(want_m[:4], np.stack([HC.words(HC.hash_uniform(r.tobytes())) for r in exp[:4]]), "model")
    for pts in got:
        _on_curve(eng, pts)


def test_the_uniform_call_equals_the_existing_group_calls(eng):
    rng = np.random.default_rng(2210)
    b = np.concatenate([rng.integers(0, 256, (120, 96), dtype=np.uint8), HC.uniform_batch(len(HC.uniform_cases()))[0]])
    p0 = eng.g1_map_to_curve_batch(b[:, :48]); p1 = eng.g1_map_to_curve_batch(b[:, 48:])
    want = eng.g1_normalize(eng.g1_add_batch(p0, p1))
    got = eng.g1_hash_to_curve_uniform_batch(b)
    _same(got, want, "map + map")
    _on_curve(eng, got); _on_curve(eng, p0)


def test_the_message_call_equals_the_uniform_call_on_the_hashlib_expansion(eng):
    """every message length around the padding seams of b_0 and every DST length around those of b_i, through both forms"""
    cases = HC.message_cases()
    assert {len(c[0]) for c in cases} == set(HC.DST_LENS) and {c[1].shape[1] for c in cases} >= {0, 1, 32}
    for dst, msgs, uniform, points in cases:
        what = (len(dst), msgs.shape[1])
        got = eng.g1_hash_to_curve_batch(msgs, dst)
        _same(got, points, what)
        _same(got, eng.g1_hash_to_curve_uniform_batch(uniform), what)
        _same(_dev_msgs(eng, msgs, dst), points, what + ("_dev",))
    _on_curve(eng, np.concatenate([c[3] for c in cases]))


def test_the_dev_forms_on_a_stream_of_their_own(eng):
    import torch
    stream = torch.cuda.Stream()
    u, want = HC.map_batch(130, start=3)
    _same(_dev_map(eng, u, stream), want, "map on a stream")
    b, want = HC.uniform_batch(70, start=2)
    _same(_dev_uniform(eng, b, stream), want, "uniform on a stream")
    msgs = HC.messages(70, 32, seed=5)
    _same(_dev_msgs(eng, msgs, HC.BLS_DST, stream), eng.g1_hash_to_curve_uniform_batch(_expanded(msgs, HC.BLS_DST)), "messages on a stream")


def test_two_host_threads_on_one_context(eng):
    """the host-buffer calls hold the context's mutex: two threads on the one context get the model's bytes"""
    u, want_u = HC.map_batch(70, start=1)
    b, want_b = HC.uniform_batch(70, start=4)
    msgs = HC.messages(70, 32, seed=9)
    want_m = eng.g1_hash_to_curve_uniform_batch(_expanded(msgs, b"threads"))
    errors = []

    def work(order):
        try:
            for _ in range(3):
                for which in order:
                    if which == 0: _same(eng.g1_map_to_curve_batch(u), want_u, "map")
                    if which == 1: _same(eng.g1_hash_to_curve_uniform_batch(b), want_b, "uniform")
                    if which == 2: _same(eng.g1_hash_to_curve_batch(msgs, b"threads"), want_m, "messages")
        except BaseException as e:                                                # reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(o,)) for o in ((0, 1, 2), (2, 1, 0))]
    for t in threads: t.start()
    for t in threads: t.join(120)
    assert not any(t.is_alive() for t in threads) and not errors, errors


def test_an_empty_batch_and_the_error_paths(eng):
    from bn_amd import _native
    assert eng.g1_map_to_curve_batch(np.zeros((0, 48), np.uint8)).shape == (0, 12)
    assert eng.g1_hash_to_curve_uniform_batch(np.zeros((0, 96), np.uint8)).shape == (0, 12)
    assert eng.g1_hash_to_curve_batch(np.zeros((0, 32), np.uint8), b"tag").shape == (0, 12)
    empty = eng.g1_hash_to_curve_batch(np.zeros((3, 0), np.uint8), b"tag")       # three empty messages: msgs is NULL
    _same(empty, np.stack([HC.words(HC.hash_to_curve(b"", b"tag"))] * 3), "empty messages")
    for dst in (b"", b"x" * 256):
        with pytest.raises(ValueError, match="1 .. 255 bytes"):
            eng.g1_hash_to_curve_batch(np.zeros((1, 4), np.uint8), dst)
    lib = _native.lib()
    out = np.zeros((1, 12), np.uint64); m = np.zeros((1, 4), np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.bn254_g1_hash_to_curve_batch(eng._h, p(m), 4, b"", 0, p(out), 1) == -2
    assert lib.bn254_g1_hash_to_curve_batch(eng._h, p(m), 4, b"x" * 256, 256, p(out), 1) == -2
    assert lib.bn254_g1_hash_to_curve_batch(eng._h, None, 4, b"x", 1, p(out), 1) == -2
    assert lib.bn254_g1_map_to_curve_batch(eng._h, None, p(out), 1) == -2
    assert not out.any()


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import G1
    msgs = [b"", b"a", b"abc", b"x" * 100]                                         # mixed lengths: hashlib and the uniform call
    got = bn_amd.g1_hash_to_curve_batch(msgs, b"face")
    assert all(np.array_equal(g.limbs, HC.words(HC.hash_to_curve(m, b"face"))) for g, m in zip(got, msgs))
    same = bn_amd.g1_hash_to_curve_batch([b"abcd", b"efgh"], b"face")             # one length: SHA-256 on the device
    assert all(np.array_equal(g.limbs, HC.words(HC.hash_to_curve(m, b"face"))) for g, m in zip(same, (b"abcd", b"efgh")))
    assert np.array_equal(G1.hash(b"abc", b"face").limbs, got[2].limbs)
    pts = bn_amd.g1_map_to_curve_batch([0, 2, 3])
    assert all(np.array_equal(p.limbs, HC.words(HC.map_to_curve(u))) for p, u in zip(pts, (0, 2, 3)))
