"""Hash-to-curve for G2 and cofactor clearing on an MI355X (run with -m gpu): bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch,
bn254_g2_hash_to_curve_uniform_batch, bn254_g2_hash_to_curve_batch and their _dev twins against the integer model of hash_g2_cases.py - every
case, the sizes around a wave, the seam between sub-launches, every padding seam of SHA-256 - against the existing group calls on the same
device, and through the wire format's curve and subgroup checks.  Neither side is checked against gnark-crypto or any other library."""
import ctypes as C
import threading

import numpy as np
import pytest

import hash_g2_cases as HC
from hash_cases import expand_message_xmd

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 129]
NOT_IN_SUBGROUP = 5


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_hash_g2_set_launch_max.argtypes = [C.c_size_t]
    return l


def _dev(fn, rows, stream=None, in_place=False):
    """a _dev form: records up, points stay on the device until the call is over"""
    import torch
    n = rows.shape[0]
    flat = np.ascontiguousarray(rows).reshape(-1).view(np.uint8)
    d_in = torch.from_numpy(flat.copy() if flat.size else np.zeros(1, np.uint8)).to("cuda:0")
    d_out = d_in if in_place else torch.full((n * 24,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    if stream is None:
        fn(d_in.data_ptr(), d_out.data_ptr(), n)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            fn(d_in.data_ptr(), d_out.data_ptr(), n, stream=stream.cuda_stream)
        stream.synchronize()
    return d_out.cpu().numpy().view(np.uint64).reshape(n, 24)


def _dev_map(eng, u, stream=None):
    return _dev(eng.g2_map_to_curve_batch_dev, u, stream)


def _dev_clear(eng, p, stream=None, in_place=False):
    return _dev(eng.g2_clear_cofactor_batch_dev, p, stream, in_place)


def _dev_uniform(eng, b, stream=None):
    return _dev(eng.g2_hash_to_curve_uniform_batch_dev, b, stream)


def _dev_msgs(eng, msgs, dst, stream=None):
    fn = lambda d_in, d_out, n, stream=0: eng.g2_hash_to_curve_batch_dev(d_in, msgs.shape[1], dst, d_out, n, stream=stream)
    return _dev(fn, msgs, stream)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint64 and got.tobytes() == want.tobytes(), (what, np.flatnonzero((got != want).any(axis=1))[:8])


def _in_g2(eng, pts):
    """independent of the model: the wire format's decoder checks the curve equation and the subgroup (the r - 1 chain) on what its encoder wrote"""
    back, st = eng.g2_decode_batch(eng.g2_encode_batch(pts))
    assert not st.any() and back.tobytes() == pts.tobytes()


def _on_the_twist_outside_g2(eng, pts):
    """the same decoder on mapped points: on the curve (or the status would say so) and outside the subgroup"""
    _, st = eng.g2_decode_batch(eng.g2_encode_batch(pts))
    assert (st == NOT_IN_SUBGROUP).all(), st


def _expanded(msgs, dst):
    return np.stack([np.frombuffer(expand_message_xmd(m.tobytes(), dst, HC.UNIFORM), np.uint8) for m in msgs])


def test_every_map_case_through_both_forms(eng):
    n = len(HC.u_cases())
    u, want = HC.map_batch(n)
    got = eng.g2_map_to_curve_batch(u)
    _same(got, want, "host buffers"); _same(_dev_map(eng, u), want, "_dev")
    _on_the_twist_outside_g2(eng, got)
    assert (got[:, 16:] == want[0, 16:]).all()                                   # z == 1 everywhere: never the point at infinity


def test_every_clear_case_through_both_forms_and_in_place(eng):
    n = len(HC.clear_cases())
    p, want = HC.clear_batch(n)
    got = eng.g2_clear_cofactor_batch(p)
    _same(got, want, "host buffers"); _same(_dev_clear(eng, p), want, "_dev"); _same(_dev_clear(eng, p, in_place=True), want, "_dev, out == p")
    lib_ = eng._lib
    buf = p.copy()                                                               # out == p through the host-buffer form
    assert lib_.bn254_g2_clear_cofactor_batch(eng._h, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data), n) == 0
    _same(buf, want, "host buffers, out == p")
    _in_g2(eng, got)
    zero = HC.words(None)
    assert [nm for (nm, _, _), r in zip(HC.clear_cases(), got) if (r == zero).all()] == ["zero", "z=0-xy", "all-zero"]


def test_every_uniform_case_through_both_forms(eng):
    n = len(HC.uniform_cases())
    b, want = HC.uniform_batch(n)
    got = eng.g2_hash_to_curve_uniform_batch(b)
    _same(got, want, "host buffers"); _same(_dev_uniform(eng, b), want, "_dev")
    _in_g2(eng, got)
    names = [c[0] for c in HC.uniform_cases()]
    zero = HC.words(None)
    assert [nm for nm, r in zip(names, got) if (r == zero).all()] == ["cancel", "cancel-small"]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_wave(eng, n):
    u, want = HC.map_batch(n, start=n)
    _same(eng.g2_map_to_curve_batch(u), want, ("map", n))
    p, want = HC.clear_batch(n, start=n)
    _same(eng.g2_clear_cofactor_batch(p), want, ("clear", n))
    b, want = HC.uniform_batch(n, start=n)
    _same(eng.g2_hash_to_curve_uniform_batch(b), want, ("uniform", n))
    msgs = HC.messages(n, 32, seed=n)
    got = eng.g2_hash_to_curve_batch(msgs, HC.BLS_G2_DST)
    _same(got, eng.g2_hash_to_curve_uniform_batch(_expanded(msgs, HC.BLS_G2_DST)), ("messages", n))
    _in_g2(eng, got)


def test_the_seam_between_sub_launches(eng, lib):
    u, want_u = HC.map_batch(131, start=7)                                       # sub-launches of 64, 64 and 3 records
    p, want_p = HC.clear_batch(131, start=3)
    b, want_b = HC.uniform_batch(131, start=5)
    msgs = HC.messages(131, 9, seed=1)
    exp = _expanded(msgs, b"seam")
    try:
        assert lib.bn254_hash_g2_set_launch_max(64) == 0
        got = (eng.g2_map_to_curve_batch(u), _dev_map(eng, u), eng.g2_clear_cofactor_batch(p), _dev_clear(eng, p), eng.g2_hash_to_curve_uniform_batch(b),
               _dev_uniform(eng, b), eng.g2_hash_to_curve_batch(msgs, b"seam"), _dev_msgs(eng, msgs, b"seam"))
    finally:
        assert lib.bn254_hash_g2_set_launch_max(0) == 0
    _same(got[0], want_u, "map"); _same(got[1], want_u, "map _dev")
    _same(got[2], want_p, "clear"); _same(got[3], want_p, "clear _dev")
    _same(got[4], want_b, "uniform"); _same(got[5], want_b, "uniform _dev")
    want_m = eng.g2_hash_to_curve_uniform_batch(exp)
    _same(got[6], want_m, "messages"); _same(got[7], want_m, "messages _dev")
    _same(want_m[:3], np.stack([HC.words(HC.hash_uniform(r.tobytes())) for r in exp[:3]]), "model")


def test_clearing_points_of_g2_equals_the_existing_multiplication_by_k(eng):
    from bn_amd import Fr, G2
    rng = np.random.default_rng(2310)
    ks = np.stack([Fr.random(rng).limbs for _ in range(64)])
    q = eng.g2_mul_base_batch(G2.one().limbs, ks)                                # 64 points of G2
    want = eng.g2_mul_batch(q, np.tile(Fr(HC.CLEAR_K).limbs, (64, 1)))           # GLS: valid here, the inputs are in the subgroup
    _same(eng.g2_clear_cofactor_batch(q), want, "clear(Q) = [k]Q")
    _same(want[0], HC.words(HC.clear(HC.affine_of(q[0]))), "model")


def test_the_uniform_call_equals_the_map_the_existing_addition_and_the_clearing(eng):
    rng = np.random.default_rng(2311)
    b = np.concatenate([rng.integers(0, 256, (100, 192), dtype=np.uint8), HC.uniform_batch(len(HC.uniform_cases()))[0]])
    p0 = eng.g2_map_to_curve_batch(b[:, :96]); p1 = eng.g2_map_to_curve_batch(b[:, 96:])
    want = eng.g2_clear_cofactor_batch(eng.g2_add_batch(p0, p1))
    got = eng.g2_hash_to_curve_uniform_batch(b)
    _same(got, want, "clear(map + map)")
    _in_g2(eng, got); _on_the_twist_outside_g2(eng, p0)


def test_the_message_call_equals_the_uniform_call_on_the_hashlib_expansion(eng):
    """every message length around the padding seams of b_0 and every DST length around those of b_i, through both forms"""
    cases = HC.message_cases()
    assert {len(c[0]) for c in cases} == set(HC.DST_LENS) and {c[1].shape[1] for c in cases} >= {0, 1, 32}
    for dst, msgs, uniform, points in cases:
        what = (len(dst), msgs.shape[1])
        got = eng.g2_hash_to_curve_batch(msgs, dst)
        _same(got, points, what)
        _same(_dev_msgs(eng, msgs, dst), points, what + ("_dev",))
    uni = np.concatenate([c[2] for c in cases]); pts = np.concatenate([c[3] for c in cases])
    _same(eng.g2_hash_to_curve_uniform_batch(uni), pts, "uniform")
    _in_g2(eng, pts)


def test_the_dev_forms_on_a_stream_of_their_own(eng):
    import torch
    stream = torch.cuda.Stream()
    u, want = HC.map_batch(70, start=3)
    _same(_dev_map(eng, u, stream), want, "map on a stream")
    p, want = HC.clear_batch(70, start=2)
    _same(_dev_clear(eng, p, stream), want, "clear on a stream")
    b, want = HC.uniform_batch(70, start=2)
    _same(_dev_uniform(eng, b, stream), want, "uniform on a stream")
    msgs = HC.messages(70, 32, seed=5)
    _same(_dev_msgs(eng, msgs, HC.BLS_G2_DST, stream), eng.g2_hash_to_curve_uniform_batch(_expanded(msgs, HC.BLS_G2_DST)), "messages on a stream")


def test_two_host_threads_on_one_context(eng):
    """the host-buffer calls hold the context's mutex: two threads on the one context get the model's bytes"""
    u, want_u = HC.map_batch(70, start=1)
    p, want_p = HC.clear_batch(70, start=1)
    b, want_b = HC.uniform_batch(70, start=4)
    msgs = HC.messages(70, 32, seed=9)
    want_m = eng.g2_hash_to_curve_uniform_batch(_expanded(msgs, b"threads"))
    errors = []

    def work(order):
        try:
            for _ in range(2):
                for which in order:
                    if which == 0: _same(eng.g2_map_to_curve_batch(u), want_u, "map")
                    if which == 1: _same(eng.g2_hash_to_curve_uniform_batch(b), want_b, "uniform")
                    if which == 2: _same(eng.g2_hash_to_curve_batch(msgs, b"threads"), want_m, "messages")
                    if which == 3: _same(eng.g2_clear_cofactor_batch(p), want_p, "clear")
        except BaseException as e:                                                # reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(o,)) for o in ((0, 1, 2, 3), (3, 2, 1, 0))]
    for t in threads: t.start()
    for t in threads: t.join(120)
    assert not any(t.is_alive() for t in threads) and not errors, errors


def test_an_empty_batch_and_the_error_paths(eng):
    assert eng.g2_map_to_curve_batch(np.zeros((0, 96), np.uint8)).shape == (0, 24)
    assert eng.g2_clear_cofactor_batch(np.zeros((0, 24), np.uint64)).shape == (0, 24)
    assert eng.g2_hash_to_curve_uniform_batch(np.zeros((0, 192), np.uint8)).shape == (0, 24)
    assert eng.g2_hash_to_curve_batch(np.zeros((0, 32), np.uint8), b"tag").shape == (0, 24)
    empty = eng.g2_hash_to_curve_batch(np.zeros((3, 0), np.uint8), b"tag")       # three empty messages: msgs is NULL
    _same(empty, np.stack([HC.words(HC.hash_to_curve(b"", b"tag"))] * 3), "empty messages")
    for dst in (b"", b"x" * 256):
        with pytest.raises(ValueError, match="1 .. 255 bytes"):
            eng.g2_hash_to_curve_batch(np.zeros((1, 4), np.uint8), dst)
    lib = eng._lib
    out = np.zeros((1, 24), np.uint64); m = np.zeros((1, 4), np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.bn254_g2_hash_to_curve_batch(eng._h, p(m), 4, b"", 0, p(out), 1) == -2
    assert lib.bn254_g2_hash_to_curve_batch(eng._h, p(m), 4, b"x" * 256, 256, p(out), 1) == -2
    assert lib.bn254_g2_hash_to_curve_batch(eng._h, None, 4, b"x", 1, p(out), 1) == -2
    assert lib.bn254_g2_map_to_curve_batch(eng._h, None, p(out), 1) == -2
    assert lib.bn254_g2_clear_cofactor_batch(eng._h, None, p(out), 1) == -2
    assert not out.any()


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import G2
    msgs = [b"", b"a", b"abc", b"x" * 100]                                         # mixed lengths: hashlib and the uniform call
    got = bn_amd.g2_hash_to_curve_batch(msgs, b"face")
    assert all(np.array_equal(g.limbs, HC.words(HC.hash_to_curve(m, b"face"))) for g, m in zip(got, msgs))
    same = bn_amd.g2_hash_to_curve_batch([b"abcd", b"efgh"], b"face")             # one length: SHA-256 on the device
    assert all(np.array_equal(g.limbs, HC.words(HC.hash_to_curve(m, b"face"))) for g, m in zip(same, (b"abcd", b"efgh")))
    assert np.array_equal(G2.hash(b"abc", b"face").limbs, got[2].limbs)
    us = [(0, 0), (0, 1), (2, 0)]
    pts = bn_amd.g2_map_to_curve_batch(us)
    assert all(np.array_equal(p.limbs, HC.words(HC.map_to_curve(u))) for p, u in zip(pts, us))
    cl = bn_amd.g2_clear_cofactor_batch(pts)
    assert all(np.array_equal(c.limbs, HC.words(HC.clear(HC.map_to_curve(u)))) for c, u in zip(cl, us))
