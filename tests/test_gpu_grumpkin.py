"""Grumpkin on an MI355X (run with -m gpu): bn254_grumpkin_validate_batch, bn254_grumpkin_add_batch, bn254_grumpkin_mul_batch,
bn254_grumpkin_msm_batch and their _dev twins against the integer model of tests/grumpkin_cases.py, byte for byte - the edge points and scalars,
the sizes around a wave and a workgroup, the seam between sub-launches, in place, a stream of its own, the segmented sum over segments on both
sides of a fold lane - and the group facts on the device itself."""
import ctypes as C

import numpy as np
import pytest

import grumpkin_cases as GC

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257]
O_ROWS = lambda n: np.zeros((n, 2, 4), np.uint64)


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own, destroyed when the module is done: the process keeps none of its streams"""
    import bn_amd
    e = bn_amd.Engine(0)
    yield e
    e.close()


class OwnStream:
    """a HIP stream created for one test and destroyed after it (hipStreamCreate / hipStreamDestroy of the runtime the library is bound to):
    unlike a stream of torch's pool it leaves nothing behind in the process, so the tests that come later see the streams they saw before"""
    def __init__(self):
        from bn_amd import _native
        path = _native._preload_shared_hip_runtime()
        self.hip = C.CDLL(path) if path else C.CDLL("libamdhip64.so")
        self.hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.hip.hipStreamDestroy.argtypes = [C.c_void_p]
        h = C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(h)) == 0 and h.value
        self.cuda_stream = h.value

    def synchronize(self):
        assert self.hip.hipStreamSynchronize(self.cuda_stream) == 0

    def destroy(self):
        self.synchronize()
        assert self.hip.hipStreamDestroy(self.cuda_stream) == 0


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_grumpkin_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def ref():
    """the model's answers, computed once: 257 points of the curve (the edge points first), 257 scalars (the edge scalars first, then 64 random
    256-bit ones, then 64-bit ones so that the model stays quick), their products, the sums of neighbours, the validation cases and the
    segmented sum's"""
    pts = list(GC.curve_points(257, 11))
    ks = [k if i < 80 else k >> 192 for i, k in enumerate(GC.scalars(257, 12))]
    qs = pts[1:] + pts[:1]
    vp, vs = GC.validate_cases()
    mp, mk, mo, mw = GC.msm_cases()
    return {"P": GC.point_rows(pts), "K": GC.scalar_rows(ks), "Q": GC.point_rows(qs), "mul": GC.point_rows([GC.mul(p, k) for p, k in zip(pts, ks)]),
            "add": GC.point_rows([GC.add(p, q) for p, q in zip(pts, qs)]), "vp": GC.point_rows(vp), "vs": np.array(vs, np.int32), "pts": pts,
            "msm": (GC.point_rows(mp), GC.scalar_rows(mk), np.array(mo, np.uint64), GC.point_rows(mw))}


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).to("cuda:0")


def dev_call(fn, ins, out, stream=None, out_is=None):
    """a _dev form on torch buffers: inputs up, the output (or, out_is = j, input j itself) back; the other inputs must come back unchanged"""
    import torch
    d_in = [_up(a) for a in ins]
    d_out = d_in[out_is] if out_is is not None else torch.from_numpy(out.view(np.int32 if out.dtype == np.int32 else np.int64).reshape(-1).copy()).to("cuda:0")
    n = ins[0].shape[0]
    torch.cuda.synchronize()
    if stream is None:
        fn(*[d.data_ptr() for d in d_in], d_out.data_ptr(), n)
        torch.cuda.synchronize()
    else:
        fn(*[d.data_ptr() for d in d_in], d_out.data_ptr(), n, stream=stream.cuda_stream)
        stream.synchronize()
    for j, (d, a) in enumerate(zip(d_in, ins)):
        if j != out_is:
            assert d.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "input %d was written" % j
    got = d_out.cpu().numpy()
    return got if out.dtype == np.int32 else got.view(np.uint64).reshape(out.shape)


def msm_dev(eng, P, K, offs, stream=None):
    """bn254_grumpkin_msm_batch_dev on torch buffers; the output starts as a pattern and the inputs must come back unchanged"""
    import torch
    m = len(offs) - 1
    d_p, d_k = _up(P if len(P) else np.zeros((1, 2, 4), np.uint64)), _up(K if len(K) else np.zeros((1, 4), np.uint64))
    d_out = _up(np.full((m, 2, 4), 0x5a5a5a5a5a5a5a5a, np.uint64))
    torch.cuda.synchronize()
    if stream is None:
        eng.grumpkin_msm_batch_dev(d_p.data_ptr(), d_k.data_ptr(), offs, m, d_out.data_ptr())
        torch.cuda.synchronize()
    else:
        eng.grumpkin_msm_batch_dev(d_p.data_ptr(), d_k.data_ptr(), offs, m, d_out.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
    if len(P):
        assert d_p.cpu().numpy().tobytes() == np.ascontiguousarray(P).tobytes() and d_k.cpu().numpy().tobytes() == np.ascontiguousarray(K).tobytes()
    return d_out.cpu().numpy().view(np.uint64).reshape(m, 2, 4)


def _all_forms(eng, ref, n, stream=None):
    P, K, Q = ref["P"][:n], ref["K"][:n], ref["Q"][:n]
    reps = -(-n // len(ref["vs"]))                                   # the validation cases, repeated up to n records
    V = np.concatenate([ref["vp"]] * reps)[:n]; vs = np.concatenate([ref["vs"]] * reps)[:n]
    st = np.full(n, -7, np.int32)
    return {
        "validate": (eng.grumpkin_validate_batch(V), dev_call(eng.grumpkin_validate_batch_dev, [V], st, stream), vs),
        "add": (eng.grumpkin_add_batch(P, Q), dev_call(eng.grumpkin_add_batch_dev, [P, Q], np.zeros_like(P), stream), ref["add"][:n]),
        "mul": (eng.grumpkin_mul_batch(P, K), dev_call(eng.grumpkin_mul_batch_dev, [P, K], np.zeros_like(P), stream), ref["mul"][:n]),
    }


def _check(forms, what):
    for name, (host, dev, want) in forms.items():
        assert host.shape == want.shape and np.array_equal(host, want), (what, name, "host buffers", np.flatnonzero((host != want).reshape(len(want), -1).any(axis=1))[:8])
        assert dev.shape == want.shape and np.array_equal(dev, want), (what, name, "_dev", np.flatnonzero((dev != want).reshape(len(want), -1).any(axis=1))[:8])


def test_the_validation_cases_cover_every_status(eng, ref):
    assert set(ref["vs"].tolist()) == {0, 1, 4}
    keep = ref["vp"].copy()
    got = eng.grumpkin_validate_batch(ref["vp"])
    assert got.dtype == np.int32 and np.array_equal(got, ref["vs"]) and np.array_equal(ref["vp"], keep)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_wave_and_a_workgroup(eng, ref, n):
    _check(_all_forms(eng, ref, n), n)


def test_the_seam_between_sub_launches(eng, lib, ref):
    try:
        assert lib.bn254_grumpkin_set_launch_max(64) == 0               # 130 records: sub-launches of 64, 64 and 2
        forms = _all_forms(eng, ref, 130)
        assert lib.bn254_grumpkin_set_launch_max(2) == 0                # 5 records: 2, 2 and 1 - an odd count, where a wrong staging offset or `lo` shows
        odd = _all_forms(eng, ref, 5)
    finally:
        assert lib.bn254_grumpkin_set_launch_max(0) == 0
    _check(forms, "seam")
    _check(odd, "seam, 5 records in sub-launches of 2")


def test_in_place(eng, ref):
    n = 65
    P, K, Q = ref["P"][:n], ref["K"][:n], ref["Q"][:n]
    assert np.array_equal(dev_call(eng.grumpkin_add_batch_dev, [P, Q], np.zeros_like(P), out_is=0), ref["add"][:n])            # out is p
    assert np.array_equal(dev_call(eng.grumpkin_add_batch_dev, [P, Q], np.zeros_like(P), out_is=1), ref["add"][:n])            # out is q
    assert np.array_equal(dev_call(eng.grumpkin_mul_batch_dev, [P, K], np.zeros_like(P), out_is=0), ref["mul"][:n])            # out is p
    lib = eng._lib
    p = lambda a: C.c_void_p(a.ctypes.data)
    buf = P.copy()
    assert lib.bn254_grumpkin_add_batch(eng._h, p(buf), p(Q), p(buf), n) == 0 and np.array_equal(buf, ref["add"][:n])
    buf = P.copy()
    assert lib.bn254_grumpkin_mul_batch(eng._h, p(buf), p(K), p(buf), n) == 0 and np.array_equal(buf, ref["mul"][:n])


def test_the_dev_forms_on_a_stream_of_their_own(eng, ref):
    s = OwnStream()
    try:
        forms = _all_forms(eng, ref, 70, s)
        P, K, offs, want = ref["msm"]
        got = msm_dev(eng, P, K, offs, s)
    finally:
        s.destroy()
    _check(forms, "on a stream")
    assert np.array_equal(got, want)


def test_the_group_order_kills_every_edge_point(eng):
    pts = [p for _, p in GC.edge_points()]
    P = GC.point_rows(pts)
    assert np.array_equal(eng.grumpkin_mul_batch(P, GC.scalar_rows([GC.Q] * len(pts))), O_ROWS(len(pts)))               # [q]P = O
    assert np.array_equal(eng.grumpkin_mul_batch(P, GC.scalar_rows([GC.Q + 1] * len(pts))), P)                           # [q + 1]P = P
    rP = eng.grumpkin_mul_batch(P[1:], GC.scalar_rows([GC.R] * (len(pts) - 1)))
    assert rP.reshape(len(pts) - 1, -1).any(axis=1).all()                                                                  # [r]P != O: r is not the order


def test_a_point_and_its_negative_sum_to_the_identity(eng, ref):
    neg = GC.point_rows([GC.neg(p) for p in ref["pts"][:70]])
    assert np.array_equal(eng.grumpkin_add_batch(ref["P"][:70], neg), O_ROWS(70))                                         # P + (-P) = O
    assert np.array_equal(eng.grumpkin_add_batch(O_ROWS(70), ref["P"][:70]), ref["P"][:70])                               # O + P = P
    assert np.array_equal(eng.grumpkin_add_batch(ref["P"][:70], O_ROWS(70)), ref["P"][:70])


def test_mul_agrees_with_repeated_add(eng):
    pts = [p for _, p in GC.edge_points()]
    P = GC.point_rows(pts)
    acc = O_ROWS(len(pts))
    for k in range(1, 20):
        acc = eng.grumpkin_add_batch(acc, P)
        assert np.array_equal(eng.grumpkin_mul_batch(P, GC.scalar_rows([k] * len(pts))), acc), k


def test_an_empty_batch_and_the_error_paths(eng, ref):
    assert eng.grumpkin_validate_batch(np.zeros((0, 2, 4), np.uint64)).shape == (0,)
    assert eng.grumpkin_mul_batch(np.zeros((0, 2, 4), np.uint64), np.zeros((0, 4), np.uint64)).shape == (0, 2, 4)
    eng.grumpkin_validate_batch_dev(None, None, 0); eng.grumpkin_add_batch_dev(None, None, None, 0); eng.grumpkin_mul_batch_dev(None, None, None, 0)
    assert eng.grumpkin_msm_batch(np.zeros((0, 2, 4), np.uint64), np.zeros((0, 4), np.uint64), [0]).shape == (0, 2, 4)
    assert np.array_equal(eng.grumpkin_msm_batch(np.zeros((0, 2, 4), np.uint64), np.zeros((0, 4), np.uint64), [0, 0, 0]), O_ROWS(2))
    lib = eng._lib
    p = lambda a: C.c_void_p(a.ctypes.data)
    P, K = ref["P"][:2].copy(), ref["K"][:2].copy(); out = np.full((2, 2, 4), 7, np.uint64)
    assert lib.bn254_grumpkin_mul_batch(eng._h, None, p(K), p(out), 1) == -2 and lib.bn254_grumpkin_mul_batch(eng._h, p(P), None, p(out), 1) == -2
    assert lib.bn254_grumpkin_mul_batch(eng._h, p(P), p(K), None, 1) == -2 and lib.bn254_grumpkin_mul_batch_dev(eng._h, p(P), p(K), p(out), (1 << 40) + 1, None) == -2
    o12, o021, o02 = np.array([1, 2], np.uint64), np.array([0, 2, 1], np.uint64), np.array([0, 2], np.uint64)
    assert lib.bn254_grumpkin_msm_batch(eng._h, p(P), p(K), p(o12), 1, p(out)) == -2                                      # offsets[0] != 0
    assert lib.bn254_grumpkin_msm_batch(eng._h, p(P), p(K), p(o021), 2, p(out)) == -2                                     # decreasing
    assert lib.bn254_grumpkin_msm_batch(eng._h, None, p(K), p(o02), 1, p(out)) == -2 and lib.bn254_grumpkin_msm_batch(eng._h, p(P), p(K), p(o02), 1, None) == -2
    assert lib.bn254_grumpkin_msm_batch_dev(eng._h, p(P), p(K), None, 1, p(out), None) == -2
    assert (out == 7).all()


def test_the_segmented_sum(eng, ref):
    """segments of 0, 1, 2, 15, 16, 17, 256 and 257 terms, a cancelling one, one of equal points, one of O points and zero scalars, an empty
    one, in ONE call: host buffers and device buffers"""
    P, K, offs, want = ref["msm"]
    lens = np.diff(offs.astype(np.int64)).tolist()
    assert lens[:8] == [0, 1, 2, 15, 16, 17, 256, 257] and lens[-1] == 0
    keepP, keepK = P.copy(), K.copy()
    got = eng.grumpkin_msm_batch(P, K, offs)
    assert np.array_equal(got, want), np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert np.array_equal(P, keepP) and np.array_equal(K, keepK)
    assert not want[8].any() and not want[10].any()                                                                        # the cancelling segment and the one of O points
    got = msm_dev(eng, P, K, offs)
    assert np.array_equal(got, want), np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))


def test_the_segmented_sum_across_sub_launch_seams(eng, lib, ref):
    P, K, offs, want = ref["msm"]
    try:
        assert lib.bn254_grumpkin_set_launch_max(64) == 0
        host, dev = eng.grumpkin_msm_batch(P, K, offs), msm_dev(eng, P, K, offs)
    finally:
        assert lib.bn254_grumpkin_set_launch_max(0) == 0
    assert np.array_equal(host, want) and np.array_equal(dev, want)


def test_the_segmented_sum_is_mul_followed_by_a_sum(eng, ref):
    from bn_amd import Fr
    P, K, offs, want = ref["msm"]
    prods = eng.grumpkin_mul_batch(P, K)
    rows = [(Fr.from_limbs(r[0]).v, Fr.from_limbs(r[1]).v) for r in prods]
    sums = []
    for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
        acc = GC.O
        for t in range(a, b):
            acc = GC.add(acc, rows[t])
        sums.append(acc)
    assert np.array_equal(GC.point_rows(sums), eng.grumpkin_msm_batch(P, K, offs)) and np.array_equal(GC.point_rows(sums), want)


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr, grumpkin as GK
    G = GK.Point.generator()
    assert G.is_valid() and GK.Point.identity().is_valid() and not GK.Point(*GC.OFF_CURVE).is_valid()
    assert G + G == G * 2 == GK.Point(*GC.mul(GC.G, 2)) and G - G == GK.Point.identity() and G * GK.Q == GK.Point.identity()
    assert G * Fr(5) == GK.Point(*GC.mul(GC.G, 5)) and -G == GK.Point(*GC.neg(GC.G)) and G * ((1 << 256) - 1) == GK.Point(*GC.mul(GC.G, (1 << 256) - 1))
    pts, ks = [GC.G, GC.mul(GC.G, 2), GC.O], [3, GC.Q - 1, 7]
    assert GK.msm(pts, ks) == GK.Point(*GC.msm(pts, ks)) and GK.msm([], []) == GK.Point.identity()
    assert bn_amd.grumpkin_validate_batch([GC.G, GC.O, GC.OFF_CURVE]).tolist() == [0, 0, 4]
    assert bn_amd.grumpkin_msm_batch([GC.G] * 3, [1, 2, 3], [0, 1, 3]) == [G, GK.Point(*GC.mul(GC.G, 5))]
    with pytest.raises(ValueError):
        bn_amd.grumpkin_mul_batch([GC.G], [1 << 256])
