"""Baby Jubjub on an MI355X (run with -m gpu): bn254_bjj_validate_batch, bn254_bjj_add_batch, bn254_bjj_mul_batch and their _dev twins against the
integer model of tests/babyjub_cases.py, byte for byte - the edge points and scalars, the sizes around a wave and a workgroup, the seam between
sub-launches, in place, a stream of its own - and the group facts on the device itself."""
import ctypes as C

import numpy as np
import pytest

import babyjub_cases as BC
import fr_cases as FC

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
    l.bn254_bjj_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def ref():
    """the model's answers, computed once: 257 points of the curve (the edge points first), 257 scalars (the edge scalars first), their products,
    the sums of neighbours and the validation cases"""
    pts = BC.curve_points(257, 11)
    ks = BC.scalars(257, 12)
    qs = pts[1:] + pts[:1]
    vp, vs = BC.validate_cases()
    return {"P": BC.point_rows(pts), "K": FC.rows(ks), "Q": BC.point_rows(qs), "mul": BC.point_rows([BC.mul(p, k) for p, k in zip(pts, ks)]),
            "add": BC.point_rows([BC.add(p, q) for p, q in zip(pts, qs)]), "vp": BC.point_rows(vp), "vs": np.array(vs, np.int32), "pts": pts}


def dev_call(fn, ins, out, stream=None, out_is=None):
    """a _dev form on torch buffers: inputs up, the output (or, out_is = j, input j itself) back; the other inputs must come back unchanged"""
    import torch
    d_in = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).to("cuda:0") for a in ins]
    d_out = d_in[out_is] if out_is is not None else torch.from_numpy(out.view(np.int32 if out.dtype == np.int32 else np.int64).reshape(-1).copy()).to("cuda:0")
    n = ins[0].shape[0]
    torch.cuda.synchronize()
    if stream is None:
        fn(*[d.data_ptr() for d in d_in], d_out.data_ptr(), n)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            fn(*[d.data_ptr() for d in d_in], d_out.data_ptr(), n, stream=stream.cuda_stream)
        stream.synchronize()
    for j, (d, a) in enumerate(zip(d_in, ins)):
        if j != out_is:
            assert d.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "input %d was written" % j
    got = d_out.cpu().numpy()
    return got if out.dtype == np.int32 else got.view(np.uint64).reshape(out.shape)


def _all_forms(eng, ref, n, stream=None):
    P, K, Q = ref["P"][:n], ref["K"][:n], ref["Q"][:n]
    reps = -(-n // len(ref["vs"]))                                   # the validation cases, repeated up to n records
    V = np.concatenate([ref["vp"]] * reps)[:n]; vs = np.concatenate([ref["vs"]] * reps)[:n]
    st = np.full(n, -7, np.int32)
    return {
        "validate": (eng.bjj_validate_batch(V), dev_call(eng.bjj_validate_batch_dev, [V], st, stream), vs),
        "add": (eng.bjj_add_batch(P, Q), dev_call(eng.bjj_add_batch_dev, [P, Q], np.zeros_like(P), stream), ref["add"][:n]),
        "mul": (eng.bjj_mul_batch(P, K), dev_call(eng.bjj_mul_batch_dev, [P, K], np.zeros_like(P), stream), ref["mul"][:n]),
    }


def _check(forms, what):
    for name, (host, dev, want) in forms.items():
        assert host.shape == want.shape and np.array_equal(host, want), (what, name, "host buffers", np.flatnonzero((host != want).reshape(len(want), -1).any(axis=1))[:8])
        assert dev.shape == want.shape and np.array_equal(dev, want), (what, name, "_dev", np.flatnonzero((dev != want).reshape(len(want), -1).any(axis=1))[:8])


def test_the_validation_cases_cover_every_status(eng, ref):
    assert set(ref["vs"].tolist()) == {0, 1, 4, 5}
    keep = ref["vp"].copy()
    got = eng.bjj_validate_batch(ref["vp"])
    assert got.dtype == np.int32 and np.array_equal(got, ref["vs"]) and np.array_equal(ref["vp"], keep)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_wave_and_a_workgroup(eng, ref, n):
    _check(_all_forms(eng, ref, n), n)


def test_the_seam_between_sub_launches(eng, lib, ref):
    try:
        assert lib.bn254_bjj_set_launch_max(64) == 0               # 130 records: sub-launches of 64, 64 and 2
        forms = _all_forms(eng, ref, 130)
        assert lib.bn254_bjj_set_launch_max(2) == 0                # 5 records: 2, 2 and 1 - an odd count, where a wrong staging offset or `lo` shows
        odd = _all_forms(eng, ref, 5)
    finally:
        assert lib.bn254_bjj_set_launch_max(0) == 0
    _check(forms, "seam")
    _check(odd, "seam, 5 records in sub-launches of 2")


def test_in_place(eng, ref):
    n = 65
    P, K, Q = ref["P"][:n], ref["K"][:n], ref["Q"][:n]
    assert np.array_equal(dev_call(eng.bjj_add_batch_dev, [P, Q], np.zeros_like(P), out_is=0), ref["add"][:n])            # out is p
    assert np.array_equal(dev_call(eng.bjj_add_batch_dev, [P, Q], np.zeros_like(P), out_is=1), ref["add"][:n])            # out is q
    assert np.array_equal(dev_call(eng.bjj_mul_batch_dev, [P, K], np.zeros_like(P), out_is=0), ref["mul"][:n])            # out is p
    lib = eng._lib
    p = lambda a: C.c_void_p(a.ctypes.data)
    buf = P.copy()
    assert lib.bn254_bjj_add_batch(eng._h, p(buf), p(Q), p(buf), n) == 0 and np.array_equal(buf, ref["add"][:n])
    buf = P.copy()
    assert lib.bn254_bjj_mul_batch(eng._h, p(buf), p(K), p(buf), n) == 0 and np.array_equal(buf, ref["mul"][:n])


def test_the_dev_forms_on_a_stream_of_their_own(eng, ref):
    import torch
    _check(_all_forms(eng, ref, 70, torch.cuda.Stream()), "on a stream")


def test_the_group_order_kills_every_edge_point(eng):
    """8 l is above r, so as a scalar it is [8]([l]P); and [l]P is O exactly for the points validation accepts"""
    pts = [p for _, p in BC.edge_points()]
    P = BC.point_rows(pts)
    lP = eng.bjj_mul_batch(P, FC.rows([BC.L] * len(pts)))
    assert np.array_equal(eng.bjj_mul_batch(lP, FC.rows([8] * len(pts))), BC.point_rows([BC.O] * len(pts)))
    is_o = (lP == BC.point_rows([BC.O])[0]).all(axis=(1, 2))
    assert np.array_equal(is_o, eng.bjj_validate_batch(P) == 0) and is_o.any() and not is_o.all()
    # and through the residue: [8 l - r]P + [r - 1]P + P == O
    a = eng.bjj_mul_batch(P, FC.rows([BC.ORDER - BC.R] * len(pts))); b = eng.bjj_mul_batch(P, FC.rows([BC.R - 1] * len(pts)))
    assert np.array_equal(eng.bjj_add_batch(eng.bjj_add_batch(a, b), P), BC.point_rows([BC.O] * len(pts)))


def test_a_point_and_its_negative_sum_to_the_identity(eng, ref):
    neg = BC.point_rows([BC.neg(p) for p in ref["pts"][:70]])
    assert np.array_equal(eng.bjj_add_batch(ref["P"][:70], neg), BC.point_rows([BC.O] * 70))


def test_mul_agrees_with_repeated_add(eng):
    pts = [p for _, p in BC.edge_points()]
    P = BC.point_rows(pts)
    acc = BC.point_rows([BC.O] * len(pts))
    for k in range(1, 20):
        acc = eng.bjj_add_batch(acc, P)
        assert np.array_equal(eng.bjj_mul_batch(P, FC.rows([k] * len(pts))), acc), k


def test_an_empty_batch_and_the_error_paths(eng, ref):
    assert eng.bjj_validate_batch(np.zeros((0, 2, 4), np.uint64)).shape == (0,)
    assert eng.bjj_mul_batch(np.zeros((0, 2, 4), np.uint64), np.zeros((0, 4), np.uint64)).shape == (0, 2, 4)
    eng.bjj_validate_batch_dev(None, None, 0); eng.bjj_add_batch_dev(None, None, None, 0); eng.bjj_mul_batch_dev(None, None, None, 0)
    lib = eng._lib
    p = lambda a: C.c_void_p(a.ctypes.data)
    P, K = ref["P"][:1].copy(), ref["K"][:1].copy(); out = np.full((1, 2, 4), 7, np.uint64)
    assert lib.bn254_bjj_mul_batch(eng._h, None, p(K), p(out), 1) == -2 and lib.bn254_bjj_mul_batch(eng._h, p(P), None, p(out), 1) == -2
    assert lib.bn254_bjj_mul_batch(eng._h, p(P), p(K), None, 1) == -2 and lib.bn254_bjj_mul_batch_dev(eng._h, p(P), p(K), p(out), (1 << 40) + 1, None) == -2
    assert (out == 7).all()


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr, babyjub as BJ
    B = BJ.Point.base()
    assert B.is_valid() and BJ.Point.identity().is_valid() and not BJ.Point.generator().is_valid()
    assert B + B == B * 2 == BJ.Point(*BC.mul(BC.B8, 2)) and B - B == BJ.Point.identity() and B * Fr(BC.L) == BJ.Point.identity()
    assert BJ.Point.generator() * 8 == B
    ks = [Fr(5), Fr(BC.R - 1)]
    assert BJ.mul_base(ks) == [BJ.Point(*BC.mul(BC.B8, k.v)) for k in ks]
    assert bn_amd.bjj_validate_batch([BC.B8, BC.G, BC.OFF_CURVE]).tolist() == [0, 5, 4]
