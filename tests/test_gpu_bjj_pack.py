"""bn254_bjj_pack_batch, bn254_bjj_unpack_batch and their _dev twins on an MI355X (run with -m gpu) against the integer model of
tests/bjj_pack_cases.py, byte for byte: every record of the unpack cases with its status, the packings of the edge points, the sizes around a
wave, two seams between sub-launches, a stream of its own, both forms of the square root, and the package's Point.pack / Point.unpack."""
import ctypes as C

import numpy as np
import pytest

import babyjub_cases as BC
import bjj_pack_cases as PK
from test_gpu_babyjub import dev_call

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_bjj_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_bjj_set_sqrt_form.argtypes = [C.c_int]
    return l


@pytest.fixture(scope="module")
def ref():
    """130 records (the unpack cases, then packings of curve points), their points and statuses; 130 points and their packings"""
    recs = list(PK.unpack_records())
    pts = BC.curve_points(130, 31)
    recs += [(PK.pack(p), p, 0) for p in pts[:130 - len(recs)]]
    assert len(recs) == 130
    return {"B": PK.byte_rows([b for b, _, _ in recs]), "P": BC.point_rows([p for _, p, _ in recs]), "st": np.array([st for _, _, st in recs], np.int32),
            "pts": BC.point_rows(pts), "packed": PK.byte_rows([PK.pack(p) for p in pts])}


def dev_unpack(eng, B, stream=None):
    import torch
    d_in = torch.from_numpy(B.view(np.int64).reshape(-1).copy()).to("cuda:0")
    d_out = torch.full((B.shape[0] * 8,), 0x5a5a5a5a, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((B.shape[0],), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    if stream is None:
        eng.bjj_unpack_batch_dev(d_in.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), B.shape[0])
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            eng.bjj_unpack_batch_dev(d_in.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), B.shape[0], stream=stream.cuda_stream)
        stream.synchronize()
    assert d_in.cpu().numpy().tobytes() == B.tobytes(), "the input was written"
    return d_out.cpu().numpy().view(np.uint64).reshape(-1, 2, 4), d_st.cpu().numpy()


def _check(eng, ref, n, stream=None):
    B, P, st = ref["B"][-n:], ref["P"][-n:], ref["st"][-n:]
    if n == 130:
        assert set(st.tolist()) == {0, 1, 3, 4}
    out, s = eng.bjj_unpack_batch(B)
    assert s.tolist() == st.tolist() and np.array_equal(out, P)
    out, s = dev_unpack(eng, B, stream)
    assert s.tolist() == st.tolist() and np.array_equal(out, P)
    pts, packed = ref["pts"][:n], ref["packed"][:n]
    assert np.array_equal(eng.bjj_pack_batch(pts), packed)
    got = dev_call(eng.bjj_pack_batch_dev, [pts], np.zeros((n, 4), np.uint64), stream)
    assert got.tobytes() == packed.tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_both_forms_of_both_calls_at_the_sizes_around_a_wave(eng, ref, n):
    _check(eng, ref, n)


def test_across_two_seams_on_a_stream(eng, lib, ref):
    import torch
    try:
        assert lib.bn254_bjj_set_launch_max(64) == 0
        _check(eng, ref, 130, torch.cuda.Stream())
    finally:
        assert lib.bn254_bjj_set_launch_max(0) == 0


def test_both_forms_of_the_square_root_give_the_same_bytes(eng, lib, ref):
    try:
        for form in (0, 1):
            assert lib.bn254_bjj_set_sqrt_form(form) == 0
            out, s = dev_unpack(eng, ref["B"])
            assert s.tolist() == ref["st"].tolist() and np.array_equal(out, ref["P"]), form
        assert lib.bn254_bjj_set_sqrt_form(2) == -2
    finally:
        assert lib.bn254_bjj_set_sqrt_form(-1) == 0


def test_pack_then_unpack_and_the_python_surface(eng, ref):
    from bn_amd import babyjub as BJ
    out, st = eng.bjj_unpack_batch(eng.bjj_pack_batch(ref["pts"]))
    assert not st.any() and np.array_equal(out, ref["pts"])
    ok = ref["st"] == 0
    assert np.array_equal(eng.bjj_pack_batch(eng.bjj_unpack_batch(ref["B"])[0][ok]), ref["B"][ok])          # pack(unpack(b)) == b for accepted b
    pts = [BJ.Point(*p) for p in (BC.G, BC.B8, BC.O, BC.neg(BC.G))]
    recs = BJ.pack_batch(pts)
    assert recs == [PK.pack((p.x, p.y)) for p in pts] == [BJ.pack_host(p) for p in pts]
    got, st = BJ.unpack_batch(recs)
    assert got == pts and not st.any()
    assert BJ.Point.unpack(pts[0].pack()) == pts[0]
    with pytest.raises(ValueError):
        BJ.Point.unpack(b"\xff" * 32)
    got, st = BJ.unpack_batch([b"\xff" * 32, (1 | 1 << 255).to_bytes(32, "little")])
    assert st.tolist() == [1, 3] and got == [BJ.Point.identity()] * 2
    assert BJ.pack_batch([]) == [] and BJ.unpack_batch([])[0] == []
