"""bn254_fr_sqrt_batch and its _dev twin on an MI355X (run with -m gpu) against the integer model of tests/bjj_pack_cases.py, byte for byte:
every case of the square root (elements of every 2-power order, every digit of the logarithm, zero, non-residues, the neighbouring roots),
the sizes around a wave, two seams between sub-launches, in place, without ok, and Fr.sqrt()."""
import ctypes as C

import numpy as np
import pytest

import bjj_pack_cases as PK
import fr_cases as FC

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
    l.bn254_fr_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def ref():
    vals = list(PK.sqrt_values())
    assert len(vals) >= 130
    want, ok = PK.model_sqrt(vals)
    return FC.rows(vals), want, ok


def dev_sqrt(eng, A, in_place=False, with_ok=True, stream=None):
    import torch
    d_a = torch.from_numpy(A.view(np.int64).reshape(-1).copy()).to("cuda:0")
    d_out = d_a if in_place else torch.full_like(d_a, 0x5a5a5a5a)
    d_ok = torch.full((A.shape[0],), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    eng.fr_sqrt_batch_dev(d_a.data_ptr(), d_out.data_ptr(), d_ok.data_ptr() if with_ok else None, A.shape[0])
    torch.cuda.synchronize()
    if not in_place:
        assert d_a.cpu().numpy().tobytes() == A.tobytes(), "the input was written"
    return d_out.cpu().numpy().view(np.uint64).reshape(A.shape), d_ok.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_both_forms_of_the_call_at_the_sizes_around_a_wave(eng, ref, n):
    A, want, ok = (x[-n:] for x in ref) if n < 130 else (x[:130] for x in ref)       # the tail holds the random elements, the head the structured ones
    out, k = eng.fr_sqrt_batch(A)
    assert np.array_equal(out, want) and k.tolist() == (ok != 0).tolist()
    out, k = dev_sqrt(eng, A)
    assert np.array_equal(out, want) and k.tolist() == ok.tolist()


def test_every_case_across_two_seams_in_place_and_without_ok(eng, lib, ref):
    A, want, ok = ref
    assert set(ok.tolist()) == {0, 1}
    try:
        assert lib.bn254_fr_set_launch_max(64) == 0
        out, k = eng.fr_sqrt_batch(A[:130])
        assert np.array_equal(out, want[:130]) and k.tolist() == (ok[:130] != 0).tolist()
        out, k = dev_sqrt(eng, A[:130], in_place=True)
        assert np.array_equal(out, want[:130]) and k.tolist() == ok[:130].tolist()
    finally:
        assert lib.bn254_fr_set_launch_max(0) == 0
    out, k = dev_sqrt(eng, A, with_ok=False)
    assert np.array_equal(out, want) and set(k.tolist()) == {-7}
    out, k = dev_sqrt(eng, A, in_place=True)
    assert np.array_equal(out, want) and k.tolist() == ok.tolist()


def test_the_python_surface(eng):
    import bn_amd
    from bn_amd import Fr
    vals = [0, 1, 4, 5, PK.HALF * PK.HALF % PK.R, PK.R - 1]
    got = bn_amd.fr_sqrt_batch([Fr(v) for v in vals])
    assert [None if g is None else g.v for g in got] == [PK.sqrt(v) for v in vals] == [0, 1, 2, None, PK.HALF, PK.sqrt(PK.R - 1)]
    assert Fr(9).sqrt() == Fr(3) and Fr(5).sqrt() is None and bn_amd.fr_sqrt_batch([]) == []
