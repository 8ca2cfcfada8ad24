"""bn254_eddsa_poseidon_verify_packed_batch and its _dev twin on an MI355X (run with -m gpu) against the integer model of
tests/bjj_pack_cases.py: the packed known answer, packed model-signed signatures, every status in its precedence among valid rows, the sizes
around a wave, two seams between sub-launches, agreement with the unpacked verifier, and the package's packed sign / verify round trip."""
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
    return l


@pytest.fixture(scope="module")
def mixed():
    """130 rows (a32, sig64, m) and their statuses: valid model-signed signatures with every row of packed_signature_rows() spread among them"""
    rows = [(PK.pack(a), PK.pack_signature(r8, s), m) for a, r8, s, m in BC.signatures(130, 21)]
    want = [0] * 130
    special = PK.packed_signature_rows()
    assert len(special) <= 43
    for j, r in enumerate(special):
        rows[3 * j] = r[1:4]; want[3 * j] = r[4]                                 # at 0, 3, .. : on both sides of the seams at 64 and 128
    rows[129] = special[-2][1:4]; want[129] = special[-2][4]
    assert set(want) == {0, 1, 3, 4, 6}
    A32, SIG, M = PK.byte_rows([r[0] for r in rows]), PK.byte_rows([r[1] for r in rows]), BC.raw_rows([r[2] for r in rows])
    return A32, SIG, M, np.array(want, np.int32)


def _both(eng, A32, SIG, M, stream=None):
    host = eng.eddsa_poseidon_verify_packed_batch(A32, SIG, M)
    dev = dev_call(eng.eddsa_poseidon_verify_packed_batch_dev, [A32, SIG, M], np.full(M.shape[0], -7, np.int32), stream)
    assert host.dtype == np.int32
    return host, dev


@pytest.mark.parametrize("n", SIZES)
def test_every_status_among_valid_rows_at_the_sizes_around_a_wave(eng, mixed, n):
    A32, SIG, M, want = (x[:n] for x in mixed)
    host, dev = _both(eng, A32, SIG, M)
    assert np.array_equal(host, want), np.flatnonzero(host != want)
    assert np.array_equal(dev, want), np.flatnonzero(dev != want)


def test_the_same_batch_across_two_seams_on_a_stream(eng, lib, mixed):
    import torch
    A32, SIG, M, want = mixed
    try:
        assert lib.bn254_bjj_set_launch_max(64) == 0
        host, dev = _both(eng, A32, SIG, M, torch.cuda.Stream())
        assert lib.bn254_bjj_set_launch_max(2) == 0                # 5 records: 2, 2 and 1 - an odd count, where a wrong staging offset or `lo` shows
        host5, dev5 = _both(eng, A32[26:31], SIG[26:31], M[26:31])
    finally:
        assert lib.bn254_bjj_set_launch_max(0) == 0
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert want[26:31].tolist() == [0, 6, 0, 0, 1] and np.array_equal(host5, want[26:31]) and np.array_equal(dev5, want[26:31])


def test_it_agrees_with_the_unpacked_verifier_where_the_points_unpack(eng, mixed):
    A32, SIG, M, want = mixed
    keep = np.flatnonzero((want == 0) | (want == 6))
    assert set(want[keep].tolist()) == {0, 6}
    A, sa = eng.bjj_unpack_batch(A32[keep]); R8, sr = eng.bjj_unpack_batch(np.ascontiguousarray(SIG[keep, :32]))
    assert not sa.any() and not sr.any()
    S = BC.raw_rows([int.from_bytes(SIG[i, 32:].tobytes(), "little") for i in keep])
    assert np.array_equal(eng.eddsa_poseidon_verify_batch(A, R8, S, M[keep]), want[keep])


def test_packed_sign_then_verify(eng):
    from bn_amd import babyjub as BJ, eddsa
    secrets = [5, BC.L - 1, 0x1234567890abcdef1234567890abcdef, 1]
    msgs = [0, BC.R - 1, 42, BC.KAT_M]
    pks = BJ.pack_batch(eddsa.public_keys(secrets))
    sigs = eddsa.sign_batch(secrets, msgs, packed=True)
    assert all(len(s) == 64 for s in sigs) and sigs == [eddsa.pack_signature(s) for s in eddsa.sign_batch(secrets, msgs)]
    assert eddsa.verify_packed_batch(pks, msgs, sigs) == [True] * 4
    assert eddsa.sign(secrets[2], msgs[2], packed=True) == sigs[2] and eddsa.verify_packed(pks[2], msgs[2], sigs[2])
    kat = (PK.pack(BC.KAT_A), BC.KAT_M, PK.pack_signature(BC.KAT_R8, BC.KAT_S))
    wrong = [sigs[1], sigs[0], sigs[2][:32] + ((int.from_bytes(sigs[2][32:], "little") + 1) % BC.L).to_bytes(32, "little"), sigs[3][:32] + b"\xff" * 32]
    cases = list(zip(pks, msgs, sigs)) + list(zip(pks, msgs, wrong)) + [kat]
    got = eddsa.verify_packed_status_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    want = [eddsa.verify_packed_status_host(*c) for c in cases]
    assert got.tolist() == want == [0] * 4 + [6, 6, 6, 1] + [0]
    assert eddsa.verify_packed_status_batch([], [], []).tolist() == []
