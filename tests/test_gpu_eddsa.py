"""EdDSA-Poseidon on an MI355X (run with -m gpu): bn254_eddsa_poseidon_challenge_batch, bn254_eddsa_poseidon_verify_batch and their _dev twins
against the integer model of tests/babyjub_cases.py - the published Poseidon5 answers and circomlibjs' signature, 200 model-signed signatures,
one row of every failing class among valid ones, the seam between sub-launches, the package's sign / verify round trip, and two host threads on
streams of their own."""
import ctypes as C

import numpy as np
import pytest

import babyjub_cases as BC
import fr_cases as FC
from test_gpu_babyjub import dev_call

pytestmark = pytest.mark.gpu
KAT = (BC.KAT_A, BC.KAT_R8, BC.KAT_S, BC.KAT_M)


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
    """(rows, statuses): 130 rows - the known answer, every failing class spread among valid model-signed signatures"""
    valid = list(BC.signatures(200, 21))
    rows = [KAT] + valid[:129]
    want = [0] * 130
    for j, (_, row, st) in enumerate(BC.failing_rows()):
        rows[3 + 9 * j] = row; want[3 + 9 * j] = st                  # 13 classes at 3, 12, .. 111: on both sides of the seam at 64
    assert set(want) == {0, 1, 4, 6} and sum(1 for w in want if w) == 9
    return rows, np.array(want, np.int32)


def _verify_both(eng, rows, stream=None):
    A, R8, S, M = BC.signature_arrays(rows)
    host = eng.eddsa_poseidon_verify_batch(A, R8, S, M)
    dev = dev_call(eng.eddsa_poseidon_verify_batch_dev, [A, R8, S, M], np.full(len(rows), -7, np.int32), stream)
    assert host.dtype == np.int32
    return host, dev


@pytest.fixture(scope="module")
def challenges():
    """(A, R8, M, the model's challenges): the published inputs, the edge elements and 63 random rows"""
    ins = list(BC.KNOWN_POSEIDON5) + [(BC.R - 1,) * 5, (0,) * 5] + [tuple(FC.rand(np.random.default_rng(i)) for _ in range(5)) for i in range(63)]
    A = BC.point_rows([(i[2], i[3]) for i in ins]); R8 = BC.point_rows([(i[0], i[1]) for i in ins]); M = FC.rows([i[4] for i in ins])
    return A, R8, M, FC.rows([BC.KNOWN_POSEIDON5.get(i) or BC.poseidon5(i) for i in ins])


def test_the_challenge_gives_the_published_answers(eng, challenges):
    A, R8, M, want = challenges
    assert np.array_equal(eng.eddsa_poseidon_challenge_batch(A, R8, M), want)
    assert np.array_equal(dev_call(eng.eddsa_poseidon_challenge_batch_dev, [A, R8, M], np.zeros_like(M)), want)
    assert np.array_equal(eng.eddsa_poseidon_challenge_batch(A[:1], R8[:1], M[:1]), want[:1])


def test_the_circomlibjs_vector_verifies(eng):
    host, dev = _verify_both(eng, [KAT])
    assert host.tolist() == [0] and dev.tolist() == [0]


def test_200_model_signed_signatures_are_valid(eng):
    sigs = BC.signatures(200, 21)
    assert sigs[0][3] == 0 and sigs[1][3] == BC.R - 1 and sigs[2][2] == BC.L - 1 and sigs[3][2] == 0
    host, dev = _verify_both(eng, list(sigs))
    assert not host.any() and not dev.any()


def test_every_failing_class_among_valid_rows(eng, mixed):
    rows, want = mixed
    host, dev = _verify_both(eng, rows)
    assert np.array_equal(host, want), np.flatnonzero(host != want)
    assert np.array_equal(dev, want), np.flatnonzero(dev != want)


def test_the_same_batch_through_the_seam_and_on_a_stream(eng, lib, mixed, challenges):
    import torch
    rows, want = mixed
    A, R8, M, ch_want = (x[:5] for x in challenges)
    try:
        assert lib.bn254_bjj_set_launch_max(64) == 0
        host, dev = _verify_both(eng, rows, torch.cuda.Stream())
        assert lib.bn254_bjj_set_launch_max(2) == 0                # 5 records: 2, 2 and 1 - an odd count, where a wrong staging offset or `lo` shows
        host5, dev5 = _verify_both(eng, rows[10:15])
        ch_host, ch_dev = eng.eddsa_poseidon_challenge_batch(A, R8, M), dev_call(eng.eddsa_poseidon_challenge_batch_dev, [A, R8, M], np.zeros_like(M))
    finally:
        assert lib.bn254_bjj_set_launch_max(0) == 0
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert want[10:15].tolist() == [0, 0, 6, 0, 0] and np.array_equal(host5, want[10:15]) and np.array_equal(dev5, want[10:15])
    assert np.array_equal(ch_host, ch_want) and np.array_equal(ch_dev, ch_want)


def test_sign_then_verify_and_the_host_verifier(eng):
    from bn_amd import babyjub as BJ, eddsa
    secrets = [5, BC.L - 1, 0x1234567890abcdef1234567890abcdef, 1]
    msgs = [0, BC.R - 1, 42, BC.KAT_M]
    pks = eddsa.public_keys(secrets)
    assert pks == [BJ.Point(*BC.mul(BC.B8, s)) for s in secrets]
    sigs = eddsa.sign_batch(secrets, msgs)
    assert eddsa.verify_batch(pks, msgs, sigs) == [True] * 4
    assert [BC.verify_status((p.x, p.y), (r8.x, r8.y), s, m) for p, m, (r8, s) in zip(pks, msgs, sigs)] == [0] * 4            # the model accepts them
    assert sigs[2] == eddsa.sign(secrets[2], msgs[2]) and eddsa.verify(pks[2], msgs[2], sigs[2])
    rho = 987654321
    a, r8, s = BC.sign(secrets[0], msgs[2], rho)                                                                                # a given nonce: the model's signature
    assert eddsa.sign(secrets[0], msgs[2], nonce=rho) == (BJ.Point(*r8), s)
    wrong = [sigs[1], sigs[0], (sigs[2][0], (sigs[2][1] + 1) % BC.L), (sigs[3][0], sigs[3][1] + BC.L)]
    cases = list(zip(pks, msgs, sigs)) + list(zip(pks, msgs, wrong)) + [(BJ.Point(*BC.KAT_A), BC.KAT_M, (BJ.Point(*BC.KAT_R8), BC.KAT_S))]
    got = eddsa.verify_status_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    want = [eddsa.verify_status_host(*c) for c in cases]
    assert got.tolist() == want == [0] * 4 + [6, 6, 6, 1] + [0]
    assert [eddsa.verify_host(*c) for c in cases] == [w == 0 for w in want]


def test_two_host_threads_on_streams_of_their_own(eng, mixed):
    """the threading contract of the _dev forms: nothing shared but the context, each thread's statuses are its own batch's"""
    import torch
    from test_gpu_threading import _run_threads
    rows, want = mixed
    batches = [(rows[:70], want[:70]), (rows[60:], want[60:])]
    ch = list(BC.KNOWN_POSEIDON5)
    A = BC.point_rows([(i[2], i[3]) for i in ch]); R8 = BC.point_rows([(i[0], i[1]) for i in ch]); M = FC.rows([i[4] for i in ch])
    ch_want = FC.rows([BC.KNOWN_POSEIDON5[i] for i in ch])
    jobs = []
    for j, (r, w) in enumerate(batches):
        arrays = BC.signature_arrays(r)
        stream = torch.cuda.Stream()

        def fn(arrays=arrays, stream=stream, n=len(r)):
            st = dev_call(eng.eddsa_poseidon_verify_batch_dev, list(arrays), np.full(n, -7, np.int32), stream)
            hm = dev_call(eng.eddsa_poseidon_challenge_batch_dev, [A, R8, M], np.zeros_like(M), stream)
            return st, hm
        jobs.append(("thread %d" % j, fn, (w, ch_want)))
    _run_threads(jobs, 2, 120)
