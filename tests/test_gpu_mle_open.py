"""The quotients of a multilinear opening on an MI355X (run with -m gpu): bn254_fr_mle_quotients, its _dev entry point, the Python faces and
bn_amd.mle.quotients.  The model is Python integers (tests/mle_open_cases.py): the expected bytes are the limbs of v * 2^256 mod r, and they
do not depend on how the levels are cut into passes.  The sizes are the smallest that reach every seam of the plan for the shipped number
of levels per pass rho, read from the library's internal hook: no variable, fewer than one pass, whole passes, passes with a remainder
(nv = 0 .. 2 rho + 1), and nv = 13, whose first pass spans several sub-launches of 256 lanes."""
import ctypes as C
import threading

import numpy as np
import pytest

import fr_cases as FC
import mle_cases as MC
import mle_open_cases as OC

pytestmark = pytest.mark.gpu
R = FC.R


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_mle_quotients_levels.argtypes = []; l.bn254_fr_mle_quotients_levels.restype = C.c_uint
    l.bn254_fr_mle_quotients_set_levels.argtypes = [C.c_uint]
    l.bn254_fr_mle_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def rho(lib):
    return int(lib.bn254_fr_mle_quotients_levels())


@pytest.fixture(scope="module")
def cases():
    """per number of variables: (table, point, the model's heap as limbs) - computed once, never changed"""
    out = {}
    for nv in list(range(10)) + [13]:
        table, z = OC.values(1 << nv, 80 + nv), OC.point(nv, nv)
        out[nv] = (table, z, FC.rows(OC.quotients(table, z)))
    return out


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    assert got.tobytes() == want.tobytes(), np.nonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))[0][:8]


def _z(z):
    return FC.rows(z) if z else np.zeros((0, 4), np.uint64)


def _passes(nv, rho, step):
    """sub-launches of a call: every pass of the model plan cut into parts of at most `step` lanes"""
    return sum(-(-p[2] // step) for p in OC.plan(nv, rho)[0])


def test_against_the_model_for_every_size_around_the_passes(eng, rho, cases):
    for nv in OC.sizes(rho) + [13]:
        table, z, want = cases[nv]
        A = FC.rows(table)
        _same(eng.fr_mle_quotients(A, _z(z)), want)
        assert A.tobytes() == FC.rows(table).tobytes()


def test_the_same_in_sub_launches_of_256_lanes(eng, lib, rho, cases):
    """at nv = 13 the first pass has 2^(13 - rho) >= 512 lanes: it spans several sub-launches and the seam is crossed"""
    eng.profile(True)
    assert lib.bn254_fr_mle_set_launch_max(256) == 0
    try:
        for nv in OC.sizes(rho) + [13]:
            table, z, want = cases[nv]
            eng.profile_reset()
            _same(eng.fr_mle_quotients(FC.rows(table), _z(z)), want)
            assert eng.kernel_stats("fr_mle_quotients")[1] == _passes(nv, rho, 256), nv
        assert _passes(13, rho, 256) > _passes(13, rho, 1 << 22) == -(-13 // rho)
    finally:
        assert lib.bn254_fr_mle_set_launch_max(0) == 0
        eng.profile(False)


def test_every_number_of_levels_per_pass_gives_the_same_bytes(eng, lib, cases):
    table, z, want = cases[7]
    try:
        for r in (1, 2, 3, 4):
            assert lib.bn254_fr_mle_quotients_set_levels(r) == 0
            eng.profile(True); eng.profile_reset()
            _same(eng.fr_mle_quotients(FC.rows(table), FC.rows(z)), want)
            assert eng.kernel_stats("fr_mle_quotients")[1] == -(-7 // r), r                      # the override is what ran
            eng.profile(False)
    finally:
        assert lib.bn254_fr_mle_quotients_set_levels(0) == 0
        eng.profile(False)


def test_the_dev_form_on_a_stream_equals_the_host_form_and_leaves_a(eng, rho, cases):
    """device-resident records on a stream that is not the default one; z is overwritten as soon as the call has returned"""
    import torch
    stream = torch.cuda.Stream()
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")
    host = lambda x: x.cpu().numpy().view(np.uint64).reshape(-1, 4)
    for nv in (0, 1, 2 * rho + 1, 13):
        table, z, want = cases[nv]
        A = FC.rows(table)
        d_a = dev(A)
        out = torch.zeros(4 << nv, dtype=torch.int64, device="cuda:0")
        Z = _z(z).copy()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            eng.fr_mle_quotients_dev(d_a.data_ptr(), Z, out.data_ptr(), stream=stream.cuda_stream)
            Z[:] = 0
        stream.synchronize()
        _same(host(out), want)
        _same(host(out), eng.fr_mle_quotients(A, _z(z)))
        assert host(d_a).tobytes() == A.tobytes()                                              # a is never written


def test_the_first_record_is_the_value_at_the_point(eng, cases):
    from bn_amd import Fr, mle
    for nv in (0, 3, 9):
        table, z, want = cases[nv]
        point = [Fr(v) for v in z]
        y, qs = mle.quotients(FC.rows(table), point, engine=eng)
        assert y == mle.evaluate(FC.rows(table), point, engine=eng) == Fr(MC.evaluate(table, z))
        assert [len(q) for q in qs] == [1 << j for j in range(nv)]
        assert [[q.v for q in qj] for qj in qs] == OC.split(OC.quotients(table, z))[1]


def test_a_call_right_after_a_sumcheck_round_shares_the_scratch(eng, rho, cases):
    """both keep their intermediate records in the same context-owned buffer: round, quotients, round, quotients on one context"""
    name, k, degree, groups = MC.group_sets()[0]
    rows = MC.rows_of(2 * 600, k, 7)
    limb_groups = [(FC.rows([c])[0], m) for c, m in groups]
    want_round = FC.rows(MC.round_sums(rows, groups, degree))
    T = MC.limbs(rows)
    for nv in (2 * rho + 1, 13):
        table, z, want = cases[nv]
        _same(eng.fr_sumcheck_round(T, limb_groups, degree), want_round)
        _same(eng.fr_mle_quotients(FC.rows(table), FC.rows(z)), want)
    _same(eng.fr_sumcheck_round(T, limb_groups, degree), want_round)


def test_two_host_threads_on_one_context_each_get_their_own_result(eng, cases):
    work = {0: cases[13], 1: cases[9]}
    got, errors = {}, []

    def run(t):
        try:
            table, z, _ = work[t]
            A, Z = FC.rows(table), FC.rows(z)
            got[t] = [eng.fr_mle_quotients(A, Z) for _ in range(4)]
        except Exception as exc:                                                                # noqa: BLE001 - reported below
            errors.append(exc)

    threads = [threading.Thread(target=run, args=(t,)) for t in work]
    for th in threads: th.start()
    for th in threads: th.join()
    assert not errors, errors
    for t in work:
        for out in got[t]:
            _same(out, work[t][2])


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr
    table, z = OC.values(8, 95), OC.point(3, 96)
    assert bn_amd.fr_mle_quotients([Fr(v) for v in table], [Fr(v) for v in z]) == [Fr(v) for v in OC.quotients(table, z)]
    assert bn_amd.fr_mle_quotients([Fr(7)], []) == [Fr(7)]
