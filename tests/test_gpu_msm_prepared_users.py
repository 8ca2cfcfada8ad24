"""The first users of the prepared bases on an MI355X (run with -m gpu): bn_amd.kzg, bn_amd.mkzg and bn_amd.groth16 accept the plain or the
prepared reference string / proving key and return identical bytes either way - on the small route (default options) and on the prepared
bucket route (msm_bucket_min = 0)."""
import numpy as np
import pytest

import dot_cases as DC
import fr_cases as FC

pytestmark = pytest.mark.gpu
N = 64
ROUTES = ({}, {"msm_bucket_min": 0})


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


def _ran(eng, fn):
    """(result, launches of the prepared bucket route's reduction during fn, G1 and G2)"""
    eng.profile(True); eng.profile_reset()
    try:
        got = fn()
        return got, eng.kernel_stats("g1_msmp_reduce")[1] + eng.kernel_stats("g2_msmp_reduce")[1]
    finally:
        eng.profile(False)


def test_kzg_commit_open_and_commit_evals(eng):
    from bn_amd import Fr, kzg
    srs = kzg.setup(N, np.random.default_rng(2950), engine=eng)
    rng = np.random.default_rng(2951)
    p = FC.rows([FC.rand(rng) for _ in range(N)])
    z = Fr(FC.rand(rng))
    c, (y, proof) = kzg.commit(srs, p, engine=eng), kzg.open(srs, p, z, engine=eng)
    lsrs = kzg.lagrange_srs(srs, 6, engine=eng)
    evals = eng.fr_ntt_batch(p, 6)
    ce = kzg.commit_evals(lsrs, evals, engine=eng)
    assert ce == c
    psrs, plsrs = kzg.prepare(srs, engine=eng), kzg.prepare(lsrs, window_bits=5, engine=eng)
    assert isinstance(psrs, kzg.PreparedSRS) and isinstance(plsrs, kzg.PreparedLagrangeSRS)
    assert psrs.prepared.count == N and psrs.prepared.group == 1 and plsrs.prepared.window_bits == 5 and plsrs.log_n == 6
    for opts in ROUTES:
        with eng.options(**opts):
            (c2, (y2, proof2), ce2, short), ran = _ran(eng, lambda: (kzg.commit(psrs, p, engine=eng), kzg.open(psrs, p, z, engine=eng), kzg.commit_evals(plsrs, evals, engine=eng),
                                                                     kzg.commit(psrs, p[:17], engine=eng)))
        assert ran == (4 if opts else 0), (opts, ran)
        assert np.array_equal(c2.limbs, c.limbs) and y2 == y and np.array_equal(proof2.limbs, proof.limbs) and np.array_equal(ce2.limbs, ce.limbs), opts
        assert np.array_equal(short.limbs, kzg.commit(srs, p[:17], engine=eng).limbs), opts              # a prefix of the powers
    assert kzg.verify(psrs, c, z, y, proof, engine=eng) is True                                          # the verifier takes either as well
    assert kzg.commit(psrs, [], engine=eng) == kzg.commit(srs, [], engine=eng)
    with pytest.raises(ValueError, match="coefficients"):
        kzg.commit(psrs, np.zeros((N + 1, 4), np.uint64), engine=eng)


def test_mkzg_commit_reads_one_level_of_the_prepared_string(eng):
    from bn_amd import mkzg
    nv = 5
    srs = mkzg.setup(nv, np.random.default_rng(2960), engine=eng)
    psrs = mkzg.prepare(srs, engine=eng)
    assert isinstance(psrs, mkzg.PreparedSRS) and psrs.prepared.count == 2 << nv
    rng = np.random.default_rng(2961)
    for m in (5, 3, 0):
        T = FC.rows([FC.rand(rng) for _ in range(1 << m)])
        want = mkzg.commit(srs, T, engine=eng)
        for opts in ROUTES:
            with eng.options(**opts):
                got, ran = _ran(eng, lambda: mkzg.commit(psrs, T, engine=eng))
            assert ran == (1 if opts else 0), (m, opts, ran)
            assert np.array_equal(got.limbs, want.limbs), (m, opts)


def test_groth16_prove_with_a_prepared_proving_key(eng):
    """the small system of tests/test_gpu_kzg.py: 12 constraints, domain 16; one rng seed -> the same proof, and it verifies"""
    from bn_amd import Fr, groth16
    l = 2
    _, nv, a, b, c, z = DC.r1cs(12, l, [1, 2, 5, 3], seed=77)
    mat = lambda m: (np.array(m[0], np.uint64), np.array(m[1], np.uint64), FC.rows(m[2]))
    system = groth16.R1CS(l, nv, mat(a), mat(b), mat(c))
    pk, vk = groth16.setup(system, np.random.default_rng(910), engine=eng)
    proof = groth16.prove(pk, system, FC.rows(z), np.random.default_rng(911), engine=eng)
    ppk = groth16.prepare_proving_key(pk, engine=eng)
    assert isinstance(ppk, groth16.PreparedProvingKey) and all(x is y for x, y in zip(ppk[:10], pk))      # the key itself, and the handles
    assert {k: (h.group, h.count) for k, h in ppk.prepared.items()} == {"a_query": (1, nv), "b_g1_query": (1, nv), "l_query": (1, nv - l - 1), "h_query": (1, 15),
                                                                         "b_g2_query": (2, nv)}
    for opts in ROUTES:
        with eng.options(**opts):
            again, ran = _ran(eng, lambda: groth16.prove(ppk, system, FC.rows(z), np.random.default_rng(911), engine=eng))
        assert ran == (5 if opts else 0), (opts, ran)
        assert all(np.array_equal(x.limbs, y.limbs) for x, y in zip(again, proof)), opts
        assert groth16.verify_batch(vk, [again], [[Fr(v) for v in z[1:l + 1]]], engine=eng).tolist() == [True]
