"""bn_amd.kzg and the setup of bn_amd.groth16 on an MI355X (run with -m gpu): the powers of the trapdoor come from ONE scan
(bn_amd.poly.powers over bn254_fr_scan_batch), an opening from ONE reverse scan (poly.divide_linear) and a multi-scalar multiplication, the
verifier from the segmented multi-scalar multiplication and the batched multi-pairing check.  Everything is checked against Python integers
with the trapdoor redrawn from the same seed."""
import numpy as np
import pytest

import dot_cases as DC
import fr_cases as FC

pytestmark = pytest.mark.gpu
N = 64


def _draws(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(64), "little") % FC.R for _ in range(count)]


def _at(p, z):
    return sum(c * pow(z, i, FC.R) for i, c in enumerate(p)) % FC.R


@pytest.fixture(scope="module")
def srs():
    from bn_amd import kzg
    tau = _draws(900, 1)[0]
    assert tau != 0                                                                             # then setup keeps the first draw
    return kzg.setup(N, np.random.default_rng(900)), tau


@pytest.fixture(scope="module")
def opened(srs):
    """(p as integers, commitment, z, y, proof) for a random polynomial of 64 coefficients"""
    from bn_amd import Fr, kzg
    s, tau = srs
    rng = np.random.default_rng(901)
    p = [FC.rand(rng) for _ in range(N)]
    z = FC.rand(rng)
    c = kzg.commit(s, [Fr(v) for v in p])
    y, proof = kzg.open(s, [Fr(v) for v in p], Fr(z))
    return p, c, z, y, proof


def test_setup_is_the_powers_of_the_redrawn_trapdoor(srs):
    from bn_amd import Fr, G1, G2
    s, tau = srs
    assert s.g1_powers.shape == (N, 12) and s.g1_powers.dtype == np.uint64
    assert s.g2_one == G2.one() and s.tau_g2 == G2.one() * Fr(tau)
    for i in (0, 1, 17, N - 1):
        assert G1(s.g1_powers[i]) == G1.one() * Fr(pow(tau, i, FC.R)), i


def test_commit_is_the_polynomial_at_tau(srs, opened):
    from bn_amd import Fr, G1, kzg
    s, tau = srs
    p, c, z, y, proof = opened
    assert c == G1.one() * Fr(_at(p, tau))
    assert kzg.commit(s, FC.rows(p[:5])) == G1.one() * Fr(_at(p[:5], tau))                      # a shorter polynomial, as limbs
    assert kzg.commit(s, []) == G1.zero()
    with pytest.raises(ValueError, match="65 coefficients"):
        kzg.commit(s, [Fr.one()] * (N + 1))


def test_open_and_verify(srs, opened):
    from bn_amd import Fr, G1, kzg
    s, tau = srs
    p, c, z, y, proof = opened
    assert y == Fr(_at(p, z))
    assert proof == G1.one() * Fr((_at(p, tau) - y.v) * pow(tau - z, -1, FC.R))                # q(tau) = (p(tau) - y) / (tau - z)
    assert kzg.verify(s, c, Fr(z), y, proof) is True
    assert kzg.verify(s, c, Fr(z), y + Fr.one(), proof) is False                                # a changed y
    assert kzg.verify(s, c, Fr(z + 1), y, proof) is False                                       # a changed z
    assert kzg.verify(s, c, Fr(z), y, proof + G1.one()) is False                                # a changed proof


def test_a_constant_polynomial_opens_with_the_point_at_infinity(srs):
    from bn_amd import Fr, G1, kzg
    s, tau = srs
    k = Fr(123456789)
    c = kzg.commit(s, [k])
    y, proof = kzg.open(s, [k], Fr(5))
    assert c == G1.one() * k and y == k and proof == G1.zero()
    assert kzg.verify(s, c, Fr(5), y, proof) is True and kzg.verify(s, c, Fr(5), y + Fr.one(), proof) is False


def test_verify_batch_points_at_the_spoiled_opening(srs):
    from bn_amd import Fr, kzg
    s, tau = srs
    rng = np.random.default_rng(902)
    cs, zs, ys, proofs = [], [], [], []
    for L in (1, 2, 17, 40, N):
        p = [Fr(FC.rand(rng)) for _ in range(L)]
        z = Fr(FC.rand(rng))
        y, proof = kzg.open(s, p, z)
        cs.append(kzg.commit(s, p)); zs.append(z); ys.append(y); proofs.append(proof)
    assert kzg.verify_batch(s, cs, zs, ys, proofs).tolist() == [True] * 5
    ys[2] = ys[2] + Fr.one()
    assert kzg.verify_batch(s, cs, zs, ys, proofs).tolist() == [True, True, False, True, True]
    assert kzg.verify_batch(s, [], [], [], []).tolist() == []


# ---- groth16.setup takes its powers from poly.powers: the h query against the redrawn trapdoor, and a proof that verifies
def test_groth16_setup_h_query_and_a_proof(srs):
    from bn_amd import Fr, G1, groth16
    l = 2
    _, nv, a, b, c, z = DC.r1cs(12, l, [1, 2, 5, 3], seed=77)
    mat = lambda m: (np.array(m[0], np.uint64), np.array(m[1], np.uint64), FC.rows(m[2]))
    system = groth16.R1CS(l, nv, mat(a), mat(b), mat(c))
    n = 16
    alpha, beta, gamma, delta, tau = _draws(910, 5)
    assert all((alpha, beta, gamma, delta, tau)) and pow(tau, n, FC.R) != 1                     # then setup keeps the first five draws
    pk, vk = groth16.setup(system, np.random.default_rng(910))
    assert pk.h_query.shape == (n - 1, 12)
    t_over_delta = (pow(tau, n, FC.R) - 1) * pow(delta, -1, FC.R) % FC.R
    for k in (0, n - 2):
        assert G1(pk.h_query[k]) == G1.one() * Fr(pow(tau, k, FC.R) * t_over_delta), k
    proof = groth16.prove(pk, system, FC.rows(z), np.random.default_rng(911))
    assert groth16.verify_batch(vk, [proof], [[Fr(v) for v in z[1:l + 1]]]).tolist() == [True]
