"""bn_amd.sumcheck on an MI355X (run with -m gpu): a proof that eq(tau, x) * (A(x) B(x) - C(x)) sums to zero over the hypercube for C = A o B, at
one variable, two, and enough for three sum levels of the round kernel; the finals against mle.evaluate; the transcript restated here
with hashlib; spoiled proofs."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import fr_cases as FC
import mle_cases as MC

pytestmark = pytest.mark.gpu
R = FC.R


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def sizes():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_sumcheck_piece.restype = C.c_uint; l.bn254_fr_sumcheck_fan.restype = C.c_uint
    P, F = int(l.bn254_fr_sumcheck_piece()), int(l.bn254_fr_sumcheck_fan())
    return [1, 2, (2 * F * P - 1).bit_length() + 1]                                             # ceil(log2(2 F P)) + 1


@pytest.fixture(scope="module")
def proofs(eng, sizes):
    """per nv: (tables as an (n, 4, 4) array, groups, proof, point) - proved once, never changed"""
    from bn_amd import Fr, sumcheck
    out = {}
    for nv in sizes:
        tau = MC.values(nv, 71)
        a, b = MC.values(1 << nv, 72), MC.values(1 << nv, 73)
        c = [x * y % R for x, y in zip(a, b)]
        T = np.stack([FC.rows(t) for t in (MC.eq_table(tau), a, b, c)], axis=1)
        groups = [(Fr(1), [0, 1, 2]), (Fr(R - 1), [0, 3])]
        proof, point = sumcheck.prove(T, groups, engine=eng)
        out[nv] = (T, groups, proof, point)
    return out


@pytest.mark.parametrize("which", [0, 1, 2])
def test_an_honest_proof_verifies_and_its_finals_are_the_tables_at_the_point(eng, sizes, proofs, which):
    from bn_amd import Fr, mle, sumcheck
    nv = sizes[which]
    T, groups, proof, point = proofs[nv]
    assert proof.claim == Fr.zero() and len(proof.rounds) == nv and len(point) == nv
    ok, vpoint = sumcheck.verify(proof, nv, groups)
    assert ok and vpoint == point
    assert proof.finals == [mle.evaluate(T[:, j], point, engine=eng) for j in range(4)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_transcript_restated_with_hashlib_gives_the_challenges(sizes, proofs, which):
    nv = sizes[which]
    T, groups, proof, point = proofs[nv]
    h = lambda b: hashlib.sha256(b).digest()
    be = lambda xs: b"".join(int(x).to_bytes(32, "big") for x in xs)
    state = h(b"bn_amd.sumcheck")
    state = h(state + be([nv, 4, 3, 2]))
    for c, m in groups:
        state = h(state + be([c.v, len(m)] + m))
    state = h(state + be([proof.claim.v]))
    chal = []
    for g in proof.rounds:
        state = h(state + be([x.v for x in g]))
        chal.append(int.from_bytes(h(state + b"\x00") + h(state + b"\x01"), "big") % R)
        state = h(state + b"\x02")
    assert [p.v for p in point] == chal[::-1]


def test_spoiled_proofs_are_rejected(sizes, proofs):
    from bn_amd import Fr, sumcheck
    nv = sizes[-1]
    T, groups, proof, point = proofs[nv]
    one = Fr.one()
    rounds = [list(g) for g in proof.rounds]
    rounds[nv // 2][2] = rounds[nv // 2][2] + one
    assert not sumcheck.verify(proof._replace(rounds=rounds), nv, groups)[0]
    finals = list(proof.finals); finals[3] = finals[3] + one
    assert not sumcheck.verify(proof._replace(finals=finals), nv, groups)[0]
    assert not sumcheck.verify(proof._replace(claim=one), nv, groups)[0]
    assert sumcheck.verify(proof, nv, groups)[0]


def test_a_sum_that_is_not_zero_has_a_non_zero_claim(eng, sizes, proofs):
    from bn_amd import Fr, sumcheck
    nv = sizes[1]
    T, groups, _, _ = proofs[nv]
    wrong = T.copy()
    wrong[1, 3] = FC.rows([5])[0]                                                               # C is no longer A o B at index 1
    proof, _ = sumcheck.prove(wrong, groups, engine=eng)
    rows = [[Fr.from_limbs(wrong[i, j]).v for j in range(4)] for i in range(1 << nv)]
    assert proof.claim == Fr(sum(MC.expression(r, [(c.v, m) for c, m in groups]) for r in rows)) != Fr.zero()
    assert sumcheck.verify(proof, nv, groups)[0] and not sumcheck.verify(proof._replace(claim=Fr.zero()), nv, groups)[0]
