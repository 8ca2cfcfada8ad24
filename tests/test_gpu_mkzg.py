"""bn_amd.mkzg on an MI355X (run with -m gpu): the reference string's levels, commitments against the host sum, openings of tables of 0, 1, 3
and 4 variables under ONE reference string, spoiled openings, a batch of mixed sizes, the homomorphism, and the end the module exists for -
the finals of a bn_amd.sumcheck proof opened against the commitments of its tables.  At most five variables throughout."""
import numpy as np
import pytest

import fr_cases as FC
import mle_cases as MC
import mle_open_cases as OC

pytestmark = pytest.mark.gpu
R = FC.R
NV = 4
SIZES = (0, 1, 3, 4)


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def srs(eng):
    from bn_amd import mkzg
    return mkzg.setup(NV, np.random.default_rng(2024), engine=eng)


@pytest.fixture(scope="module")
def openings(eng, srs):
    """per number of variables: (table, point, commitment, value, proofs) - made once, never changed"""
    from bn_amd import Fr, mkzg
    out = {}
    for m in SIZES:
        table, z = OC.values(1 << m, 300 + m), OC.point(m, 50 + m)
        T, point = FC.rows(table), [Fr(v) for v in z]
        c = mkzg.commit(srs, T, engine=eng)
        y, proofs = mkzg.open(srs, T, point, engine=eng)
        out[m] = (table, point, c, y, proofs)
    return out


def test_every_level_of_the_reference_string_folds_into_the_level_below(eng, srs):
    """eq(tau[:j], i) = eq(tau[:j+1], i) + eq(tau[:j+1], i + 2^j): the two halves of level j + 1 add up to level j"""
    from bn_amd import G1
    g = srs.g1_levels
    assert g.shape == (2 << NV, 12) and len(srs.tau_g2) == NV
    assert eng.g1_eq(g[1:2], G1.one().limbs.reshape(1, 12))[0] and G1(g[0]).is_zero()
    for j in range(NV):
        lo, hi = g[(2 << j):(2 << j) + (1 << j)], g[(2 << j) + (1 << j):(4 << j)]
        assert eng.g1_eq(g[(1 << j):(2 << j)], eng.g1_add_batch(lo, hi)).all(), j


def test_commit_is_the_host_sum_of_the_terms(eng, srs, openings):
    from bn_amd import G1
    for m in (0, 3):
        table, _, c, _, _ = openings[m]
        terms = eng.g1_mul_batch(srs.g1_levels[1 << m:2 << m], FC.rows(table))
        acc = G1.zero().limbs
        for t in terms:
            acc = eng.g1_add_batch(acc, t)[0]
        assert eng.g1_eq(c.limbs, acc)[0], m


@pytest.mark.parametrize("m", SIZES)
def test_an_opening_verifies_under_the_one_reference_string(eng, srs, openings, m):
    from bn_amd import Fr, mkzg
    table, point, c, y, proofs = openings[m]
    assert y == Fr(MC.evaluate(table, [p.v for p in point])) and len(proofs) == m
    assert mkzg.verify(srs, c, point, y, proofs, engine=eng)


def test_spoiled_openings_are_rejected(eng, srs, openings):
    from bn_amd import Fr, mkzg
    table, point, c, y, proofs = openings[3]
    assert mkzg.verify(srs, c, point, y, proofs, engine=eng)
    assert not mkzg.verify(srs, c, point, y + Fr.one(), proofs, engine=eng)                     # a wrong value
    assert not mkzg.verify(srs, c, point, y, [proofs[0], proofs[2], proofs[2]], engine=eng)      # one proof replaced
    assert not mkzg.verify(srs, c, [point[0], point[1] + Fr.one(), point[2]], y, proofs, engine=eng)   # one coordinate of the point
    other = mkzg.commit(srs, FC.rows(OC.values(8, 399)), engine=eng)
    assert not mkzg.verify(srs, other, point, y, proofs, engine=eng)                             # the commitment of another table
    table0, point0, c0, y0, _ = openings[0]
    assert not mkzg.verify(srs, c0, [], y0 + Fr.one(), [], engine=eng)


def test_a_batch_of_mixed_sizes_reports_exactly_the_spoiled_ones(eng, srs, openings):
    from bn_amd import Fr, mkzg
    order = [4, 0, 3, 1, 3, 4]
    cs = [openings[m][2] for m in order]
    points = [list(openings[m][1]) for m in order]
    ys = [openings[m][3] for m in order]
    proofs = [list(openings[m][4]) for m in order]
    ys[1] = ys[1] + Fr.one()                                                                    # the constant table opened to another value
    proofs[4][1] = proofs[4][0]                                                                 # one proof of a three-variable opening replaced
    got = mkzg.verify_batch(srs, cs, points, ys, proofs, engine=eng)
    assert got.dtype == bool and list(got) == [True, False, True, True, False, True]


def test_commitments_and_openings_are_homomorphic(eng, srs, openings):
    from bn_amd import mkzg
    table, point, ca, ya, pa = openings[3]
    other = OC.values(8, 398)
    cb = mkzg.commit(srs, FC.rows(other), engine=eng)
    yb, pb = mkzg.open(srs, FC.rows(other), point, engine=eng)
    both = [(a + b) % R for a, b in zip(table, other)]
    y, p = mkzg.open(srs, FC.rows(both), point, engine=eng)
    assert y == ya + yb and mkzg.commit(srs, FC.rows(both), engine=eng) == ca + cb
    assert all(pj == aj + bj for pj, aj, bj in zip(p, pa, pb))
    assert mkzg.verify(srs, ca + cb, point, ya + yb, [aj + bj for aj, bj in zip(pa, pb)], engine=eng)


def test_the_finals_of_a_sumcheck_proof_open_against_the_commitments_of_its_tables(eng, srs):
    """sumcheck.prove over three committed tables of four variables; every final is the opening of its table at the proof's point"""
    from bn_amd import Fr, mkzg, sumcheck
    name, k, degree, groups = MC.group_sets()[0]
    assert name == "degree 3, four groups" and k == 3
    rows = MC.rows_of(1 << NV, k, 17)
    T = MC.limbs(rows)
    commitments = [mkzg.commit(srs, T[:, j], engine=eng) for j in range(k)]
    fr_groups = [(Fr(c), m) for c, m in groups]
    proof, point = sumcheck.prove(T, fr_groups, engine=eng)
    ok, vpoint = sumcheck.verify(proof, NV, fr_groups)
    assert ok and vpoint == point
    opened = [mkzg.open(srs, T[:, j], point, engine=eng) for j in range(k)]
    assert [y for y, _ in opened] == proof.finals
    cs, pts, pfs = commitments, [point] * k, [p for _, p in opened]
    assert mkzg.verify_batch(srs, cs, pts, proof.finals, pfs, engine=eng).all()
    finals = list(proof.finals); finals[1] = finals[1] + Fr.one()                               # a proof with one final altered
    assert list(mkzg.verify_batch(srs, cs, pts, finals, pfs, engine=eng)) == [True, False, True]
    assert not mkzg.verify(srs, cs[1], point, finals[1], pfs[1], engine=eng)
