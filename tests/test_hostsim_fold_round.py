"""The body of bn254_fr_sumcheck_fold_round (bn_amd/csrc/mle_ops.hpp fr_sumcheck_fold_round_body) and the level arithmetic of its round
(host_plan.hpp bn_sumcheck_plan) on the CPU: tests/hostsim/hostsim_fold_round.cpp runs the kernel's own code over host arrays along the
plan's own levels against Python integers - MC.fold followed by MC.round_sums -, for several piece lengths P and fans F, out of place and in
place.  folded and out are pre-filled with a pattern, and the simulation checks every level against the scratch before its lanes run."""
import numpy as np
import pytest

import fold_round_cases as FR
import fr_cases as FC
import hostsim_fold_round_lib as HF
import mle_cases as MC

R = FC.R
SETS = FR.group_sets()


@pytest.fixture(scope="module")
def PF():
    sim = HF.lib()
    return int(sim.hfr_shipped_piece()), int(sim.hfr_shipped_fan())


def _pf(PF):
    P, _ = PF
    return sorted({(4, 2), (8, 16), (16, 4), (P, 16), (P, 2)})


def _same(got, want):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), np.nonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))[0][:8]


def _pattern(a):
    assert (a == HF.PATTERN).all()


def test_the_shipped_choices_are_among_the_swept_ones(PF):
    assert PF[0] in (4, 8, 16) and PF[1] == 16


@pytest.fixture(scope="module")
def cases(PF):
    """per group set: rows for the largest h2 of any (P, F) below - computed once, never changed"""
    most = max(F * F * P + 1 for P, F in _pf(PF))
    return {name: (k, degree, groups, MC.rows_of(4 * most, k, 17 + i)) for i, (name, k, degree, groups) in enumerate(SETS)}


def _check(rows, r, groups, degree, P, F, want, step=1 << 22):
    """one call out of place and one in place against the model's (folded, sums); returns the sub-launches"""
    n, k = len(rows), len(rows[0])
    folded_w, out_w = want
    before = MC.limbs(rows)
    T, folded, out, launches = HF.fold_round(rows, r, groups, degree, P, F, step)
    _same(T, before)                                                        # out of place: the tables are unchanged
    _same(folded[:n // 2 * k].reshape(n // 2, k, 4), folded_w); _pattern(folded[n // 2 * k:])
    _same(out[:degree + 1], out_w); _pattern(out[degree + 1:])
    T, _, out, launches2 = HF.fold_round(rows, r, groups, degree, P, F, step, in_place=True)
    _same(T[:n // 2], folded_w)
    _same(T[n // 2:], before[n // 2:])                                      # in place: rows [n/2, n) are left as they were
    _same(out[:degree + 1], out_w); _pattern(out[degree + 1:])
    assert launches2 == launches
    return launches


@pytest.mark.parametrize("name", [g[0] for g in SETS])
def test_fold_round_over_every_shape_piece_length_fan_and_challenge(PF, cases, name):
    k, degree, groups, rows = cases[name]
    want = {}
    for P, F in _pf(PF):
        for h2 in MC.round_shapes(P, F):
            if h2 < 1:
                continue
            sub = FR.rows_for(rows, h2)
            for r in FR.challenges(h2) if h2 <= 2 * P else FR.challenges(h2)[3:]:      # the edge challenges on the short shapes, a random one on all
                if (h2, r) not in want:
                    folded, sums = FR.fold_round(sub, r, groups, degree)
                    want[h2, r] = (MC.limbs(folded), FC.rows(sums))
                    if r in (0, 1):                                         # the folded table is the lower / the upper half
                        _same(want[h2, r][0], MC.limbs(sub)[2 * h2 * r:2 * h2 * (r + 1)])
                launches = _check(sub, r, groups, degree, P, F, want[h2, r])
                assert launches == FR.launches(h2, degree, P, F, 1 << 22), (P, F, h2)
    assert len({h2 for h2, _ in want}) >= 9


def test_the_unnamed_table_is_folded_all_the_same(PF, cases):
    name, k, degree, groups = SETS[-1]
    assert k == 4 and all(3 not in m for _, m in groups)
    rows = FR.rows_for(cases[name][3], PF[0] + 1)
    r = FR.challenges(5)[3]
    T, folded, _, _ = HF.fold_round(rows, r, groups, degree, *PF)
    n = len(rows)
    column = folded[:n // 2 * k].reshape(n // 2, k, 4)[:, 3]
    _same(column, FC.rows(MC.fold([row[3] for row in rows], r)))


def test_the_seam_between_sub_launches(PF, cases):
    """25 lanes in sub-launches of 20"""
    name, k, degree, groups = SETS[0]
    P, F = PF
    sub = FR.rows_for(cases[name][3], 25 * P)
    r = FR.challenges(25)[3]
    folded, sums = FR.fold_round(sub, r, groups, degree)
    launches = _check(sub, r, groups, degree, P, F, (MC.limbs(folded), FC.rows(sums)), step=20)
    assert launches == FR.launches(25 * P, degree, P, F, 20) and launches[0] == 2


def test_the_limits_sixteen_tables_and_sixteen_groups(PF):
    P, F = PF
    rng = np.random.default_rng(3)
    rows = MC.rows_of(4 * (P + 1), 16, 21)
    groups = [(FC.rand(rng), [c, (c * 5 + 3) % 16, 15 - c][:1 + c % 3]) for c in range(16)]
    r = FC.rand(rng)
    folded, sums = FR.fold_round(rows, r, groups, 3)
    _check(rows, r, groups, 3, P, F, (MC.limbs(folded), FC.rows(sums)))


def test_the_model_is_the_two_existing_bodies(PF, cases):
    """the fused simulation against the simulation of the fold and of the round (tests/hostsim/hostsim_mle.cpp), not only against integers"""
    import hostsim_mle_lib as HM
    name, k, degree, groups = SETS[1]
    P, F = PF
    sub = FR.rows_for(cases[name][3], F * P + 1)
    r = FR.challenges(7)[3]
    T, folded, out, _ = HF.fold_round(sub, r, groups, degree, P, F)
    n = len(sub)
    two, _ = HM.fold(sub, r)
    _same(folded[:n // 2 * k], two)
    rnd, _ = HM.round_(MC.fold(sub, r), groups, degree, P, F)
    _same(out[:degree + 1], rnd)
