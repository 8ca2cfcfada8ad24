"""The bodies of bn254_fr_mle_eq, bn254_fr_mle_fold and bn254_fr_sumcheck_round (bn_amd/csrc/mle_ops.hpp) and the level arithmetic of a round
(host_plan.hpp bn_sumcheck_plan) on the CPU: tests/hostsim/hostsim_mle.cpp runs the kernels' own code over host arrays along the plan's own
levels against Python integers (tests/mle_cases.py over tests/fr_cases.py), for several piece lengths P and fans F.  The simulation also
checks every level against the scratch before its lanes run, so a plan that reads or writes outside it fails here and never on a device."""
import numpy as np
import pytest

import fr_cases as FC
import hostsim_mle_lib as HM
import mle_cases as MC

R = FC.R


@pytest.fixture(scope="module")
def PF():
    sim = HM.lib()
    return int(sim.hsm_shipped_piece()), int(sim.hsm_shipped_fan())


def _pf(PF):
    P, F = PF
    return sorted({(4, 2), (8, 16), (16, 4), (32, 16), (P, F), (P, 2)})


def _same(got, want):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), np.nonzero((got != want).any(axis=1))[0][:8]


def test_the_shipped_choices_are_among_the_swept_ones(PF):
    assert PF[0] in (4, 8, 16, 32) and PF[1] == 16


@pytest.fixture(scope="module")
def cases(PF):
    """per group set: rows for the largest half length of any (P, F) below and the model's sums for every half length a test asks for -
    computed once, never changed"""
    most = max(F * F * P + 1 for P, F in _pf(PF))
    return {name: (k, degree, groups, MC.rows_of(2 * most, k, 7 + i)) for i, (name, k, degree, groups) in enumerate(MC.group_sets())}


def _rows_for(rows, h):
    """2 h rows: the first h and h more, so that every half length sees other pairs"""
    return rows[:h] + rows[len(rows) - h:]


@pytest.mark.parametrize("name", [g[0] for g in MC.group_sets()])
def test_the_round_over_every_shape_piece_length_and_fan(PF, cases, name):
    k, degree, groups, rows = cases[name]
    want = {}
    for P, F in _pf(PF):
        for h in MC.round_shapes(P, F):
            if 2 * h > len(rows) or h < 1:
                continue
            sub = _rows_for(rows, h)
            if h not in want:
                want[h] = FC.rows(MC.round_sums(sub, groups, degree))
            got, launches = HM.round_(sub, groups, degree, P, F)
            _same(got, want[h])
            assert launches == MC.launches(h, degree, P, F, 1 << 22), (P, F, h)
            assert len(HM.plan(h, degree, P, F)[1]) == MC.sum_levels(h, P, F)
    assert len(want) >= 9


def test_the_first_two_values_add_up_to_the_whole_sum(PF, cases):
    k, degree, groups, rows = cases["degree 3, four groups"]
    P, F = PF
    sub = _rows_for(rows, F * P + 1)
    got = MC.round_sums(sub, groups, degree)
    assert (got[0] + got[1]) % R == sum(MC.expression(r, groups) for r in sub) % R


def test_the_seam_between_sub_launches_of_a_round(PF, cases):
    """25 lanes in sub-launches of 20"""
    k, degree, groups, rows = cases["degree 3, four groups"]
    P, F = PF
    sub = _rows_for(rows, 25 * P)
    got, launches = HM.round_(sub, groups, degree, P, F, step=20)
    _same(got, FC.rows(MC.round_sums(sub, groups, degree)))
    assert launches == MC.launches(25 * P, degree, P, F, 20) and launches[0] == 2


def test_the_limits_sixteen_tables_and_sixteen_groups(PF):
    P, F = PF
    rng = np.random.default_rng(3)
    rows = MC.rows_of(2 * (P + 1), 16, 21)
    groups = [(FC.rand(rng), [c, (c * 5 + 3) % 16, 15 - c][:1 + c % 3]) for c in range(16)]
    got, _ = HM.round_(rows, groups, 3, P, F)
    _same(got, FC.rows(MC.round_sums(rows, groups, 3)))


def test_the_plan_levels_tile_the_scratch(PF):
    for P, F in _pf(PF):
        for h in MC.round_shapes(P, F):
            for degree in (1, 4):
                lanes, levels, slots = HM.plan(h, degree, P, F)
                assert lanes == -(-h // P)
                if lanes == 1:
                    assert len(levels) == 0 and slots == 0
                    continue
                at, cnt = 0, lanes
                for cnt_l, lanes_l, src, dst, to_out in levels:
                    assert (cnt_l, src) == (cnt, at) and lanes_l == (degree + 1) * -(-cnt // F)
                    at += (degree + 1) * cnt; cnt = -(-cnt // F)
                    assert to_out == (cnt == 1) and (to_out or dst == at)
                assert at == slots and cnt == 1


@pytest.mark.parametrize("length", [2, 4, 254, 256, 258])
def test_fold_against_the_model(length):
    t = MC.values(length, 31)
    rng = np.random.default_rng(length)
    for r in (0, 1, R - 1, FC.rand(rng)):
        want = FC.rows(MC.fold(t, r))
        got, launches = HM.fold(t, r)
        _same(got, want); assert launches == 1
        whole, _ = HM.fold(t, r, in_place=True)
        _same(whole[:length // 2], want)
        _same(whole[length // 2:], FC.rows(t[length // 2:]))                # the upper half is left as it was
    got, launches = HM.fold(t, 5, step=100)
    _same(got, FC.rows(MC.fold(t, 5))); assert launches == -(-(length // 2) // 100)


def test_one_flat_fold_folds_index_major_tables_together():
    rows = MC.rows_of(2, 3, 33)
    got, _ = HM.fold(rows, 77)
    _same(got, FC.rows([MC.fold([rows[0][j], rows[1][j]], 77)[0] for j in range(3)]))
    rows = MC.rows_of(8, 3, 34)
    got, _ = HM.fold(rows, R - 2)
    _same(got, FC.rows([v for r in MC.fold(rows, R - 2) for v in r]))


def test_fold_rejects_an_odd_length_and_accepts_none():
    import ctypes as C
    sim = HM.lib()
    buf = np.zeros((4, 4), np.uint64); n = C.c_size_t()
    p = buf.ctypes.data_as(HM._U32P)
    assert sim.hsm_fold(p, 3, buf.ctypes.data, 64, p, C.byref(n)) == -2
    assert sim.hsm_fold(None, 0, None, 64, None, C.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("nv", [0, 1, 2, 7, 10])
def test_eq_against_the_model(nv):
    rng = np.random.default_rng(40 + nv)
    z = [(R - 1) if j % 3 == 1 else FC.rand(rng) for j in range(nv)]
    got, launches = HM.eq(z)
    _same(got, FC.rows(MC.eq_table(z))); assert launches == 1
    assert sum(MC.eq_table(z)) % R == 1
    bits = [(j * 5 + 1) % 3 % 2 for j in range(nv)]                         # a point of the hypercube: the indicator of its index
    want = [0] * (1 << nv); want[sum(b << j for j, b in enumerate(bits))] = 1
    _same(HM.eq(bits)[0], FC.rows(want))
    if nv == 10:
        got, launches = HM.eq(z, step=256)
        _same(got, FC.rows(MC.eq_table(z))); assert launches == 4


def test_evaluate_is_nv_folds():
    t = MC.values(32, 51)
    point = MC.values(5, 52)
    cur = t
    for r in point[::-1]:
        cur = MC.fold(cur, r)
    assert cur == [MC.evaluate(t, point)]
