"""The body of bn254_fr_mle_quotients (bn_amd/csrc/mle_ops.hpp fr_mle_quotients_body) driven through the passes of host_plan.hpp
(bn_mle_quotients_plan) on the CPU: tests/hostsim/hostsim_mle_open.cpp runs the kernel's own code over host arrays, with the bounds of fr.hpp
enforced, against Python integers (tests/mle_open_cases.py), for every number of levels per pass the library compiles.  The simulation
checks every pass against the scratch before its lanes run, so a plan that reads or writes outside it fails here and never on a device."""
import numpy as np
import pytest

import fr_cases as FC
import hostsim_mle_open_lib as HO
import mle_open_cases as OC

R = FC.R
RHOS = (1, 2, 3, 4)


def _same(got, want):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), np.nonzero((got != want).any(axis=1))[0][:8]


def test_the_shipped_choice_is_among_the_compiled_ones():
    sim = HO.lib()
    assert int(sim.hso_shipped_levels()) in RHOS and int(sim.hso_levels_max()) == max(RHOS)


@pytest.fixture(scope="module")
def cases():
    """per number of variables: the table, the point and the model's heap - computed once, never changed"""
    out = {}
    for nv in range(2 * max(RHOS) + 2):
        table, z = OC.values(1 << nv, 80 + nv), OC.point(nv, nv)
        out[nv] = (table, z, FC.rows(OC.quotients(table, z)))
    return out


def test_the_model_satisfies_the_opening_identity_at_random_points(cases):
    """evaluate(table, x) - y == sum_j (x_j - z_j) * evaluate(q_j, x[:j]), and y is the value at z"""
    rng = np.random.default_rng(5)
    for nv in (0, 1, 2, 5, 8):
        table, z, _ = cases[nv]
        assert OC.quotients(table, z)[0] == OC.evaluate(table, z)
        for x in ([FC.rand(rng) for _ in range(nv)], [0] * nv, [1] * nv, z):
            assert OC.identity_gap(table, z, x) == 0, (nv, x)
    table, z, _ = cases[4]
    spoiled = list(table); spoiled[3] = (spoiled[3] + 1) % R
    y, qs = OC.split(OC.quotients(table, z))
    x = [FC.rand(rng) for _ in range(4)]
    assert (OC.evaluate(spoiled, x) - y - sum((x[j] - z[j]) * OC.evaluate(qs[j], x[:j]) for j in range(4))) % R != 0


@pytest.mark.parametrize("rho", RHOS)
def test_quotients_against_the_model_for_every_size_around_the_passes(cases, rho):
    for nv in OC.sizes(rho):
        table, z, want = cases[nv]
        assert {0, 1, R - 1} <= set(z) or nv < 4
        got, a, launches = HO.quotients(table, z, rho)
        _same(got, want)
        _same(a, FC.rows(table))                                            # a is never written
        assert launches == -(-nv // rho), (nv, rho)


@pytest.mark.parametrize("rho", RHOS)
def test_the_seam_between_sub_launches_of_a_pass(cases, rho):
    """2^(nv - rho) lanes of the first pass in sub-launches of 20: more than one per pass while a pass has more than 20 lanes"""
    nv = 2 * rho + 1
    table, z, want = cases[nv]
    got, _, launches = HO.quotients(table, z, rho, step=20)
    _same(got, want)
    passes, _ = HO.plan(nv, rho)
    assert launches == sum(-(-p[2] // 20) for p in passes) and (launches > len(passes) or (1 << (nv - rho)) <= 20)
    got, _, launches = HO.quotients(table, z, rho, step=1)
    _same(got, want)
    assert launches == sum(p[2] for p in passes)


def test_edge_points_fold_to_the_corners():
    """z on the hypercube: the value is the table's entry there, whatever the levels per pass"""
    table = OC.values(32, 91)
    for bits in ([0] * 5, [1] * 5, [1, 0, 1, 1, 0]):
        for rho in RHOS:
            got, _, _ = HO.quotients(table, bits, rho)
            _same(got[:1], FC.rows([table[sum(b << j for j, b in enumerate(bits))]]))
    for rho in RHOS:
        got, _, _ = HO.quotients(table, [R - 1] * 5, rho)
        _same(got, FC.rows(OC.quotients(table, [R - 1] * 5)))
