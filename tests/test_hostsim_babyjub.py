"""The bodies of bn_amd/csrc/babyjub_ops.hpp and the width-6 Poseidon permutation on the CPU (tests/hostsim/hostsim_babyjub.cpp, g++ -DBN_BOUNDS:
fr_dot's operand and carry checks abort the process) against the integer model of tests/babyjub_cases.py, byte for byte: every edge point
times every edge scalar, both joint windows of the verifier, both forms of the width-6 matrix row, the known answers and one signature of
each failing class."""
import numpy as np
import pytest

import babyjub_cases as BC
import fr_cases as FC
import hostsim_babyjub_lib as H

R = BC.R


def test_validate_on_the_edge_points_and_across_a_seam():
    pts, want = BC.validate_cases()
    got, launches = H.validate(BC.point_rows(pts))
    assert got.tolist() == want and launches == 1
    assert set(want) == {0, 1, 4, 5}
    got, launches = H.validate(BC.point_rows(pts), step=7)
    assert got.tolist() == want and launches == -(-len(pts) // 7)


def test_every_edge_point_times_every_edge_scalar():
    pts = [p for _, p in BC.edge_points()]
    P = [p for p in pts for _ in BC.EDGE_SCALARS]
    K = [k for _ in pts for k in BC.EDGE_SCALARS]
    want = BC.point_rows([BC.mul(p, k) for p, k in zip(P, K)])
    got, _ = H.mul(BC.point_rows(P), FC.rows(K))
    assert np.array_equal(got, want)
    got, launches = H.mul(BC.point_rows(P[:50]), FC.rows(K[:50]), step=16, in_place=True)        # out is p, across sub-launch seams
    assert np.array_equal(got, want[:50]) and launches == 4


def test_the_chain_takes_the_whole_group_order():
    """8 l is above r, so no Fr holds it; the chain takes plain integers"""
    pts = [p for _, p in BC.edge_points()]
    assert np.array_equal(H.mul_raw(BC.point_rows(pts), [BC.ORDER] * len(pts)), BC.point_rows([BC.O] * len(pts)))
    ks = [BC.ORDER - 1, BC.ORDER + 1, (1 << 254) - 1, (1 << 256) - 1]
    assert np.array_equal(H.mul_raw(BC.point_rows([BC.G] * 4), ks), BC.point_rows([BC.mul(BC.G, k) for k in ks]))


def test_add_on_the_edge_pairs():
    pts = [p for _, p in BC.edge_points()]
    a = [p for p in pts for _ in pts]
    b = [q for _ in pts for q in pts]                        # every pair: P with P, P with -P, with O, with every small order
    want = BC.point_rows([BC.add(p, q) for p, q in zip(a, b)])
    got, _ = H.add(BC.point_rows(a), BC.point_rows(b))
    assert np.array_equal(got, want)
    got, _ = H.add(BC.point_rows(a), BC.point_rows(b), in_place=True)
    assert np.array_equal(got, want)
    neg = [BC.neg(p) for p in pts]
    assert np.array_equal(H.add(BC.point_rows(pts), BC.point_rows(neg))[0], BC.point_rows([BC.O] * len(pts)))


@pytest.mark.parametrize("split", [False, True])
def test_the_width_6_permutation_and_the_challenge(split):
    states = BC.PC.states(6, 40, 77)
    want = BC.PC.rows([BC.PC.permute(s) for s in states]).reshape(len(states), 6, 4)
    assert np.array_equal(H.permute6(BC.PC.rows(states).reshape(len(states), 6, 4), split=split), want)
    ins = list(BC.KNOWN_POSEIDON5)
    A = BC.point_rows([(i[2], i[3]) for i in ins]); R8 = BC.point_rows([(i[0], i[1]) for i in ins]); M = FC.rows([i[4] for i in ins])
    got, _ = H.challenge(A, R8, M, split=split)
    assert np.array_equal(got, FC.rows([BC.KNOWN_POSEIDON5[i] for i in ins]))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("window", [1, 2])
def test_verify_the_known_answer_and_every_failing_class(window, split):
    rows = [(BC.KAT_A, BC.KAT_R8, BC.KAT_S, BC.KAT_M)] + [row for _, row, _ in BC.failing_rows()] + list(BC.signatures(8, 5))
    want = [0] + [st for _, _, st in BC.failing_rows()] + [0] * 8
    A, R8, S, M = BC.signature_arrays(rows)
    got, launches = H.verify(A, R8, S, M, window, split=split)
    assert got.tolist() == want and launches == 1
    got, launches = H.verify(A, R8, S, M, window, step=5, split=split)
    assert got.tolist() == want and launches == -(-len(rows) // 5)


@pytest.mark.parametrize("window", [1, 2])
def test_verify_at_the_edge_scalars(window):
    """S and hm at the seams of the windows: A = O makes R8 = [S]B8 valid for every S below l, and a key of small order too"""
    ss = [k for k in BC.EDGE_SCALARS if k < BC.L] + [BC.L - 2, (1 << 250) + 1, 1 << 250]
    sm = list(BC.small_order_points().values())
    rows = [(sm[i % len(sm)], BC.mul(BC.B8, s), s, i) for i, s in enumerate(ss)]
    rows += [(sm[i % len(sm)], BC.mul(BC.B8, s + 1), s, i) for i, s in enumerate(ss)]        # and the wrong R8
    want = [0] * len(ss) + [6] * len(ss)
    assert [BC.verify_status(*r) for r in rows] == want
    got, _ = H.verify(*BC.signature_arrays(rows), window)
    assert got.tolist() == want


def test_the_library_ships_one_of_the_two_windows():
    assert H.lib().hsb_shipped_window() in (1, 2)
