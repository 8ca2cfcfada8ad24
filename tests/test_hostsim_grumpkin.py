"""The bodies of bn_amd/csrc/grumpkin_ops.hpp on the CPU (tests/hostsim/hostsim_grumpkin.cpp, g++ -DBN_BOUNDS) against the integer model of
tests/grumpkin_cases.py, byte for byte: validation, every edge pair added, every edge point times every edge scalar, in place, across
sub-launch seams, the dedicated doubling against add(P, P), and the segmented sum replayed over bn_dot_plan."""
import numpy as np

import grumpkin_cases as GC
import hostsim_grumpkin_lib as H


def test_validate_on_the_edge_points_and_across_a_seam():
    pts, want = GC.validate_cases()
    got, launches = H.validate(GC.point_rows(pts))
    assert got.tolist() == want and launches == 1 and set(want) == {0, 1, 4}
    got, launches = H.validate(GC.point_rows(pts), step=7)
    assert got.tolist() == want and launches == -(-len(pts) // 7)


def test_add_on_the_edge_pairs():
    pts = [p for _, p in GC.edge_points()]
    a = [p for p in pts for _ in pts]
    b = [q for _ in pts for q in pts]                        # every pair: P with P, P with -P, with O, O with O
    want = GC.point_rows([GC.add(p, q) for p, q in zip(a, b)])
    got, _ = H.add(GC.point_rows(a), GC.point_rows(b))
    assert np.array_equal(got, want)
    got, _ = H.add(GC.point_rows(a), GC.point_rows(b), in_place=True)
    assert np.array_equal(got, want)
    neg = [GC.neg(p) for p in pts]
    assert np.array_equal(H.add(GC.point_rows(pts), GC.point_rows(neg))[0], np.zeros((len(pts), 2, 4), np.uint64))        # O is sixteen zero words


def test_every_edge_point_times_every_edge_scalar():
    pts = [p for _, p in GC.edge_points()]
    P = [p for p in pts for _ in GC.EDGE_SCALARS]
    K = [k for _ in pts for k in GC.EDGE_SCALARS]
    want = GC.point_rows([GC.mul(p, k) for p, k in zip(P, K)])
    got, _ = H.mul(GC.point_rows(P), GC.scalar_rows(K))
    assert np.array_equal(got, want)
    got, launches = H.mul(GC.point_rows(P[:50]), GC.scalar_rows(K[:50]), step=16, in_place=True)        # out is p, across sub-launch seams
    assert np.array_equal(got, want[:50]) and launches == 4
    assert np.array_equal(H.mul(GC.point_rows(P), GC.scalar_rows(K), window=5)[0], want)                                    # the buildable 5-bit window: digits across word seams
    q = GC.scalar_rows([GC.Q] * len(pts))
    assert np.array_equal(H.mul(GC.point_rows(pts), q)[0], np.zeros((len(pts), 2, 4), np.uint64))                          # [q]P = O


def test_sub_launches_of_64_over_130_records():
    P, K = GC.curve_points(130, 3), GC.scalars(130, 4)
    small = [k if i < len(GC.EDGE_SCALARS) else k & 0xffffffff for i, k in enumerate(K)]                                 # the model stays quick
    want = GC.point_rows([GC.mul(p, k) for p, k in zip(P, small)])
    got, launches = H.mul(GC.point_rows(P), GC.scalar_rows(small), step=64)
    assert np.array_equal(got, want) and launches == 3
    Q = P[1:] + P[:1]
    got, launches = H.add(GC.point_rows(P), GC.point_rows(Q), step=64, in_place=True)
    assert np.array_equal(got, GC.point_rows([GC.add(a, b) for a, b in zip(P, Q)])) and launches == 3
    got, launches = H.validate(GC.point_rows(P), step=64)
    assert got.tolist() == [0] * 130 and launches == 3


def test_the_doubling_agrees_with_add_p_p_on_every_test_point():
    pts = list(GC.curve_points(40, 3))
    out, ok = H.double_vs_add(GC.point_rows(pts))
    assert ok.tolist() == [3] * len(pts)
    assert np.array_equal(out, GC.point_rows([GC.add(p, p) for p in pts]))


def test_the_segmented_sum_over_its_plan():
    pts, ks, offs, want = GC.msm_cases()
    P, K = GC.point_rows(pts), GC.scalar_rows(ks)
    got, (slots, levels, launches) = H.msm(P, K, offs)
    assert np.array_equal(got, GC.point_rows(want))
    fan = H.lib().hsg_fan()
    assert fan == 16 and levels == 4 and launches == 4                       # 257 terms: 17 partial sums after one fold level, 2 after two, then the last
    want_slots = 0
    for L in (b - a for a, b in zip(offs, offs[1:]) if b - a > 1):
        want_slots += L
        while L > fan:
            L = -(-L // fan); want_slots += L
    assert slots == want_slots
    got, (_, _, launches) = H.msm(P, K, offs, step=64)                        # the same call across sub-launch seams
    assert np.array_equal(got, GC.point_rows(want)) and launches > 3
    # msm == mul followed by a host-side sum
    prods, _ = H.mul(P, K)
    from bn_amd import Fr
    rows = [(Fr.from_limbs(r[0]).v, Fr.from_limbs(r[1]).v) for r in prods]
    sums = []
    for a, b in zip(offs, offs[1:]):
        acc = GC.O
        for t in range(a, b):
            acc = GC.add(acc, rows[t])
        sums.append(acc)
    assert sums == list(want)


def test_the_segmented_sum_checks_its_offsets():
    P, K = GC.point_rows([GC.G] * 3), GC.scalar_rows([1, 2, 3])
    assert H.msm(P, K, [1, 3]) == -2 and H.msm(P, K, [0, 3, 2]) == -2
    got, (slots, levels, launches) = H.msm(P[:0], K[:0], [0, 0, 0])          # empty segments only: (0, 0) each, one level, no scratch
    assert not got.any() and (slots, levels, launches) == (0, 1, 1)
