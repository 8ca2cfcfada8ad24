"""The planner of bn254_fr_scan_batch (host_plan.hpp bn_scan_plan) without a device: tests/hostsim/hostsim_scan.cpp hands its work list out as
plain words.  Every term is covered exactly once, no scratch slot is written twice, a level reads only what earlier levels wrote, and the
levels a segment of L terms takes part in are the documented 1 (L <= P) or 2 u + 3 (u up levels, u + 1 down levels)."""
import numpy as np
import pytest

import hostsim_scan_lib as HS
import scan_cases as SC

PIECES = (8, 16, 32, 64)
FANS = (2, 4, 16)
REDUCE, UP, DOWN, APPLY = range(4)


def _level_rows(pieces, levels):
    return [(int(kind), pieces[first:first + count]) for kind, first, count in levels]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("F", FANS)
@pytest.mark.parametrize("P", PIECES)
def test_the_invariants_of_the_plan(P, F, reverse):
    lens = SC.lengths(P, F) + [0, 0, 3 * F * P + 5]
    offsets = SC.offsets_of(lens)
    o = [int(v) for v in offsets]
    m, n = len(lens), o[-1]
    pieces, levels, slots = HS.plan(offsets, P, F, reverse)
    rows = _level_rows(pieces, levels)
    kinds = [k for k, _ in rows]
    u_max = max(SC.up_levels(L, P, F) for L in lens)
    assert kinds == [REDUCE] + [UP] * u_max + [DOWN] * (u_max + 1) + [APPLY]                    # the levels of the longest segment, in launch order
    assert len(kinds) == max(SC.plan_levels(L, P, F) for L in lens)
    # the apply level: every term exactly once, in pieces of at most P terms inside their segment, in the order of the recurrence
    apply = rows[-1][1]
    assert np.array_equal(apply, rows[0][1])                                                    # reduce runs over the same list
    assert len(apply) == sum(-(-L // P) for L in lens)
    covered = np.zeros(n, np.int64)
    at = {}
    for first, ln, flag, seg, slot in apply:
        assert 1 <= ln <= P and 0 <= seg < m
        lo, hi = (first + 1 - ln, first + 1) if reverse else (first, first + ln)
        assert o[seg] <= lo and hi <= o[seg + 1]
        covered[lo:hi] += 1
        assert bool(flag) == (lens[seg] <= P)
        expect = at.get(seg, o[seg + 1] - 1 if reverse else o[seg])                             # pieces of a segment follow each other
        assert first == expect
        at[seg] = first - ln if reverse else first + ln
    assert (covered == 1).all()
    assert sorted(at) == [j for j, L in enumerate(lens) if L]                                   # an empty segment has no piece
    # maps: written once, by reduce or an up level, before anything reads them; carries: written once by a down level before they are read
    map_level, carry_level = {}, {}
    seg_levels = {j: set() for j in range(m)}
    for l, (kind, rws) in enumerate(rows):
        for first, ln, flag, seg, slot in rws:
            seg_levels[int(seg)].add(l)
            if kind == REDUCE:
                if not flag:
                    assert slot not in map_level and 0 <= slot < slots
                    map_level[int(slot)] = l
            elif kind == UP:
                assert 1 <= ln <= F and not flag
                assert all(map_level[c] < l for c in range(first, first + ln))
                assert slot not in map_level and 0 <= slot < slots
                map_level[int(slot)] = l
            elif kind == DOWN:
                assert 1 <= ln <= F
                assert all(map_level[c] < l for c in range(first, first + ln))
                if not flag:
                    assert carry_level[int(slot)] < l
                for c in range(first, first + ln):
                    assert c not in carry_level
                    carry_level[c] = l
            else:
                if not flag:
                    assert carry_level[int(slot)] < l
    assert sorted(map_level) == list(range(slots)) and sorted(carry_level) == list(range(slots))
    assert slots < 2 * n // P + 64 * m
    # per segment: the number of levels it has a piece in is the documented count (a direct piece is in the shared reduce list but does nothing there)
    for j, L in enumerate(lens):
        got = len(seg_levels[j]) - (1 if 0 < L <= P else 0)
        assert got == SC.plan_levels(L, P, F), (L, got)
    tops = [r for kind, rws in rows if kind == DOWN for r in rws if r[2]]
    assert sorted(int(r[3]) for r in tops) == [j for j, L in enumerate(lens) if L > P]         # one lane per long segment starts from init[j]


def test_only_short_segments_are_one_level():
    P, F = 16, 16
    pieces, levels, slots = HS.plan(SC.offsets_of([0, 3, P, 0, 1]), P, F)
    assert [list(l) for l in levels] == [[APPLY, 0, 3]] and slots == 0 and all(p[2] for p in pieces)


@pytest.mark.parametrize("P, F", [(16, 16), (8, 2), (64, 4)])
def test_the_level_count_formula(P, F):
    for L in [P + 1, F * P, F * P + 1, F * F * P, F * F * P + 1, F * F * F * P + 1]:
        _, levels, _ = HS.plan(SC.offsets_of([L]), P, F)
        assert len(levels) == SC.plan_levels(L, P, F) == 2 * SC.up_levels(L, P, F) + 3
    assert SC.up_levels(F * P, P, F) == 0 and SC.up_levels(F * P + 1, P, F) == 1 and SC.up_levels(F * F * P + 1, P, F) == 2


def test_the_launch_counts_of_the_model_match_the_plan():
    P, F = 16, 16
    lens = [P] * 25 + [20 * P]
    _, levels, _ = HS.plan(SC.offsets_of(lens), P, F)
    per_kind = [0, 0, 0, 0]
    for kind, first, count in levels:
        per_kind[kind] += -(-count // 20)
    assert tuple(per_kind) == SC.launches(lens, P, F, 20) == (3, 1, 2, 3)
