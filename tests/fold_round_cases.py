"""TEST INFRASTRUCTURE - inputs and expected values of the fused fold-then-round call (bn254_fr_sumcheck_fold_round: tests/test_hostsim_fold_round.py
and tests/test_fold_round_abi.py on the CPU, tests/test_gpu_fold_round.py on the GPU).  The model is tests/mle_cases.py: MC.fold followed by
MC.round_sums, in Python integers - the bytes of the two existing calls, however the fused kernel cuts the work."""
import numpy as np

import fr_cases as FC
import mle_cases as MC

R = FC.R


def group_sets():
    """MC.group_sets() and one more whose table 3 NO group names: its folded column must still be right"""
    rng = np.random.default_rng(200)
    c, c2 = FC.rand(rng), FC.rand(rng)
    return MC.group_sets() + [("a table no group names", 4, 3, [(c, [0, 1, 2]), (R - 1, [0, 2]), (c2, [1, 1])])]


def challenges(seed):
    """the fold's edge challenges - 0 keeps the lower half, 1 the upper - and a random one"""
    return [0, 1, R - 1, FC.rand(np.random.default_rng(300 + seed))]


def rows_for(rows, h2):
    """4 h2 rows: the first 2 h2 and the last 2 h2, so that every length sees other quadruples"""
    return rows[:2 * h2] + rows[len(rows) - 2 * h2:]


def fold_round(rows, r, groups, degree):
    """(the n / 2 folded rows, the degree + 1 sums of the round over them)"""
    folded = MC.fold(rows, r)
    return folded, MC.round_sums(folded, groups, degree)


def launches(h2, degree, P, F, step):
    """sub-launches (of the fused kernel, of the sum levels) of a call over n = 4 h2 rows: the round's over h2 indices"""
    return MC.launches(h2, degree, P, F, step)


def fold_piece(h2, P, fill):
    """the model of host_plan.hpp bn_sumcheck_fold_piece: P halved down to 4 while ceil(h2 / P) < fill"""
    while P > 4 and -(-h2 // P) < fill:
        P //= 2
    return P
