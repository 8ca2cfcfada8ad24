"""TEST INFRASTRUCTURE - inputs and expected values of the multilinear calls over Fr (bn254_fr_mle_eq, bn254_fr_mle_fold, bn254_fr_sumcheck_round:
tests/test_hostsim_mle.py and tests/test_mle_abi.py on the CPU, tests/test_gpu_mle.py and tests/test_gpu_sumcheck.py on the GPU).  The model
is Python integers (tests/fr_cases.py): every product and sum is canonical, so the expected bytes are those of the integer sums however a plan
deals the indices out.  Conventions: index i of a table of nv variables is the point whose variable j is bit j of i; a fold binds the MOST
significant variable; k tables are stored index-major, rows[i][j] = table j at index i."""
import numpy as np

import fr_cases as FC

R = FC.R


def values(n, seed):
    """n integers: seeded random ones with 0, r - 1, 1 and the other FC.SPECIAL values sprinkled in at co-prime strides"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        v = FC.rand(rng)
        if t % 37 == 5 + seed % 3: v = 0
        elif t % 41 == 7: v = R - 1
        elif t % 13 == 3: v = 1
        elif t % 29 == 11: v = FC.SPECIAL[(t // 29) % len(FC.SPECIAL)]
        out.append(v)
    return out


def rows_of(n, k, seed):
    """n rows of k integers: table j at index i is rows[i][j]"""
    flat = values(n * k, seed)
    return [flat[i * k:(i + 1) * k] for i in range(n)]


def limbs(rows):
    """rows of k integers -> the (n, k, 4) uint64 array of Montgomery images"""
    n, k = len(rows), len(rows[0])
    return FC.rows([v for r in rows for v in r]).reshape(n, k, 4)


def eq_table(z):
    """[prod_j (z[j] if bit j of i else 1 - z[j]) for i < 2^len(z)]"""
    out = [1]
    for zj in z:
        out = [v * (1 - zj) % R for v in out] + [v * zj % R for v in out]
    return out


def fold(table, r):
    """the most significant variable bound to r; the entries may be integers or rows of integers"""
    half = len(table) // 2
    one = lambda lo, hi: (lo + r * (hi - lo)) % R
    if table and isinstance(table[0], (list, tuple)):
        return [[one(a, b) for a, b in zip(table[i], table[i + half])] for i in range(half)]
    return [one(table[i], table[i + half]) for i in range(half)]


def expression(row, groups):
    """sum_c coeff_c * prod_{j in group c} row[j]"""
    total = 0
    for c, members in groups:
        term = c
        for j in members:
            term = term * row[j] % R
        total += term
    return total % R


def round_sums(rows, groups, degree):
    """[sum_{i < h} expression at the rows interpolated to t, for t = 0 .. degree], h = len(rows) / 2"""
    h = len(rows) // 2
    out = []
    for t in range(degree + 1):
        total = 0
        for i in range(h):
            total += expression([(lo + t * (hi - lo)) % R for lo, hi in zip(rows[i], rows[i + h])], groups)
        out.append(total % R)
    return out


def degree_of(groups):
    return max(len(m) for _, m in groups)


def evaluate(table, point):
    return sum(t * e for t, e in zip(table, eq_table(point))) % R


def prove(rows, groups, challenge):
    """the model prover: (claim, rounds, finals, point) as integers.  challenge(s, g) gives the challenge of round s from its values g (the
    caller owns the transcript); point[j] is the challenge of round nv - 1 - j."""
    degree = degree_of(groups)
    rounds, chal = [], []
    while len(rows) > 1:
        g = round_sums(rows, groups, degree)
        r = challenge(len(rounds), g)
        rows = fold(rows, r)
        rounds.append(g); chal.append(r)
    return (rounds[0][0] + rounds[0][1]) % R, rounds, list(rows[0]), chal[::-1]


def round_shapes(P, F):
    """half lengths around every seam of the plan with P indices per lane and levels of fan F: one and two indices, around one lane, two lanes,
    exactly one sum lane per t, one more (a second sum level), and F * F lanes and one index (a third)"""
    return [1, 2, P - 1, P, P + 1, 2 * P, F * P, F * P + 1, F * F * P + 1]


def sum_levels(h, P, F):
    """sum levels of a round over h indices: none for one lane, else how often cnt -> ceil(cnt / F) is taken until one is left"""
    cnt, levels = -(-h // P), 0
    while cnt > 1:
        cnt = -(-cnt // F); levels += 1
    return levels


def launches(h, degree, P, F, step):
    """sub-launches (of the round kernel, of the sum levels) of a round over h indices, `step` lanes per sub-launch at most"""
    parts = lambda lanes: -(-lanes // step)
    cnt = -(-h // P)
    total = 0
    while cnt > 1:
        cnt = -(-cnt // F)
        total += parts((degree + 1) * cnt)
    return parts(-(-h // P)), total


# the group sets of the GPU and host-simulation tests: (name, k, degree, groups) with coefficients from the edge values
def group_sets(seed=0):
    rng = np.random.default_rng(100 + seed)
    c, c2 = FC.rand(rng), FC.rand(rng)
    return [
        ("degree 3, four groups", 3, 3, [(c, [0, 1, 2]), (R - 1, [0, 2]), (0, [1]), (c2, [1, 1])]),
        ("degree 4, a table twice", 3, 4, [(c, [0, 1, 2, 0]), (c2, [1])]),
        ("degree 1, one table", 1, 1, [(1, [0])]),
        ("degree 4 over short groups", 3, 4, [(c, [0, 1]), (c2, [2]), (R - 2, [2, 2])]),
    ]
