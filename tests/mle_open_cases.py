"""TEST INFRASTRUCTURE - the integer model of the quotients of a multilinear opening (bn254_fr_mle_quotients: tests/test_hostsim_mle_open.py,
tests/test_host_plan_mle_open.py and tests/test_mle_open_abi.py on the CPU, tests/test_gpu_mle_open.py and tests/test_gpu_mkzg.py on the GPU),
over tests/mle_cases.py: Python integers, every difference and sum canonical, so the expected bytes are those of the model however a plan
cuts the levels into passes.  Conventions as there: index i is the point whose variable j is bit j of i; the MOST significant variable is
bound first."""
import numpy as np

import fr_cases as FC
import mle_cases as MC

R = FC.R
values = MC.values
evaluate = MC.evaluate


def quotients(table, z):
    """the heap of len(table) = 2^len(z) integers: out[0] = f(z) and out[2^j + i] = q_j[i] for j < nv, i < 2^j - from t = table, for
    j = nv - 1 down to 0 with half = 2^j, q_j[i] = t[i + half] - t[i] and t[i] = t[i] + z[j] q_j[i]"""
    nv = len(z)
    assert len(table) == 1 << nv
    t, out = list(table), [0] * len(table)
    for j in range(nv - 1, -1, -1):
        half = 1 << j
        for i in range(half):
            q = (t[i + half] - t[i]) % R
            out[half + i] = q
            t[i] = (t[i] + z[j] * q) % R
        t = t[:half]
    out[0] = t[0] % R
    return out


def split(heap):
    """(value, [q_0, .., q_{nv-1}]) of a heap"""
    nv = len(heap).bit_length() - 1
    return heap[0], [heap[1 << j:2 << j] for j in range(nv)]


def identity_gap(table, z, x):
    """evaluate(table, x) - y - sum_j (x_j - z_j) evaluate(q_j, x[:j]) mod r: zero for every x when the heap is the quotients of table at z"""
    y, qs = split(quotients(table, z))
    return (evaluate(table, x) - y - sum((x[j] - z[j]) * evaluate(qs[j], x[:j]) for j in range(len(z)))) % R


def point(nv, seed):
    """nv integers: 0, 1 and r - 1 among seeded random ones"""
    rng = np.random.default_rng(1000 + seed)
    z = [FC.rand(rng) for _ in range(nv)]
    for j, v in ((0, R - 1), (2, 0), (3, 1)):
        if j < nv:
            z[j] = v
    return z


def sizes(rho):
    """the numbers of variables around every seam of a plan of rho levels per pass: none, fewer than one pass, whole passes, one with a remainder"""
    return list(range(2 * rho + 2))


def plan(nv, rho):
    """the passes the planner must give, as (levels, vars, lanes, first, last) rows, and the scratch records"""
    rows, left = [], nv
    while left:
        levels = min(rho, left)
        rows.append((levels, left, 1 << (left - levels), int(left == nv), int(left == levels)))
        left -= levels
    return rows, (rows[0][2] if rows else 0)
