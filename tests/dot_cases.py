"""TEST INFRASTRUCTURE - inputs and expected values of the sparse linear maps over Fr (bn254_fr_dot_batch: tests/test_hostsim_dot.py on the
CPU, tests/test_gpu_dot.py on the GPU) and of the Groth16 prover built on them.  The model is Python integers (tests/fr_cases.py): every
result is canonical, so the expected bytes are those of the integer sum whichever way a plan cuts a segment."""
import numpy as np

import fr_cases as FC
import ntt_cases as NC

R = FC.R


def lengths(P, F):
    """segment lengths around every seam of a plan with pieces of P terms and a fold of fan F: empty, one term, around one piece, a few
    pieces, exactly one fold lane, one more (a second fold level), and F * F pieces and one term (a third)"""
    return [0, 1, P - 1, P, P + 1, 2 * P + 3, F * P, F * P + 1, F * F * P + 1]


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def terms(n, seed):
    """(coeff, xval) integers for n terms.  The first 2 * FC.N_PAIR_HEAD terms have coefficient one and values a_0, b_0, a_1, b_1, .. of
    FC.pairs, so that the running sum of a segment lands just below, at and just above r; the rest are the same pairs from the start as
    products a * b: the sums' operands, edge values against random ones, zero on either side, then random products."""
    a, b = FC.pairs(max(n, 1), seed)
    H = FC.N_PAIR_HEAD
    coeff, xval = [], []
    for t in range(n):
        if t < 2 * H:
            coeff.append(1); xval.append(a[t // 2] if t % 2 == 0 else b[t // 2])
        else:
            coeff.append(a[t - 2 * H]); xval.append(b[t - 2 * H])
    return coeff, xval


def gathered(xval, seed, spare=3):
    """(x, index) with x[index[t]] == xval[t]: the values scattered over a vector of len(xval) + spare elements (the spare ones are random and
    named by no index)"""
    rng = np.random.default_rng(seed)
    n = len(xval)
    perm = rng.permutation(n + spare)[:n]
    x = [FC.rand(rng) for _ in range(n + spare)]
    for t, at in enumerate(perm):
        x[int(at)] = xval[t]
    return x, [int(i) for i in perm]


def model(coeff, x, offsets, index=None):
    """[sum of coeff[t] * x[index[t]] over the terms of segment j] as integers mod r"""
    o = [int(v) for v in offsets]
    at = (lambda t: t) if index is None else (lambda t: int(index[t]))
    return [sum(coeff[t] * x[at(t)] for t in range(o[j], o[j + 1])) % R for j in range(len(o) - 1)]


def plan_levels(L, P, F):
    """fold levels a segment of L terms takes: ceil(log_F(ceil(L / P))), none for a segment of at most one piece"""
    k, levels = -(-L // P), 0
    while k > 1:
        k = -(-k // F); levels += 1
    return levels


# ---- a rank-1 constraint system with a satisfying assignment by construction
def r1cs(constraints, l, row_lengths, seed, inputs=3):
    """(num_public, num_variables, a, b, c, z): z = (1, l public values, `inputs` private values, one fresh variable per constraint); constraint
    j defines its variable k as z_k = (A_j . z)(B_j . z) over variables in front of k, and C_j = e_k.  The lengths of the rows of A and B cycle
    through row_lengths (A from the front, B from the back; a row may name a variable more than once); coefficients and the free entries of z
    take FC.SPECIAL values first, then random ones.  Matrices are CSR triples (offsets, index, coeff) of integer lists."""
    rng = np.random.default_rng(seed)
    special = list(FC.SPECIAL)
    draw = lambda: special.pop(0) if special else FC.rand(rng)
    z = [1] + [draw() for _ in range(l + inputs)]
    coeffs = list(FC.SPECIAL)
    a, b, c = ([0], [], []), ([0], [], []), ([0], [], [])
    for j in range(constraints):
        k = len(z)
        dots = []
        for mat, L in ((a, row_lengths[j % len(row_lengths)]), (b, row_lengths[-1 - j % len(row_lengths)])):
            idx = [int(i) for i in rng.integers(0, k, L)]
            co = [coeffs.pop(0) if coeffs else FC.rand(rng) for _ in range(L)]
            mat[1].extend(idx); mat[2].extend(co); mat[0].append(len(mat[1]))
            dots.append(sum(cv * z[i] for cv, i in zip(co, idx)) % R)
        c[1].append(k); c[2].append(1); c[0].append(len(c[1]))
        z.append(dots[0] * dots[1] % R)
    return l, len(z), a, b, c, z


def lagrange_at(tau, log_n):
    """[L_j(tau) for j < n] over the subgroup of order n = 2^log_n, by Lagrange's formula: L_j(tau) = w^j (tau^n - 1) / (n (tau - w^j))"""
    n = 1 << log_n
    w = NC.root(log_n)
    t = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    return [pow(w, j, R) * t % R * pow(tau - pow(w, j, R), -1, R) % R for j in range(n)]


def column_values(mat, num_variables, lag):
    """[sum_j M[j, i] * lag[j] for i < num_variables]: u_i(tau) of a matrix given as a CSR triple"""
    out = [0] * num_variables
    o, idx, co = mat
    for j in range(len(o) - 1):
        for t in range(o[j], o[j + 1]):
            out[idx[t]] = (out[idx[t]] + co[t] * lag[j]) % R
    return out
