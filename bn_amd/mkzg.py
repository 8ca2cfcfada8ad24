"""Multilinear KZG (PST) polynomial commitments over BN254 on the GPU, from calls the engine already has and bn_amd.fr_mle_quotients.

A multilinear polynomial f of m variables is the table of its 2^m values over the hypercube (bn_amd.mle: index i is the point whose variable
j is bit j of i).  With a structured reference string eq((tau_0 .. tau_{j-1}), i) G for every level j <= nv, H and tau_j H for a secret
point tau (G, H the generators of G1, G2):
    commit(f)   C = f(tau) G = sum_i f[i] (eq(tau, i) G)                          one multi-scalar multiplication against level m
    open(f, z)  y = f(z) and pi_j = q_j(tau_0 .. tau_{j-1}) G for the m quotients
                f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1})               one fr_mle_quotients, one segmented multi-scalar multiplication
    verify      e(C - y G, H) == prod_j e(pi_j, (tau_j - z_j) H), checked as
                e(C - y G + sum_j z_j pi_j, H) * prod_j e(-pi_j, tau_j H) == 1    so that nothing is computed in G2
Level j of the reference string is both the basis that commits a table of j variables and the basis of proof j, and fr_mle_quotients
writes q_j to records [2^j, 2^(j+1)) of its output - the rows of level j -, so open copies nothing.  This is what ties the `finals` of a
bn_amd.sumcheck proof to committed tables: the prover opens every table at the sumcheck's point.  verify_batch answers for many openings, of
mixed sizes, from ONE call sequence: one segmented multi-scalar multiplication of m + 2 terms per opening, one batched subtraction for the
negations, one batched multi-pairing check of m + 1 pairs per opening.  Not built: opening several tables at one point (combine them with a
random linear combination: commitments are homomorphic), a random linear combination of the checks into one multi-pairing, Zeromorph /
HyperKZG over the univariate kzg, a bucket-method route for the top proof levels."""
import collections

import numpy as np

from .api import Fr, G1, G2, _scalar_array, default_engine, pairing_check_batch
from .engine import G1_WORDS, G2_WORDS, _mle_quotients_args
from .groth16 import _draw

SRS = collections.namedtuple("SRS", "nv g1_levels g2_one tau_g2")
SRS.__doc__ = ("nv: variables, at most; g1_levels: (2^(nv+1), 12) uint64, the normalized points g1_levels[2^j + i] = eq((tau_0 .. tau_{j-1}), i) G for "
               "j <= nv, i < 2^j, record 0 G1.zero() - so g1_levels[1] = G -, ready for the multi-scalar multiplications; g2_one: H; tau_g2: the nv points tau_j H")


def setup(nv, rng, engine=None):
    """The reference string for tables of at most nv variables from a secret point tau drawn from rng - FOR TESTS AND DEVELOPMENT ONLY:
    whoever knows tau opens any commitment to any value, and this function knows it.  A ceremony that nobody can reconstruct is out of
    scope.  rng: an object with .bytes(n) (a numpy Generator); every tau_j is 64 bytes little endian mod r, drawn again while zero.  The
    levels are nv + 1 calls of fr_mle_eq over the prefixes of tau; the points one fixed-base call per group."""
    if nv < 0:
        raise ValueError(f"a reference string is for nv >= 0 variables, got nv = {nv}")
    e = engine or default_engine()
    tau = []
    while len(tau) < nv:
        t = _draw(rng)
        if t:
            tau.append(Fr(t))
    T = _scalar_array(tau)
    scalars = np.concatenate([np.zeros((1, 4), np.uint64)] + [e.fr_mle_eq(T[:j]) for j in range(nv + 1)])
    g1 = e.g1_mul_base_batch(G1.one().limbs, scalars)
    g1[0] = G1.zero().limbs
    g2 = e.g2_mul_base_batch(G2.one().limbs, np.concatenate([Fr.one().limbs.reshape(1, 4), T]))
    return SRS(nv, g1, G2(g2[0]), [G2(q) for q in g2[1:]])


PreparedSRS = collections.namedtuple("PreparedSRS", "nv g1_levels g2_one tau_g2 prepared")
PreparedSRS.__doc__ = "an SRS and `prepared`, the PreparedMSM of its g1_levels: commit runs level m as the range from 2^m of that handle"


def prepare(srs, window_bits=None, engine=None):
    """SRS -> PreparedSRS: the levels go to the device once (Engine.g1_msm_prepare); commit accepts either and returns the same bytes.
    The prepared string is used with the engine that prepared it."""
    return PreparedSRS(srs.nv, srs.g1_levels, srs.g2_one, srs.tau_g2, (engine or default_engine()).g1_msm_prepare(srs.g1_levels, window_bits))


def _table(srs, table):
    """(the (2^m, 4) array, m)"""
    T = _scalar_array(table)
    n = T.shape[0]
    if n == 0 or n & (n - 1):
        raise ValueError(f"the table holds {n} values: a multilinear polynomial has a power of two, one at least")
    if n > 1 << srs.nv:
        raise ValueError(f"the table holds {n} values but the reference string is for {srs.nv} variables: at most {1 << srs.nv}")
    return T, n.bit_length() - 1


def commit(srs, table, engine=None):
    """C = f(tau) G -> G1 for the multilinear f with these 2^m values (Fr values or an (n,4) uint64 array), m <= nv: one multi-scalar
    multiplication against level m of the reference string.  ValueError for a length that is not a power of two or is too long."""
    T, m = _table(srs, table)
    e = engine or default_engine()
    prep = getattr(srs, "prepared", None)
    if prep is not None:
        return G1(e.g1_msm_prepared(prep, T, first=1 << m))
    return G1(e.g1_msm(srs.g1_levels[1 << m:2 << m], T))


def open(srs, table, point, engine=None):
    """(y, proofs): y = f(point) as an Fr and proofs[j] = q_j(tau_0 .. tau_{j-1}) G, a G1, for the m quotients of f at point - ONE
    fr_mle_quotients, then ONE segmented multi-scalar multiplication whose segment j is records [2^j, 2^(j+1)) of its output against the same
    rows of the reference string.  A table of one record has no proofs.  ValueError unless len(table) == 2^len(point) <= 2^nv."""
    T, m = _table(srs, table)
    T, z = _mle_quotients_args(T, _scalar_array(point))
    e = engine or default_engine()
    out = e.fr_mle_quotients(T, z)
    y = Fr.from_limbs(out[0])
    if m == 0:
        return y, []
    n = 1 << m
    offsets = np.array([(1 << j) - 1 for j in range(m + 1)], np.uint64)
    return y, [G1(p) for p in e.g1_msm_batch(srs.g1_levels[1:n], out[1:n], offsets)]


def verify_batch(srs, cs, points, ys, proofs, engine=None):
    """numpy bool array, one entry per opening: is ys[k] the value at points[k] of the multilinear polynomial committed to by cs[k], by
    proofs[k]?  cs: a sequence of G1; points: sequences of Fr; ys: a sequence of Fr; proofs: sequences of G1, as many as the point has
    variables.  Openings of different numbers of variables may be mixed.  ValueError when the four differ in length, a point and its proofs
    differ in length or a point has more than nv variables - before any device call."""
    cs, points, ys, proofs = list(cs), [list(z) for z in points], list(ys), [list(p) for p in proofs]
    count = len(cs)
    if not (len(points) == len(ys) == len(proofs) == count):
        raise ValueError(f"{count} commitments, {len(points)} points, {len(ys)} values and {len(proofs)} lists of proofs")
    for k in range(count):
        if len(points[k]) != len(proofs[k]):
            raise ValueError(f"opening {k}: the point has {len(points[k])} variables but {len(proofs[k])} proofs were given")
        if len(points[k]) > srs.nv:
            raise ValueError(f"opening {k}: the point has {len(points[k])} variables but the reference string is for {srs.nv}")
    if count == 0:
        return np.zeros(0, bool)
    e = engine or default_engine()
    g, one, h = G1.one().limbs, Fr.one().limbs, srs.g2_one.limbs
    ms = np.array([len(z) for z in points], np.uint64)
    seg = np.concatenate([[0], np.cumsum(ms + 2)]).astype(np.uint64)          # the terms of the left sides
    pair = np.concatenate([[0], np.cumsum(ms + 1)]).astype(np.uint64)         # the pairs of the checks
    pts = np.empty((int(seg[-1]), G1_WORDS), np.uint64); scalars = np.empty((int(seg[-1]), 4), np.uint64)
    for k in range(count):
        at = int(seg[k])
        pts[at] = cs[k].limbs; scalars[at] = one
        pts[at + 1] = g; scalars[at + 1] = (-ys[k]).limbs
        for j, (pi, zj) in enumerate(zip(proofs[k], points[k])):
            pts[at + 2 + j] = pi.limbs; scalars[at + 2 + j] = zj.limbs
    left = e.g1_msm_batch(pts, scalars, seg)
    P = np.empty((int(pair[-1]), G1_WORDS), np.uint64); Q = np.empty((int(pair[-1]), G2_WORDS), np.uint64)
    pis = [pi.limbs for p in proofs for pi in p]
    neg = iter(e.g1_add_batch(np.tile(G1.zero().limbs, (len(pis), 1)), np.stack(pis), negate_b=True) if pis else ())
    for k in range(count):
        at = int(pair[k])
        P[at] = left[k]; Q[at] = h
        for j in range(int(ms[k])):
            P[at + 1 + j] = next(neg); Q[at + 1 + j] = srs.tau_g2[j].limbs
    return pairing_check_batch(P, Q, offsets=pair, engine=e)


def verify(srs, c, point, y, proofs, engine=None):
    """bool: e(c - y G + sum_j point_j proofs_j, H) * prod_j e(-proofs_j, tau_j H) == 1, the opening equation
    e(c - y G, H) = prod_j e(proofs_j, (tau_j - point_j) H) with the point moved to the G1 side"""
    return bool(verify_batch(srs, [c], [point], [y], [proofs], engine=engine)[0])
