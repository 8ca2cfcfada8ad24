"""KZG polynomial commitments over BN254 on the GPU, from calls the engine already has.

With a structured reference string (tau^i G)_{i<n}, H, tau H for a secret tau (G, H the generators of G1, G2):
    commit(p)   C = p(tau) G = sum p_i (tau^i G)                                one multi-scalar multiplication
    open(p, z)  y = p(z) and pi = q(tau) G with q = (p - y) / (X - z)           one reverse scan (poly.divide_linear), one multi-scalar multiplication
    verify      e(C - y G, H) == e(pi, (tau - z) H), checked as
                e(C - y G + z pi, H) * e(-pi, tau H) == 1                       so that nothing is computed in G2
verify_batch answers for m openings from ONE call sequence: one segmented multi-scalar multiplication of m three-term segments
(C_j * 1 + G * (-y_j) + pi_j * z_j), one batched subtraction for the negations, one batched multi-pairing check of two pairs per opening.
A random linear combination of the checks into one multi-pairing is not built."""
import collections

import numpy as np

from . import poly
from .api import Fr, G1, G2, _scalar_array, default_engine, pairing_check_batch
from .engine import G1_WORDS, G2_WORDS
from .groth16 import _draw

SRS = collections.namedtuple("SRS", "g1_powers g2_one tau_g2")
SRS.__doc__ = "g1_powers: (n, 12) uint64, the normalized points tau^i G for i < n, ready for the multi-scalar multiplications; g2_one: H; tau_g2: tau H"


def setup(n, rng, engine=None):
    """The reference string for polynomials of at most n coefficients from a secret tau drawn from rng - FOR TESTS AND DEVELOPMENT ONLY:
    whoever knows tau opens any commitment to any value, and this function knows it.  A ceremony that nobody can reconstruct is out of
    scope.  rng: an object with .bytes(n) (a numpy Generator); tau is 64 bytes little endian mod r, drawn again while zero.  The powers of
    tau are ONE scan (poly.powers); the points one fixed-base call per group."""
    if n < 1:
        raise ValueError(f"a reference string holds at least one power, got n = {n}")
    e = engine or default_engine()
    tau = 0
    while tau == 0:
        tau = _draw(rng)
    tau_powers = poly.powers(Fr(tau), n, engine=e, limbs=True)
    g1 = e.g1_mul_base_batch(G1.one().limbs, tau_powers)
    g2 = e.g2_mul_base_batch(G2.one().limbs, np.stack([Fr.one().limbs, Fr(tau).limbs]))
    return SRS(g1, G2(g2[0]), G2(g2[1]))


def _coefficients(srs, p):
    P = _scalar_array(p)
    if P.shape[0] > srs.g1_powers.shape[0]:
        raise ValueError(f"the polynomial has {P.shape[0]} coefficients but the reference string holds {srs.g1_powers.shape[0]} powers")
    return P


def commit(srs, p, engine=None):
    """C = p(tau) G -> G1: one multi-scalar multiplication of the coefficients (Fr values or an (k,4) uint64 array, constant term first)
    against the first k powers.  The empty polynomial commits to G1.zero().  ValueError when len(p) > n."""
    P = _coefficients(srs, p)
    if P.shape[0] == 0:
        return G1.zero()
    return G1((engine or default_engine()).g1_msm(srs.g1_powers[:P.shape[0]], P))


def open(srs, p, z, engine=None):
    """(y, proof): y = p(z) as an Fr and proof = q(tau) G for the quotient q of p by X - z - poly.divide_linear's one reverse scan, then one
    multi-scalar multiplication of q.  A constant (or empty) polynomial has the quotient zero: proof = G1.zero().  ValueError when len(p) > n."""
    P = _coefficients(srs, p)
    if P.shape[0] == 0:
        return Fr.zero(), G1.zero()
    e = engine or default_engine()
    out = poly._horner(P, z, e)
    y = Fr.from_limbs(out[0])
    if P.shape[0] == 1:
        return y, G1.zero()
    return y, G1(e.g1_msm(srs.g1_powers[:P.shape[0] - 1], out[1:]))


def verify_batch(srs, cs, zs, ys, proofs, engine=None):
    """numpy bool array, one entry per opening: is ys[j] the value at zs[j] of the polynomial committed to by cs[j], by proofs[j]?
    cs, proofs: sequences of G1; zs, ys: sequences of Fr.  ValueError when the four differ in length - before any device call."""
    cs, zs, ys, proofs = list(cs), list(zs), list(ys), list(proofs)
    m = len(cs)
    if not (len(zs) == len(ys) == len(proofs) == m):
        raise ValueError(f"{m} commitments, {len(zs)} points, {len(ys)} values and {len(proofs)} proofs")
    if m == 0:
        return np.zeros(0, bool)
    e = engine or default_engine()
    g, one = G1.one().limbs, Fr.one().limbs
    pi = np.stack([p.limbs for p in proofs])
    points = np.empty((m, 3, G1_WORDS), np.uint64); scalars = np.empty((m, 3, 4), np.uint64)
    points[:, 0] = np.stack([c.limbs for c in cs]); scalars[:, 0] = one
    points[:, 1] = g; scalars[:, 1] = np.stack([(-y).limbs for y in ys])
    points[:, 2] = pi; scalars[:, 2] = np.stack([z.limbs for z in zs])
    left = e.g1_msm_batch(points.reshape(-1, G1_WORDS), scalars.reshape(-1, 4), np.arange(m + 1, dtype=np.uint64) * 3)
    neg = e.g1_add_batch(np.tile(G1.zero().limbs, (m, 1)), pi, negate_b=True)
    P = np.empty((m, 2, G1_WORDS), np.uint64); Q = np.empty((m, 2, G2_WORDS), np.uint64)
    P[:, 0] = left; Q[:, 0] = srs.g2_one.limbs
    P[:, 1] = neg; Q[:, 1] = srs.tau_g2.limbs
    return pairing_check_batch(P.reshape(-1, G1_WORDS), Q.reshape(-1, G2_WORDS), offsets=np.arange(m + 1, dtype=np.uint64) * 2, engine=e)


def verify(srs, c, z, y, proof, engine=None):
    """bool: e(c - y G + z proof, H) * e(-proof, tau H) == 1, the opening equation e(c - y G, H) = e(proof, (tau - z) H) with the z moved to
    the G1 side"""
    return bool(verify_batch(srs, [c], [z], [y], [proof], engine=engine)[0])
