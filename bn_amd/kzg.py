"""KZG polynomial commitments over BN254 on the GPU, from calls the engine already has.

With a structured reference string (tau^i G)_{i<n}, H, tau H for a secret tau (G, H the generators of G1, G2):
    commit(p)   C = p(tau) G = sum p_i (tau^i G)                                one multi-scalar multiplication
    open(p, z)  y = p(z) and pi = q(tau) G with q = (p - y) / (X - z)           one reverse scan (poly.divide_linear), one multi-scalar multiplication
    verify      e(C - y G, H) == e(pi, (tau - z) H), checked as
                e(C - y G + z pi, H) * e(-pi, tau H) == 1                       so that nothing is computed in G2
verify_batch answers for m openings from ONE call sequence: one segmented multi-scalar multiplication of m three-term segments
(C_j * 1 + G * (-y_j) + pi_j * z_j), one batched subtraction for the negations, one batched multi-pairing check of two pairs per opening.
A random linear combination of the checks into one multi-pairing is not built.
Over the transforms on G1 (bn254_g1_ntt_batch), none of which needs tau:
    lagrange_srs    the points L_j(tau) G of the domain {w^j}: one inverse transform of the powers
    commit_evals    C from the n evaluations of p over the domain: one multi-scalar multiplication against those points
    open_all        every opening of p over the domain (FK20): three transforms over G1, two over Fr, one batched multiplication
prepare(srs) / prepare(lsrs) take the points of a reference string once (Engine.g1_msm_prepare); commit, open and commit_evals accept the
prepared string wherever they accept the plain one and return the same bytes."""
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


PreparedSRS = collections.namedtuple("PreparedSRS", "g1_powers g2_one tau_g2 prepared")
PreparedSRS.__doc__ = "an SRS and `prepared`, the PreparedMSM of its g1_powers: commit and open run their multi-scalar multiplications against it"
PreparedLagrangeSRS = collections.namedtuple("PreparedLagrangeSRS", "g1_lagrange log_n g2_one tau_g2 prepared")
PreparedLagrangeSRS.__doc__ = "a LagrangeSRS and `prepared`, the PreparedMSM of its g1_lagrange: commit_evals runs against it"


def prepare(srs, window_bits=None, engine=None):
    """SRS -> PreparedSRS, LagrangeSRS -> PreparedLagrangeSRS: the points of the string go to the device once, as the affine multiples of
    every window (Engine.g1_msm_prepare); every later commit / open / commit_evals sends the scalars only.  The prepared string is used
    with the engine that prepared it."""
    e = engine or default_engine()
    if hasattr(srs, "g1_lagrange"):
        return PreparedLagrangeSRS(srs.g1_lagrange, srs.log_n, srs.g2_one, srs.tau_g2, e.g1_msm_prepare(srs.g1_lagrange, window_bits))
    return PreparedSRS(srs.g1_powers, srs.g2_one, srs.tau_g2, e.g1_msm_prepare(srs.g1_powers, window_bits))


def _msm(e, srs, points, k):
    """normalize(sum points[i] * k[i]) over the first len(k) points of the string: against the handle of a prepared string"""
    prep = getattr(srs, "prepared", None)
    return e.g1_msm_prepared(prep, k, 0) if prep is not None else e.g1_msm(points[:k.shape[0]], k)


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
    return G1(_msm(engine or default_engine(), srs, srs.g1_powers, P))


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
    return y, G1(_msm(e, srs, srs.g1_powers, out[1:]))


LagrangeSRS = collections.namedtuple("LagrangeSRS", "g1_lagrange log_n g2_one tau_g2")
LagrangeSRS.__doc__ = "g1_lagrange: (2^log_n, 12) uint64, the normalized points L_j(tau) G over the domain {w^j}; g2_one: H; tau_g2: tau H"


def lagrange_srs(srs, log_n, engine=None):
    """The reference string in the Lagrange basis of the domain {w^j}, w = Fr.root_of_unity(log_n), WITHOUT tau: ONE inverse transform over
    G1 of the first n = 2^log_n powers, L_j(tau) G = n^-1 sum_k w^(-j k) (tau^k G).  ValueError when the string holds fewer than n powers."""
    n = 1 << log_n
    if srs.g1_powers.shape[0] < n:
        raise ValueError(f"a Lagrange basis of 2^{log_n} points needs {n} powers but the reference string holds {srs.g1_powers.shape[0]}")
    return LagrangeSRS((engine or default_engine()).g1_ntt_batch(srs.g1_powers[:n], log_n, True), log_n, srs.g2_one, srs.tau_g2)


def commit_evals(lsrs, evals, engine=None):
    """C = p(tau) G -> G1 for the polynomial of degree < n given by its n evaluations over the domain (Fr values or an (n,4) uint64 array):
    one multi-scalar multiplication against the Lagrange points - the commitment commit() gives for the inverse transform of evals.
    ValueError unless there are exactly n evaluations."""
    E = _scalar_array(evals)
    if E.shape[0] != lsrs.g1_lagrange.shape[0]:
        raise ValueError(f"{E.shape[0]} evaluations against a Lagrange basis of {lsrs.g1_lagrange.shape[0]} points")
    return G1(_msm(engine or default_engine(), lsrs, lsrs.g1_lagrange, E))


def open_all(srs, p, log_n, engine=None):
    """(ys, proofs): every opening of p on the domain {w^m}, w = Fr.root_of_unity(log_n) - ys[m] = p(w^m) and proofs[m] the proof
    open(srs, p, w^m) gives - from a few transforms instead of n multi-scalar multiplications (Feist and Khovratovich's FK20).  With
    d = len(p) - 1 the proofs are the forward transform over G1 of (h_0 .. h_(d-1), O, ..), h_k = sum_(i <= d-1-k) p_(i+k+1) (tau^i G), and
    the h_k are a convolution of the coefficients with the reversed powers: entries d-1 .. 2d-2 of the inverse transform of size 2n of the
    entry-wise product (one g1_mul_batch) of the transformed coefficients and the transformed points.  The transform of the points depends
    on the reference string and d only; it is not kept between calls.  A constant or empty polynomial has all-infinity proofs.
    ValueError when len(p) > n or len(p) > the powers of the string, or 2n is above the largest transform over G1."""
    P = _coefficients(srs, p)
    n, L = 1 << log_n, P.shape[0]
    if L > n:
        raise ValueError(f"the polynomial has {L} coefficients but the domain holds {n} points")
    e = engine or default_engine()
    zero_fr = np.zeros((1, 4), np.uint64)
    ys = e.fr_ntt_batch(np.concatenate([P, np.tile(zero_fr, (n - L, 1))]), log_n)
    inf = G1.zero().limbs
    d = L - 1
    if d <= 0:
        return [Fr.from_limbs(r) for r in ys], [G1.zero() for _ in range(n)]
    s_hat = np.concatenate([srs.g1_powers[:d][::-1], np.tile(inf, (2 * n - d, 1))])
    c = np.concatenate([P[1:], np.tile(zero_fr, (2 * n - d, 1))])
    prod = e.g1_mul_batch(e.g1_ntt_batch(s_hat, log_n + 1), e.fr_ntt_batch(c, log_n + 1))
    h = e.g1_ntt_batch(prod, log_n + 1, True)[d - 1:2 * d - 1]
    proofs = e.g1_ntt_batch(np.concatenate([h, np.tile(inf, (n - d, 1))]), log_n)
    return [Fr.from_limbs(r) for r in ys], [G1(r) for r in proofs]


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
