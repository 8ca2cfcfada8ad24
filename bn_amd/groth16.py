"""Groth16 verification of a block of proofs under one verifying key, on the GPU.

A proof (A: G1, B: G2, C: G1) with public inputs a_1 .. a_l is valid when
    e(A, B) = e(alpha, beta) * e(L, gamma) * e(C, delta),        L = IC[0] + sum a_i * IC[i]
which is checked as  e(A, B) * e(-alpha, beta) * e(-L, gamma) * e(-C, delta) == 1.  A block takes three calls: one segmented multi-scalar
multiplication for every L (bn_amd.g1_msm_batch, segment j: IC[0] * 1, IC[i] * a_ji), one batched subtraction for the negations and one
batched multi-pairing check (bn_amd.pairing_check_batch, four pairs per proof).  With prepared=True the G2 side of the block - the key's beta,
gamma, delta and every proof's B - is prepared once on the device (Engine.g2_prepare) and the check runs over the native line tables
(Engine.pairing_product_batch_prepared_native): the four pairs of a proof share one Miller accumulator.

verify_aggregate answers for the whole block at once: a random linear combination of the m checks is ONE multi-pairing of m + 3 pairs."""
import collections
import secrets

import numpy as np

from .api import Fr, G1, Gt, R_MOD, default_engine, pairing_check_batch
from .engine import G1_WORDS, G2_WORDS

VerifyingKey = collections.namedtuple("VerifyingKey", "alpha_g1 beta_g2 gamma_g2 delta_g2 ic")
VerifyingKey.__doc__ = "alpha_g1: G1; beta_g2, gamma_g2, delta_g2: G2; ic: l + 1 G1 points for l public inputs"


def verify_batch(vk, proofs, public_inputs, engine=None, prepared=False):
    """numpy bool array, one entry per proof.  proofs: sequence of (A: G1, B: G2, C: G1); public_inputs: one sequence of l = len(vk.ic) - 1
    Fr per proof.  prepared: run the pairing checks over ONE prepared handle [beta, gamma, delta, B_0 .. B_{m-1}] (check j: points 3 + j, 0,
    1, 2), made for this block and closed before returning; same answers.  Worth it for blocks of many thousand proofs (2^16: 0.78 of the
    default path's kernel time, preparation included); a small block pays ~1.3 ms of preparation for nothing (profiles/r09_product_batch_prepared.txt)."""
    e = engine or default_engine()
    proofs = list(proofs); public_inputs = [list(a) for a in public_inputs]
    m, l = len(proofs), len(vk.ic) - 1
    if len(public_inputs) != m:
        raise ValueError(f"{m} proofs but {len(public_inputs)} sets of public inputs")
    if any(len(a) != l for a in public_inputs):
        raise ValueError(f"every proof takes {l} public inputs (len(vk.ic) - 1)")
    if m == 0:
        return np.zeros(0, bool)
    ic = np.stack([p.limbs for p in vk.ic])
    one = Fr.one().limbs
    K = np.stack([one if i == 0 else a[i - 1].limbs for a in public_inputs for i in range(l + 1)])
    L = e.g1_msm_batch(np.tile(ic, (m, 1)), K, np.arange(m + 1, dtype=np.uint64) * (l + 1))
    # -alpha, -L_j, -C_j in one call: zero - x (lib.rs:113-114)
    C = np.stack([c.limbs for _, _, c in proofs])
    neg = e.g1_add_batch(np.tile(G1.zero().limbs, (1 + 2 * m, 1)), np.concatenate([vk.alpha_g1.limbs[None], L, C]), negate_b=True)
    P = np.empty((m, 4, G1_WORDS), np.uint64); Q = np.empty((m, 4, G2_WORDS), np.uint64)
    P[:, 0] = np.stack([a.limbs for a, _, _ in proofs]); Q[:, 0] = np.stack([b.limbs for _, b, _ in proofs])
    P[:, 1] = neg[0]; Q[:, 1] = vk.beta_g2.limbs
    P[:, 2] = neg[1:1 + m]; Q[:, 2] = vk.gamma_g2.limbs
    P[:, 3] = neg[1 + m:]; Q[:, 3] = vk.delta_g2.limbs
    if prepared:
        q_index = np.empty((m, 4), np.uint64)
        q_index[:, 0] = 3 + np.arange(m, dtype=np.uint64); q_index[:, 1:] = np.arange(3, dtype=np.uint64)
        h = e.g2_prepare(np.concatenate([vk.beta_g2.limbs[None], vk.gamma_g2.limbs[None], vk.delta_g2.limbs[None], Q[:, 0]]))
        try:
            out = e.pairing_product_batch_prepared_native(P.reshape(-1, G1_WORDS), h, np.arange(m + 1, dtype=np.uint64) * 4, q_index.reshape(-1))
        finally:
            h.close()
        return (out == Gt.one().limbs).all(axis=1)
    return pairing_check_batch(P.reshape(-1, G1_WORDS), Q.reshape(-1, G2_WORDS), offsets=np.arange(m + 1, dtype=np.uint64) * 4, engine=e)


def _block_args(vk, proofs, public_inputs):
    proofs = list(proofs); public_inputs = [list(a) for a in public_inputs]
    m, l = len(proofs), len(vk.ic) - 1
    if len(public_inputs) != m:
        raise ValueError(f"{m} proofs but {len(public_inputs)} sets of public inputs")
    if any(len(a) != l for a in public_inputs):
        raise ValueError(f"every proof takes {l} public inputs (len(vk.ic) - 1)")
    return proofs, public_inputs, m, l


def verify_aggregate(vk, proofs, public_inputs, engine=None, rng=None):
    """ONE bool for the whole block: with random 128-bit r_j,
        prod_j [e(A_j, B_j) e(-alpha, beta) e(-L_j, gamma) e(-C_j, delta)]^(r_j) == 1
    evaluated as the multi-pairing  prod_j e(r_j A_j, B_j) * e(-(sum r_j) alpha, beta) * e(-sum_j r_j L_j, gamma) * e(-sum_j r_j C_j, delta):
    m + 3 Miller loops and one final exponentiation where verify_batch runs 4 m and m.  The scaled A_j are one g1_mul_batch, the products
    r_j * a_ji (a_j0 = 1) one fr_mul_batch, the three sums one g1_msm_batch of three segments, their negation one g1_add_batch.
    A block that holds a bad proof is accepted with probability about 2^-128 (the r_j are drawn from `secrets`); the answer does not say
    WHICH proof failed - verify_batch does.  rng: tests only - an object with .bytes(n) (numpy Generator) that makes the r_j reproducible.
    An empty block is True.  Arguments as for verify_batch, and rejected like there before any device call."""
    proofs, public_inputs, m, l = _block_args(vk, proofs, public_inputs)
    if m == 0:
        return True
    e = engine or default_engine()
    draw = (lambda: int.from_bytes(rng.bytes(16), "little")) if rng is not None else (lambda: secrets.randbits(128))
    r = [Fr(draw()) for _ in range(m)]
    R = np.stack([x.limbs for x in r])
    A = e.g1_mul_batch(np.stack([a.limbs for a, _, _ in proofs]), R)
    one = Fr.one().limbs
    inputs = np.stack([one if i == 0 else a[i - 1].limbs for a in public_inputs for i in range(l + 1)])
    ra = e.fr_mul_batch(np.repeat(R, l + 1, axis=0), inputs)
    ic = np.stack([p.limbs for p in vk.ic])
    C = np.stack([c.limbs for _, _, c in proofs])
    rsum = Fr(sum(x.v for x in r) % R_MOD).limbs
    n1 = m * (l + 1)
    sums = e.g1_msm_batch(np.concatenate([vk.alpha_g1.limbs[None], np.tile(ic, (m, 1)), C]), np.concatenate([rsum[None], ra, R]),
                          np.array([0, 1, 1 + n1, 1 + n1 + m], np.uint64))
    neg = e.g1_add_batch(np.tile(G1.zero().limbs, (3, 1)), sums, negate_b=True)
    P = np.concatenate([A, neg])
    Q = np.concatenate([np.stack([b.limbs for _, b, _ in proofs]), vk.beta_g2.limbs[None], vk.gamma_g2.limbs[None], vk.delta_g2.limbs[None]])
    return bool(np.array_equal(e.pairing_product(P, Q), Gt.one().limbs))
