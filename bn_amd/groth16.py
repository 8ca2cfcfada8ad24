"""Groth16 verification of a block of proofs under one verifying key, on the GPU.

A proof (A: G1, B: G2, C: G1) with public inputs a_1 .. a_l is valid when
    e(A, B) = e(alpha, beta) * e(L, gamma) * e(C, delta),        L = IC[0] + sum a_i * IC[i]
which is checked as  e(A, B) * e(-alpha, beta) * e(-L, gamma) * e(-C, delta) == 1.  A block takes three calls: one segmented multi-scalar
multiplication for every L (bn_amd.g1_msm_batch, segment j: IC[0] * 1, IC[i] * a_ji), one batched subtraction for the negations and one
batched multi-pairing check (bn_amd.pairing_check_batch, four pairs per proof)."""
import collections

import numpy as np

from .api import Fr, G1, default_engine, pairing_check_batch
from .engine import G1_WORDS, G2_WORDS

VerifyingKey = collections.namedtuple("VerifyingKey", "alpha_g1 beta_g2 gamma_g2 delta_g2 ic")
VerifyingKey.__doc__ = "alpha_g1: G1; beta_g2, gamma_g2, delta_g2: G2; ic: l + 1 G1 points for l public inputs"


def verify_batch(vk, proofs, public_inputs, engine=None):
    """numpy bool array, one entry per proof.  proofs: sequence of (A: G1, B: G2, C: G1); public_inputs: one sequence of l = len(vk.ic) - 1
    Fr per proof."""
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
    return pairing_check_batch(P.reshape(-1, G1_WORDS), Q.reshape(-1, G2_WORDS), offsets=np.arange(m + 1, dtype=np.uint64) * 4, engine=e)
