"""The sumcheck protocol over BN254's Fr on the GPU, from bn_amd.fr_sumcheck_round and bn_amd.fr_mle_fold: the interactive proof that
    claim = sum over x in {0,1}^nv of  sum_c coeff_c * prod_{j in group c} T_j(x)
for multilinear tables T_0 .. T_{k-1} (bn_amd.mle), made non-interactive with a hash transcript - the core of Spartan, HyperPlonk, GKR and
lookup arguments.  Round s (from 0) binds variable nv - 1 - s: the prover sends the values at t = 0 .. degree of
    g_s(t) = sum over the remaining hypercube of the same expression with that variable set to t,
the verifier checks g_s(0) + g_s(1) against the running value (the claim at first), draws r_s, and moves the running value to g_s(r_s).  After
nv rounds the running value must be the expression at the tables' values at the point, point[j] = r_{nv-1-j}; the prover sends those k
values (`finals`) and the CALLER checks them against their own commitments or tables (mle.evaluate) - verify only checks that they fit.
Against commitments that check is bn_amd.mkzg: the prover opens every committed table at the point (mkzg.open) and the verifier accepts
finals[j] with mkzg.verify against the commitment of table j.

prove uses the host-buffer calls, as kzg and groth16 do: the tables go up once per round for the round polynomial and once for the fold,
halving every round - about four times their bytes in total over a proof, twice per call kind.  prove_resident is the resident prover, on
ONE device buffer: the tables go up once, round 0 is Engine.fr_sumcheck_round_dev, every later round ONE Engine.fr_sumcheck_fold_round_dev in place
- the fused fold-then-round call, which folds by the challenge just drawn and sums the next round polynomial in one pass over the tables -
and one Engine.fr_mle_fold_dev leaves the finals; per round only degree + 1 records come down.  Same proof, byte for byte.
Measured at nv = 20 over four tables at degree 3 (tools/time_fold_round.py, profiles/r20_fold_round.txt; medians of 5): prove_resident takes
3.49 ms of kernel time and 7.3 ms of wall time, the same loop with the two _dev calls per round 7.00 and 10.5 ms, prove 7.12 and 146 ms.  The
rule fixed before measuring - the fused call ships if the [min, max] of its whole-proof kernel time lies wholly below the two-call loop's -
came out for the fused call (2.01 x).  The gain is in the small rounds, where the fused call takes 4 indices per lane instead of the round's
fixed 16 and is one launch fewer (2.0 to 2.2 x from 2^16 to 2^20 entries); on tables of 2^22 entries it is 0.92 x the two calls: it runs at
1.31 x the plain batched product on its products, so there the tables' second trip was never the cost.
Not built: folding inside the factor walk of the fused fold-then-round call (the folded records would not come back through the cache, for
two more products per factor occurrence), a factored eq table (low bits times high bits, as the transform's twiddles), a device-side
transcript."""
import collections
import hashlib

import numpy as np

from .api import Fr, R_MOD, _scalar_array, default_engine
from .engine import _sumcheck_args

Proof = collections.namedtuple("Proof", "claim rounds finals")
Proof.__doc__ = "claim: the sum, an Fr; rounds: nv lists of degree + 1 Fr, g_s(0) .. g_s(degree); finals: the k tables' values at the point"


class Transcript:
    """A hash chain over hashlib.sha256 with a 32-byte state.  The exact bytes:
        start       state = SHA256(label)                                    label: the UTF-8 bytes of the string (bytes are taken as they are)
        absorb(xs)  state = SHA256(state || be(x_0) || be(x_1) || ..)        be(x): the canonical integer of the Fr x as 32 bytes, big endian
        challenge() r = Fr.interpret(SHA256(state || 0x00) || SHA256(state || 0x01))   the 64 bytes as a big-endian integer mod r (lib.rs:27-29)
                    state = SHA256(state || 0x02)                            then the state ratchets, so two draws in a row differ
    Small integers (sizes, table numbers) are absorbed as the Fr of that value."""

    def __init__(self, label):
        self.state = hashlib.sha256(label if isinstance(label, bytes) else label.encode()).digest()

    def absorb(self, frs):
        self.state = hashlib.sha256(self.state + b"".join(x.v.to_bytes(32, "big") for x in frs)).digest()

    def challenge(self):
        r = Fr.interpret(hashlib.sha256(self.state + b"\x00").digest() + hashlib.sha256(self.state + b"\x01").digest())
        self.state = hashlib.sha256(self.state + b"\x02").digest()
        return r


def _groups(groups):
    """[(Fr coefficient, [table numbers])] and the degree: the longest group"""
    gs = [(c if isinstance(c, Fr) else Fr.from_limbs(c), [int(j) for j in m]) for c, m in groups]
    if not gs or any(not m for _, m in gs):
        raise ValueError("groups needs at least one product, each of at least one table")
    return gs, max(len(m) for _, m in gs)


def _absorb_statement(tr, nv, k, degree, gs, claim):
    tr.absorb([Fr(nv), Fr(k), Fr(degree), Fr(len(gs))])
    for c, m in gs:
        tr.absorb([c, Fr(len(m))] + [Fr(j) for j in m])
    tr.absorb([claim])


def prove(tables, groups, transcript=None, engine=None):
    """(Proof(claim, rounds, finals), point) for the sum over the hypercube of sum_c coeff_c * prod_{j in group c} T_j.  tables: a sequence of k
    tables of n = 2^nv Fr each (nv >= 1), or an (n, k, 4) uint64 array with table j at index i in [i, j]; groups: a list of (coeff, [table
    numbers]).  The transcript (default Transcript("bn_amd.sumcheck")) absorbs nv, k, the degree, the groups and the claim; per round ONE
    fr_sumcheck_round, whose degree + 1 values are absorbed, a challenge r, and ONE fr_mle_fold of the whole (n, k) array by r.  claim is
    out[0] + out[1] of round 0; finals are the k records left at the end; point[j] is the challenge of round nv - 1 - j.
    Host-buffer calls: see the module's docstring for what that moves and what a resident prover looks like."""
    if not isinstance(tables, np.ndarray):
        tables = np.stack([_scalar_array(t) for t in tables], axis=1)
    gs, degree = _groups(groups)
    T, _, _, _, degree = _sumcheck_args(tables, [(c.limbs, m) for c, m in gs], degree)
    n, k = T.shape[0], T.shape[1]
    nv = n.bit_length() - 1
    if n != 1 << nv:
        raise ValueError(f"tables hold {n} indices: a power of two is needed")
    e = engine or default_engine()
    tr = transcript or Transcript("bn_amd.sumcheck")
    limb_groups = [(c.limbs, m) for c, m in gs]
    rounds, challenges, claim = [], [], None
    for s in range(nv):
        g = [Fr.from_limbs(r) for r in e.fr_sumcheck_round(T, limb_groups, degree)]
        if s == 0:
            claim = g[0] + g[1]
            _absorb_statement(tr, nv, k, degree, gs, claim)
        tr.absorb(g)
        r = tr.challenge()
        T = e.fr_mle_fold(T, r.limbs)
        rounds.append(g); challenges.append(r)
    return Proof(claim, rounds, [Fr.from_limbs(x) for x in T[0]]), challenges[::-1]


# What prove_resident runs between two challenges: the fused bn254_fr_sumcheck_fold_round_dev, or bn254_fr_mle_fold_dev in place followed by
# bn254_fr_sumcheck_round_dev.  The rule was fixed before measuring (tools/time_fold_round.py, profiles/r20_fold_round.txt): the fused call if
# the [min, max] of its whole-proof kernel time at nv = 20 lies wholly below that of the two-call loop.  It does: 3.49 ms [3.43 3.57]
# against 7.00 ms [6.86 7.05].
FUSED = True


def prove_resident(tables, groups, transcript=None, engine=None):
    """prove on ONE device buffer: the same arguments, the same (Proof, point), byte for byte, for the same transcript.  The (n, k) array goes up
    once, into a torch tensor on the engine's device that also holds the degree + 1 records of a round; round 0 is fr_sumcheck_round_dev,
    rounds 1 .. nv - 1 are fr_sumcheck_fold_round_dev in place (the fold by the challenge just drawn and the next round polynomial in one pass
    - or, with FUSED off, fr_mle_fold_dev in place and fr_sumcheck_round_dev), and one fr_mle_fold_dev leaves the finals.  Per round only the
    degree + 1 records the transcript absorbs come down."""
    return _prove_resident(tables, groups, transcript, engine, FUSED)


def _prove_resident(tables, groups, transcript, engine, fused):
    import torch
    if not isinstance(tables, np.ndarray):
        tables = np.stack([_scalar_array(t) for t in tables], axis=1)
    gs, degree = _groups(groups)
    limb_groups = [(c.limbs, m) for c, m in gs]
    T, _, _, _, degree = _sumcheck_args(tables, limb_groups, degree)
    n, k = T.shape[0], T.shape[1]
    nv = n.bit_length() - 1
    if n != 1 << nv:
        raise ValueError(f"tables hold {n} indices: a power of two is needed")
    e = engine or default_engine()
    tr = transcript or Transcript("bn_amd.sumcheck")
    dev = torch.device("cuda", e.device)
    buf = torch.empty((n * k + degree + 1) * 4, dtype=torch.int64, device=dev)          # the tables, then the records of a round
    buf[:n * k * 4].copy_(torch.from_numpy(T.reshape(-1).view(np.int64)))
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_tables, d_out = buf.data_ptr(), buf.data_ptr() + 32 * n * k

    def down(first, count):
        """records [first, first + count) of the buffer as Fr; the copy is ordered on the stream and waits for it"""
        words = buf[first * 4:(first + count) * 4].cpu().numpy().view(np.uint64).reshape(count, 4)
        return [Fr.from_limbs(x) for x in words]

    e.fr_sumcheck_round_dev(d_tables, n, k, limb_groups, d_out, degree, stream)
    g = down(n * k, degree + 1)
    claim = g[0] + g[1]
    _absorb_statement(tr, nv, k, degree, gs, claim)
    rounds, challenges = [], []
    for s in range(nv):
        tr.absorb(g)
        r = tr.challenge()
        rounds.append(g); challenges.append(r)
        rows = n >> s                                                                    # before the fold by r
        if s == nv - 1:
            e.fr_mle_fold_dev(d_tables, rows * k, r.limbs, d_tables, stream)
        elif fused:
            e.fr_sumcheck_fold_round_dev(d_tables, rows, k, r.limbs, limb_groups, d_tables, d_out, degree, stream)
        else:
            e.fr_mle_fold_dev(d_tables, rows * k, r.limbs, d_tables, stream)
            e.fr_sumcheck_round_dev(d_tables, rows // 2, k, limb_groups, d_out, degree, stream)
        if s < nv - 1:
            g = down(n * k, degree + 1)
    return Proof(claim, rounds, down(0, k)), challenges[::-1]


def _at(values, r):
    """the polynomial of degree len(values) - 1 through (t, values[t]) at r, by Lagrange interpolation over 0 .. d, in integers"""
    d = len(values) - 1
    total = 0
    for t, y in enumerate(values):
        num = den = 1
        for u in range(d + 1):
            if u != t:
                num = num * (r.v - u) % R_MOD
                den = den * (t - u) % R_MOD
        total = (total + y.v * num * pow(den, -1, R_MOD)) % R_MOD
    return Fr(total)


def verify(proof, nv, groups, transcript=None):
    """(ok, point): host integer arithmetic only.  Every round's g_s(0) + g_s(1) must equal the running value (first the claim), which moves to
    g_s(r_s) by interpolation over 0 .. degree; the last must equal sum_c coeff_c * prod_{j in group c} finals[j].  The transcript must start
    as the prover's did.  point[j] is the challenge of round nv - 1 - j: the caller checks proof.finals against their own commitments or
    tables there (mle.evaluate) - without that check nothing ties the proof to any tables."""
    gs, degree = _groups(groups)
    k = len(proof.finals)
    ok = len(proof.rounds) == nv and all(len(g) == degree + 1 for g in proof.rounds) and all(0 <= j < k for _, m in gs for j in m)
    if not ok:
        return False, None
    tr = transcript or Transcript("bn_amd.sumcheck")
    _absorb_statement(tr, nv, k, degree, gs, proof.claim)
    running, challenges = proof.claim, []
    for g in proof.rounds:
        ok = ok and g[0] + g[1] == running
        tr.absorb(g)
        r = tr.challenge()
        running = _at(g, r)
        challenges.append(r)
    last = Fr.zero()
    for c, m in gs:
        term = c
        for j in m:
            term = term * proof.finals[j]
        last = last + term
    return ok and last == running, challenges[::-1]
