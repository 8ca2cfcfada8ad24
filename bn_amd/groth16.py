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

from . import poly
from .api import Fr, G1, G2, Gt, R_MOD, _scalar_array, default_engine, pairing_check_batch
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


def encode_proofs(proofs, format="ark", engine=None):
    """bytes: A | B | C per proof in the compressed layout `format` ("ark" or "gnark"), 32 + 64 + 32 = 128 bytes each - one G1 call over the
    2 m points A_0, C_0, A_1, ... and one G2 call"""
    e = engine or default_engine()
    proofs = list(proofs)
    m = len(proofs)
    if m == 0:
        return b""
    ac = e.g1_compress_batch(np.stack([p.limbs for a, _, c in proofs for p in (a, c)]), format).reshape(m, 2, 32)
    b = e.g2_compress_batch(np.stack([b.limbs for _, b, _ in proofs]), format)
    return np.concatenate([ac[:, 0], b, ac[:, 1]], axis=1).tobytes()


def decode_proofs(blob, format="ark", engine=None):
    """(proofs, status): the proofs of encode_proofs' bytes as (A: G1, B: G2, C: G1) and an (m, 3) int32 array of the decoder's statuses for A,
    B, C (0 ok, 3 flags, 1 range, 4 no such point, 5 not in the subgroup); a rejected point is the group's zero.  ValueError unless the blob is
    whole 128-byte records."""
    e = engine or default_engine()
    raw = np.frombuffer(bytes(blob), np.uint8)
    if raw.size % 128:
        raise ValueError(f"{raw.size} bytes are not whole proofs of 128")
    rec = raw.reshape(-1, 128)
    m = rec.shape[0]
    if m == 0:
        return [], np.zeros((0, 3), np.int32)
    ac, st_ac = e.g1_decompress_batch(np.ascontiguousarray(rec[:, [*range(32), *range(96, 128)]]).reshape(2 * m, 32), format)
    b, st_b = e.g2_decompress_batch(np.ascontiguousarray(rec[:, 32:96]), format)
    st_ac = st_ac.reshape(m, 2)
    status = np.stack([st_ac[:, 0], st_b, st_ac[:, 1]], axis=1).astype(np.int32)
    return [(G1(ac[2 * j]), G2(b[j]), G1(ac[2 * j + 1])) for j in range(m)], status


def verify_batch_compressed(vk, blob, public_inputs, format="ark", engine=None, prepared=False):
    """verify_batch over encode_proofs' bytes: the proofs are decompressed on the device (two calls), verified, and a proof with any non-zero
    decode status is False whatever the pairing check of its zeroed points says"""
    proofs, status = decode_proofs(blob, format, engine=engine)
    ok = verify_batch(vk, proofs, public_inputs, engine=engine, prepared=prepared)
    return ok & (status == 0).all(axis=1)


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


# ---- proving: a rank-1 constraint system, its witness map, a development setup and the prover, from calls the engine already has
R1CS = collections.namedtuple("R1CS", "num_public num_variables a b c")
R1CS.__doc__ = """num_public: l public inputs; num_variables: columns, the length of z = (1, public_1 .. public_l, private ...) with z[0] = 1;
a, b, c: the three matrices, each a CSR triple (offsets, index, coeff) over num_variables columns - offsets of rows + 1 entries, index and coeff
(Fr values or an (nnz,4) uint64 array) of offsets[rows] entries - with the same number of rows.  z satisfies the system when
(a z)[j] * (b z)[j] == (c z)[j] for every row j."""
ProvingKey = collections.namedtuple("ProvingKey", "alpha_g1 beta_g1 beta_g2 delta_g1 delta_g2 a_query b_g1_query b_g2_query l_query h_query")
ProvingKey.__doc__ = """alpha_g1, beta_g1, delta_g1: G1; beta_g2, delta_g2: G2; the queries are normalized points as uint64 arrays, ready for
the multi-scalar multiplications: a_query (num_variables, 12) = u_i(tau) G1, b_g1_query (num_variables, 12) and b_g2_query (num_variables, 24)
= v_i(tau) G, l_query (num_variables - l - 1, 12) = ((beta u_i + alpha v_i + w_i) / delta) G1 for the private variables, h_query (n - 1, 12) =
(tau^k (tau^n - 1) / delta) G1 with n the domain size."""
_MONT = (1 << 256) % R_MOD
_M64 = (1 << 64) - 1


def _limbs(values):
    """integers mod r -> (len, 4) uint64 Montgomery images"""
    out = np.zeros((len(values), 4), np.uint64)
    for i, v in enumerate(values):
        m = v % R_MOD * _MONT % R_MOD
        out[i] = [(m >> (64 * j)) & _M64 for j in range(4)]
    return out


def _draw(rng):
    """one scalar from 64 bytes of rng (an object with .bytes(n), e.g. a numpy Generator): little endian, mod r"""
    return int.from_bytes(rng.bytes(64), "little") % R_MOD


def _matrices(r1cs):
    """the three CSR triples as arrays, checked: [(offsets uint64, index uint64, coeff (nnz,4))] and the common number of rows"""
    out = []
    nv = int(r1cs.num_variables)
    if not 0 <= int(r1cs.num_public) < nv:
        raise ValueError(f"{r1cs.num_public} public inputs do not fit {nv} variables (z[0] is the constant one)")
    for name, (offsets, index, coeff) in zip("abc", (r1cs.a, r1cs.b, r1cs.c)):
        o = np.asarray(offsets, np.uint64).reshape(-1)
        i = np.asarray(index, np.uint64).reshape(-1)
        c = _scalar_array(coeff)
        if o.size == 0 or int(o[0]) != 0 or bool((o[1:] < o[:-1]).any()) or int(o[-1]) != i.size or c.shape[0] != i.size:
            raise ValueError(f"matrix {name} is no CSR triple: offsets start at 0, never decrease and end at len(index) == len(coeff)")
        if i.size and int(i.max()) >= nv:
            raise ValueError(f"matrix {name} names column {int(i.max())} but the system has {nv} variables")
        out.append((o, i, c))
    rows = out[0][0].size - 1
    if any(o.size - 1 != rows for o, _, _ in out):
        raise ValueError("the three matrices differ in their number of rows")
    return out, rows


def _assignment(r1cs, z):
    Z = _scalar_array(z)
    if Z.shape[0] != int(r1cs.num_variables):
        raise ValueError(f"the assignment holds {Z.shape[0]} values but the system has {r1cs.num_variables} variables")
    if Z.shape[0] == 0 or not np.array_equal(Z[0], Fr.one().limbs):
        raise ValueError("z[0] is the constant one")
    return Z


def _stacked(mats):
    """three CSR matrices as one: the rows of b behind those of a, those of c behind b's"""
    offsets = [np.zeros(1, np.uint64)]
    at = 0
    for o, _, _ in mats:
        offsets.append(o[1:] + np.uint64(at))
        at += int(o[-1])
    return np.concatenate(offsets), np.concatenate([i for _, i, _ in mats]), np.concatenate([c for _, _, c in mats])


def _domain(rows):
    """log2 of the next power of two >= rows (at least 1: the quotient needs a domain)"""
    return max(1, (rows - 1).bit_length())


def witness_map(r1cs, z, engine=None):
    """(a_evals, b_evals, c_evals): the products A z, B z, C z of the three matrices with the assignment z (a sequence of Fr or a
    (num_variables, 4) uint64 array), each as an (n, 4) uint64 array padded with zero rows to the domain size n, the next power of two >= rows
    (0 * 0 = 0 keeps A B = C on the whole domain) - the evaluations poly.quotient takes.  The three matrices are stacked and run as ONE sparse
    matrix-vector product of 3 * rows segments.  ValueError, before any device call, for matrices that are no CSR triples over
    num_variables columns or differ in their rows, for len(z) != num_variables and for z[0] != 1."""
    mats, rows = _matrices(r1cs)
    Z = _assignment(r1cs, z)
    offsets, index, coeff = _stacked(mats)
    out = (engine or default_engine()).fr_dot_batch(coeff, Z, offsets, index)
    n = 1 << _domain(rows)
    evals = np.zeros((3, n, 4), np.uint64)
    evals[:, :rows] = out.reshape(3, rows, 4)
    return evals[0], evals[1], evals[2]


def _transposed(o, i, c, nv):
    """the CSR triple of the transposed matrix: nv rows whose indices are the rows of the original"""
    row_of = np.repeat(np.arange(o.size - 1, dtype=np.uint64), np.diff(o).astype(np.int64))
    order = np.argsort(i, kind="stable")
    counts = np.bincount(i.astype(np.int64), minlength=nv)
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(counts).astype(np.uint64)]), row_of[order], c[order]


def setup(r1cs, rng, engine=None):
    """(ProvingKey, VerifyingKey) of the system from a trapdoor (alpha, beta, gamma, delta, tau) drawn from rng - FOR TESTS AND DEVELOPMENT
    ONLY: whoever knows the trapdoor forges proofs, and this function knows it.  A ceremony that nobody can reconstruct is out of scope.
    rng: an object with .bytes(n) (a numpy Generator).  The five scalars are drawn in that order, each as 64 bytes little endian mod r, and
    drawn again while zero (tau: while tau^n == 1, where the domain's vanishing polynomial is zero).
    With n the domain size (the next power of two >= rows) and H its subgroup: the Lagrange values L_j(tau), j < n, are the inverse transform
    of (tau^k)_k, which are ONE scan (poly.powers); u_i(tau) = sum_j A[j,i] L_j(tau) and likewise v_i, w_i for B, C are ONE sparse matrix-vector product over the three
    transposed matrices (transposed with numpy on the host); the combinations (beta u_i + alpha v_i + w_i) / gamma for i <= l, / delta for
    i > l, and tau^k (tau^n - 1) / delta for k <= n - 2, are batched field arithmetic; every group element is a fixed-base multiple of the
    generator (one call per group)."""
    mats, rows = _matrices(r1cs)
    e = engine or default_engine()
    nv, l = int(r1cs.num_variables), int(r1cs.num_public)
    log_n = _domain(rows)
    n = 1 << log_n
    trap = []
    while len(trap) < 5:
        v = _draw(rng)
        if v and not (len(trap) == 4 and pow(v, n, R_MOD) == 1):
            trap.append(v)
    alpha, beta, gamma, delta, tau = trap
    P = poly.powers(Fr(tau), n, engine=e, limbs=True)
    lagrange = e.fr_ntt_batch(P, log_n, inverse=True)
    offsets, index, coeff = _stacked([_transposed(o, i, c, nv) for o, i, c in mats])
    uvw = e.fr_dot_batch(coeff, lagrange, offsets, index)
    u, v, w = uvw[:nv], uvw[nv:2 * nv], uvw[2 * nv:]
    scaled = e.fr_mul_batch(uvw[:2 * nv], np.repeat(_limbs([beta, alpha]), nv, axis=0))
    k = e.fr_add_batch(e.fr_add_batch(scaled[:nv], scaled[nv:]), w)
    inv_gamma, inv_delta = pow(gamma, -1, R_MOD), pow(delta, -1, R_MOD)
    t_over_delta = (pow(tau, n, R_MOD) - 1) * inv_delta % R_MOD
    tail = e.fr_mul_batch(np.concatenate([k, P[:n - 1]]),
                          np.concatenate([np.repeat(_limbs([inv_gamma, inv_delta]), [l + 1, nv - l - 1], axis=0), np.tile(_limbs([t_over_delta]), (n - 1, 1))]))
    g1 = e.g1_mul_base_batch(G1.one().limbs, np.concatenate([_limbs([alpha, beta, delta]), u, v, tail]))
    g2 = e.g2_mul_base_batch(G2.one().limbs, np.concatenate([_limbs([beta, gamma, delta]), v]))
    kq = g1[3 + 2 * nv:3 + 3 * nv]
    pk = ProvingKey(G1(g1[0]), G1(g1[1]), G2(g2[0]), G1(g1[2]), G2(g2[2]), g1[3:3 + nv], g1[3 + nv:3 + 2 * nv], g2[3:], kq[l + 1:], g1[3 + 3 * nv:])
    vk = VerifyingKey(G1(g1[0]), G2(g2[0]), G2(g2[1]), G2(g2[2]), [G1(r) for r in kq[:l + 1]])
    return pk, vk


PreparedProvingKey = collections.namedtuple("PreparedProvingKey", ProvingKey._fields + ("prepared",))
PreparedProvingKey.__doc__ = """a ProvingKey and `prepared`: the PreparedMSM handles of its five queries, a dict with the keys a_query,
b_g1_query, l_query, h_query (G1) and b_g2_query (G2).  prove() takes it wherever it takes the plain key and returns the same proof."""


def prepare_proving_key(pk, window_bits=None, engine=None):
    """ProvingKey -> PreparedProvingKey: the five queries go to the device once (Engine.g1_msm_prepare / g2_msm_prepare); every later
    prove() sends the scalars only.  The prepared key is used with the engine that prepared it."""
    e = engine or default_engine()
    prepared = {name: e.g1_msm_prepare(getattr(pk, name), window_bits) for name in ("a_query", "b_g1_query", "l_query", "h_query")}
    prepared["b_g2_query"] = e.g2_msm_prepare(pk.b_g2_query, window_bits)
    return PreparedProvingKey(*pk[:len(ProvingKey._fields)], prepared)


def _prepared_sums(e, prepared, Z, l, H):
    """the five sums of prove() against the handles of a prepared key: (sum_a, sum_b1, sum_l, sum_h, sum_b2)"""
    return (e.g1_msm_prepared(prepared["a_query"], Z), e.g1_msm_prepared(prepared["b_g1_query"], Z), e.g1_msm_prepared(prepared["l_query"], Z[l + 1:]),
            e.g1_msm_prepared(prepared["h_query"], H), e.g2_msm_prepared(prepared["b_g2_query"], Z))


def prove(pk, r1cs, z, rng, engine=None):
    """The proof (A: G1, B: G2, C: G1) that the prover knows an assignment z = (1, public_1 .. public_l, private ...) of the system, for the
    keys of setup(); verify_batch(vk, [proof], [z[1:l + 1]]) accepts it.  With h = poly.quotient(*witness_map(r1cs, z)) and r, s drawn from
    rng (in that order, 64 bytes each, little endian mod r):
        A = alpha + sum z_i a_query_i + r delta
        B = beta + sum z_i b_g2_query_i + s delta                          (in G2; the same sum in G1 is B1)
        C = sum_{i>l} z_i l_query_i + sum_k h_k h_query_k + s A + r B1 - r s delta
    The five sums are multi-scalar multiplications, four in G1 and one in G2 (pk may be a PreparedProvingKey: they then run against its handles); what remains - a handful of terms per output - is one segmented
    multi-scalar multiplication per group.  It is NOT checked that z satisfies the system: an assignment that does not yields a proof that
    does not verify (the quotient is then the quotient of nothing).  ValueError, before any device call, when len(z) != num_variables or
    z[0] != 1."""
    Z = _assignment(r1cs, z)
    e = engine or default_engine()
    l = int(r1cs.num_public)
    a_evals, b_evals, c_evals = witness_map(r1cs, Z, engine=e)
    h = poly.quotient(a_evals, b_evals, c_evals, engine=e)
    H = np.stack([x.limbs for x in h[:-1]])
    r, s = _draw(rng), _draw(rng)
    if getattr(pk, "prepared", None) is not None:
        sum_a, sum_b1, sum_l, sum_h, sum_b2 = _prepared_sums(e, pk.prepared, Z, l, H)
    else:
        sum_a, sum_b1 = e.g1_msm(pk.a_query, Z), e.g1_msm(pk.b_g1_query, Z)
        sum_l, sum_h = e.g1_msm(pk.l_query, Z[l + 1:]), e.g1_msm(pk.h_query, H)
        sum_b2 = e.g2_msm(pk.b_g2_query, Z)
    # s A + r B1 - r s delta = s alpha + s sum_a + r beta + r sum_b1 + r s delta
    points = np.stack([pk.alpha_g1.limbs, sum_a, pk.delta_g1.limbs,
                       sum_l, sum_h, pk.alpha_g1.limbs, sum_a, pk.beta_g1.limbs, sum_b1, pk.delta_g1.limbs])
    ac = e.g1_msm_batch(points, _limbs([1, 1, r, 1, 1, s, s, r, r, r * s]), np.array([0, 3, 10], np.uint64))
    b = e.g2_msm_batch(np.stack([pk.beta_g2.limbs, sum_b2, pk.delta_g2.limbs]), _limbs([1, 1, s]), np.array([0, 3], np.uint64))
    return G1(ac[0]), G2(b[0]), G1(ac[1])
