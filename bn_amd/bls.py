"""BLS signatures over BN254 in the min-signature layout EIP-197 verifiers use: signatures in G1, public keys in G2.

    pk = G2::one() * sk,   sig = H(m) * sk,   verify:  e(H(m), pk) * e(-sig, G2::one()) == 1

H is hash_to_curve of RFC 9380 for G1 (Shallue-van de Woestijne map, SHA-256 XMD; bn_amd.hash_to_curve) under the tag DST.  The map's constants
were derived from the RFC's formulas and are not checked against gnark-crypto or any other library, so signatures made here are not promised to
verify elsewhere.  Every function is a fixed, small number of engine calls whatever the batch size: hashing is one call (on the device for
messages of one length), the pairings one call.  Points travel as bn_amd.G1 / G2 or as (n,12) / (n,24) uint64 arrays; messages as a sequence of
bytes or an (n, msg_len) uint8 array.  The min-pubkey layout (keys in G1, hash to G2) is bn_amd.bls_minpk.  Not built: proofs of possession themselves, multi-GPU forms."""
import numpy as np

from . import api
from .api import Fr, G1, G2, Gt
from .hash_to_curve import BLS_DST

DST = BLS_DST


def _engine(engine):
    return engine or api.default_engine()


def _count(msgs):
    return msgs.shape[0] if isinstance(msgs, np.ndarray) else len(msgs)


def _is_one(gt_limbs):
    return (np.asarray(gt_limbs).reshape(-1, Gt.one().limbs.size) == Gt.one().limbs).all(axis=1)


def keygen(rng):
    """(sk, pk): sk a uniform Fr from rng (a numpy Generator), pk = G2::one() * sk"""
    sk = Fr.random(rng)
    return sk, public_keys([sk])[0]


def public_keys(sks, engine=None):
    """[G2::one() * sk for sk in sks]: one fixed-base call"""
    return [G2(r) for r in _engine(engine).g2_mul_base_batch(G2.one().limbs, api._scalar_array(sks))]


def sign_batch(sks, msgs, dst=DST, engine=None):
    """[H(m) * sk]: one hash call and one scalar-multiplication call"""
    k = api._scalar_array(sks)
    if k.shape[0] != _count(msgs):
        raise ValueError("as many messages as secret keys")
    if k.shape[0] == 0:
        return []
    e = _engine(engine)
    h = api._hash_to_curve_limbs(msgs, dst, e)
    return [G1(r) for r in e.g1_mul_batch(h, k)]


def sign(sk, msg, dst=DST, engine=None):
    return sign_batch([sk], [msg], dst, engine)[0]


def verify_batch(pks, msgs, sigs, dst=DST, engine=None, validate=False):
    """numpy bool array: entry i holds iff e(H(msgs[i]), pks[i]) e(-sigs[i], G2::one()) == 1.  One hash call, one addition call (the negated
    signatures) and one batched pairing check of two-pair segments.  Keys and signatures are TRUSTED to be valid points - a key outside the
    order-r subgroup of the twist makes the check meaningless - unless validate=True: then one validation call per group comes first, and a
    row whose key or signature is not a valid point, or whose key is the point at infinity, is False (its points are replaced by the
    generators for the pairing call; the other rows are unaffected)."""
    pk = api._point_array(G2, pks); sg = api._point_array(G1, sigs)
    n = _count(msgs)
    if pk.shape[0] != n or sg.shape[0] != n:
        raise ValueError("as many public keys and signatures as messages")
    if n == 0:
        return np.zeros(0, bool)
    e = _engine(engine)
    valid = None
    if validate:
        valid = api._valid_rows(e, sg, pk, pk)
        pk = np.where(valid[:, None], pk, G2.one().limbs); sg = np.where(valid[:, None], sg, G1.one().limbs)
    h = api._hash_to_curve_limbs(msgs, dst, e)
    neg = e.g1_add_batch(np.tile(G1.zero().limbs, (n, 1)), sg, negate_b=True)
    P = np.empty((2 * n, G1.WORDS), np.uint64); P[0::2] = h; P[1::2] = neg
    Q = np.empty((2 * n, G2.WORDS), np.uint64); Q[0::2] = pk; Q[1::2] = G2.one().limbs
    ok = api.pairing_check_batch(P, Q, np.arange(0, 2 * n + 1, 2, dtype=np.uint64), engine=e)
    return ok if valid is None else ok & valid


def verify(pk, msg, sig, dst=DST, engine=None):
    return bool(verify_batch([pk], [msg], [sig], dst, engine)[0])


def aggregate(sigs, engine=None):
    """the sum of the signatures, normalised: one multi-scalar multiplication with every scalar one"""
    sg = api._point_array(G1, sigs)
    return G1(_engine(engine).g1_msm(sg, np.tile(Fr.one().limbs, (sg.shape[0], 1))))


def verify_aggregate(pks, msgs, sig, dst=DST, engine=None):
    """e(H(m_1), pk_1) .. e(H(m_k), pk_k) e(-sig, G2::one()) == 1 for an aggregate over DISTINCT messages: a repeated message raises
    ValueError before any device call (equal messages need proofs of possession: fast_aggregate_verify).  One hash call and one pairing
    product of k + 1 pairs."""
    keys = [bytes(m) for m in msgs] if not isinstance(msgs, np.ndarray) else [m.tobytes() for m in msgs]
    if len(set(keys)) != len(keys):
        raise ValueError("verify_aggregate needs distinct messages")
    pk = api._point_array(G2, pks)
    if pk.shape[0] != len(keys):
        raise ValueError("as many public keys as messages")
    if not keys:
        return False
    e = _engine(engine)
    h = api._hash_to_curve_limbs(msgs, dst, e)
    s = np.asarray(sig.limbs if isinstance(sig, G1) else sig, np.uint64).reshape(1, G1.WORDS).copy()
    s[0, 4:8] = _neg_fq_limbs(s[0, 4:8])
    return bool(_is_one(e.pairing_product(np.concatenate([h, s]), np.concatenate([pk, G2.one().limbs[None, :]])))[0])


def fast_aggregate_verify(pks, msg, sig, dst=DST, engine=None):
    """every key signed the SAME message: e(H(m), pk_1 + .. + pk_k) e(-sig, G2::one()) == 1.  Sound only for keys with proofs of possession
    (a rogue key cancels the others otherwise); checking those is the caller's business.  One multi-scalar multiplication over the keys, one
    hash call and one pairing product of two pairs."""
    pk = api._point_array(G2, pks)
    if pk.shape[0] == 0:
        return False
    e = _engine(engine)
    apk = e.g2_msm(pk, np.tile(Fr.one().limbs, (pk.shape[0], 1)))
    h = api._hash_to_curve_limbs([msg], dst, e)
    s = np.asarray(sig.limbs if isinstance(sig, G1) else sig, np.uint64).reshape(1, G1.WORDS).copy()
    s[0, 4:8] = _neg_fq_limbs(s[0, 4:8])
    return bool(_is_one(e.pairing_product(np.concatenate([h, s]), np.stack([np.asarray(apk, np.uint64).reshape(-1), G2.one().limbs])))[0])


def _neg_fq_limbs(y):
    """-y of a canonical Montgomery image (four uint64 words) on the host: one point, no device call"""
    v = sum(int(x) << (64 * i) for i, x in enumerate(y))
    return api._limbs(-v % api.Q_MOD)
