"""BLS signatures over BN254 in the min-pubkey layout: public keys in G1, signatures in G2 (bn_amd.bls is the other way round).

    pk = G1::one() * sk,   sig = H(m) * sk,   verify:  e(pk, H(m)) * e(-G1::one(), sig) == 1

H is hash_to_curve of RFC 9380 into G2 (Shallue-van de Woestijne map over Fq2, SHA-256 XMD to 192 bytes; bn_amd.hash_to_curve) followed by the
cofactor clearing [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P), under the tag DST.  The map's constants were derived from the RFC's formulas and
the clearing is the one step the RFC defines no suite for: neither the constants nor the outputs are checked against gnark-crypto or any other
library, so signatures made here are not promised to verify elsewhere.  Every function is a fixed, small number of engine calls whatever the
batch size: hashing is one call (on the device for messages of one length), the pairings one call.  H(m) is in G2, so signing may take the GLS
multiplication.  Points travel as bn_amd.G1 / G2 or as (n,12) / (n,24) uint64 arrays; messages as a sequence of bytes or an (n, msg_len) uint8
array.  Not built: proofs of possession themselves, multi-GPU forms."""
import numpy as np

from . import api
from .api import Fr, G1, G2, Gt
from .hash_to_curve import BLS_G2_DST

DST = BLS_G2_DST


def _engine(engine):
    return engine or api.default_engine()


def _count(msgs):
    return msgs.shape[0] if isinstance(msgs, np.ndarray) else len(msgs)


def _is_one(gt_limbs):
    return (np.asarray(gt_limbs).reshape(-1, Gt.one().limbs.size) == Gt.one().limbs).all(axis=1)


def _neg_g1_one():
    """-G1::one() = (1, -2, 1): a constant, so verifying needs no addition call"""
    return np.concatenate([api._one_fq(), api._mont(api.Q_MOD - 2, api.Q_MOD), api._one_fq()])


def keygen(rng):
    """(sk, pk): sk a uniform Fr from rng (a numpy Generator), pk = G1::one() * sk"""
    sk = Fr.random(rng)
    return sk, public_keys([sk])[0]


def public_keys(sks, engine=None):
    """[G1::one() * sk for sk in sks]: one fixed-base call"""
    return [G1(r) for r in _engine(engine).g1_mul_base_batch(G1.one().limbs, api._scalar_array(sks))]


def sign_batch(sks, msgs, dst=DST, engine=None):
    """[H(m) * sk]: one hash call and one scalar-multiplication call"""
    k = api._scalar_array(sks)
    if k.shape[0] != _count(msgs):
        raise ValueError("as many messages as secret keys")
    if k.shape[0] == 0:
        return []
    e = _engine(engine)
    h = api._g2_hash_to_curve_limbs(msgs, dst, e)
    return [G2(r) for r in e.g2_mul_batch(h, k)]


def sign(sk, msg, dst=DST, engine=None):
    return sign_batch([sk], [msg], dst, engine)[0]


def verify_batch(pks, msgs, sigs, dst=DST, engine=None, validate=False):
    """numpy bool array: entry i holds iff e(pks[i], H(msgs[i])) e(-G1::one(), sigs[i]) == 1.  One hash call and one batched pairing check of
    two-pair segments (the negated generator is a constant).  Keys and signatures are TRUSTED to be valid points - a signature outside the
    order-r subgroup of the twist makes the check meaningless - unless validate=True: then one validation call per group comes first, and a
    row whose key or signature is not a valid point, or whose key is the point at infinity, is False (its points are replaced by the
    generators for the pairing call; the other rows are unaffected)."""
    pk = api._point_array(G1, pks); sg = api._point_array(G2, sigs)
    n = _count(msgs)
    if pk.shape[0] != n or sg.shape[0] != n:
        raise ValueError("as many public keys and signatures as messages")
    if n == 0:
        return np.zeros(0, bool)
    e = _engine(engine)
    valid = None
    if validate:
        valid = api._valid_rows(e, pk, sg, pk)
        pk = np.where(valid[:, None], pk, G1.one().limbs); sg = np.where(valid[:, None], sg, G2.one().limbs)
    h = api._g2_hash_to_curve_limbs(msgs, dst, e)
    P = np.empty((2 * n, G1.WORDS), np.uint64); P[0::2] = pk; P[1::2] = _neg_g1_one()
    Q = np.empty((2 * n, G2.WORDS), np.uint64); Q[0::2] = h; Q[1::2] = sg
    ok = api.pairing_check_batch(P, Q, np.arange(0, 2 * n + 1, 2, dtype=np.uint64), engine=e)
    return ok if valid is None else ok & valid


def verify(pk, msg, sig, dst=DST, engine=None):
    return bool(verify_batch([pk], [msg], [sig], dst, engine)[0])


def aggregate(sigs, engine=None):
    """the sum of the signatures, normalised: one multi-scalar multiplication with every scalar one"""
    sg = api._point_array(G2, sigs)
    return G2(_engine(engine).g2_msm(sg, np.tile(Fr.one().limbs, (sg.shape[0], 1))))


def _sig_row(sig):
    return np.asarray(sig.limbs if isinstance(sig, G2) else sig, np.uint64).reshape(1, G2.WORDS)


def verify_aggregate(pks, msgs, sig, dst=DST, engine=None):
    """e(pk_1, H(m_1)) .. e(pk_k, H(m_k)) e(-G1::one(), sig) == 1 for an aggregate over DISTINCT messages: a repeated message raises
    ValueError before any device call (equal messages need proofs of possession: fast_aggregate_verify).  One hash call and one pairing
    product of k + 1 pairs."""
    keys = [bytes(m) for m in msgs] if not isinstance(msgs, np.ndarray) else [m.tobytes() for m in msgs]
    if len(set(keys)) != len(keys):
        raise ValueError("verify_aggregate needs distinct messages")
    pk = api._point_array(G1, pks)
    if pk.shape[0] != len(keys):
        raise ValueError("as many public keys as messages")
    if not keys:
        return False
    e = _engine(engine)
    h = api._g2_hash_to_curve_limbs(msgs, dst, e)
    return bool(_is_one(e.pairing_product(np.concatenate([pk, _neg_g1_one()[None, :]]), np.concatenate([h, _sig_row(sig)])))[0])


def fast_aggregate_verify(pks, msg, sig, dst=DST, engine=None):
    """every key signed the SAME message: e(pk_1 + .. + pk_k, H(m)) e(-G1::one(), sig) == 1.  Sound only for keys with proofs of possession
    (a rogue key cancels the others otherwise); checking those is the caller's business.  One multi-scalar multiplication over the keys, one
    hash call and one pairing product of two pairs."""
    pk = api._point_array(G1, pks)
    if pk.shape[0] == 0:
        return False
    e = _engine(engine)
    apk = e.g1_msm(pk, np.tile(Fr.one().limbs, (pk.shape[0], 1)))
    h = api._g2_hash_to_curve_limbs([msg], dst, e)
    return bool(_is_one(e.pairing_product(np.stack([np.asarray(apk, np.uint64).reshape(-1), _neg_g1_one()]), np.concatenate([h, _sig_row(sig)])))[0])
