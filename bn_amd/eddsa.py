"""EdDSA-Poseidon on Baby Jubjub: the signature scheme of circomlib (eddsaposeidon.circom, circomlibjs' signPoseidon / verifyPoseidon), iden3
and the Hermez-style rollups, with the point arithmetic and the hash on the GPU.

    key      an integer secret s; the public key is A = [s]B8
    sign     R8 = [rho]B8,  hm = Poseidon5(R8.x, R8.y, A.x, A.y, M),  S = (rho + 8 hm s) mod l;  the signature is (R8, S)
    verify   R8 and A on the curve, S < l, [S]B8 == R8 + [8 hm]A - the scalar is the INTEGER 8 hm, not its value mod l, and there is NO subgroup
             check: A = O (or any A of small order) with R8 = [S]B8 verifies, exactly as in circomlib

circomlib's A is [key >> 3]B8 with S = rho + hm * key: the same equation with s = key >> 3 (key is a multiple of 8).  circomlib derives key and
rho with BLAKE-512, which Python's hashlib does not have: KEY AND NONCE DERIVATION HERE ARE NOT circomlib's - the default nonce is SHA-512 of
secret and message reduced mod l, a secret is whatever integer the caller brings.  Only the signatures (and what verifies) are circomlib's; one
published circomlibjs vector is checked by the tests, nothing beyond it.

Packed forms (pack_signature / unpack_signature, verify_packed*, sign_batch(packed=True)): a key is babyjub's 32-byte packed point, a
signature is 64 bytes - the packed R8, then S as 32 little-endian bytes - the layout of circomlibjs' packSignature as its documentation
describes it, written from memory: NO packed vector of circomlibjs has been checked (the one published vector is affine).  verify_packed* run
ONE launch on the wire bytes: a lane unpacks both points (a square root in Fr each) and then runs the hash and the chain of the unpacked
verifier.  A point with x == 0 and the sign bit set is rejected (status 3): this project's decision, which may differ from circomlibjs."""
import hashlib

import numpy as np

from . import babyjub as BJ
from . import poseidon
from .api import R_MOD, Fr, eddsa_poseidon_challenge_batch, eddsa_poseidon_verify_batch, eddsa_poseidon_verify_packed_batch


def _int(v):
    return v.v if isinstance(v, Fr) else int(v)


def public_keys(secrets, engine=None):
    """[[s]B8 for s in secrets] -> list of babyjub.Point: one bjj_mul_batch.  A secret is an integer (or Fr) in [0, r)"""
    return BJ.mul_base([Fr(_int(s)) for s in secrets], engine=engine)


def default_nonce(secret, msg):
    """SHA-512 of the secret and the message (32 little-endian bytes each) reduced mod l.  NOT circomlib's derivation (BLAKE-512 of the key's hash and the message)"""
    h = hashlib.sha512(_int(secret).to_bytes(32, "little") + _int(msg).to_bytes(32, "little")).digest()
    return int.from_bytes(h, "little") % BJ.L


def sign_batch(secrets, msgs, nonces=None, engine=None, packed=False):
    """[(R8, S)] for messages (Fr or integers mod r) under integer secrets: one bjj_mul_batch for the keys and the R8 together, one challenge
    call, S in host integers.  nonces: integers, None for default_nonce.  packed: 64-byte signatures instead (one bjj_pack_batch more)"""
    secrets = [_int(s) for s in secrets]; msgs = [_int(m) % R_MOD for m in msgs]
    if len(secrets) != len(msgs):
        raise ValueError(f"{len(secrets)} secrets, {len(msgs)} messages")
    nonces = [default_nonce(s, m) for s, m in zip(secrets, msgs)] if nonces is None else [int(x) for x in nonces]
    if len(nonces) != len(msgs):
        raise ValueError(f"{len(nonces)} nonces, {len(msgs)} messages")
    if not msgs:
        return []
    pts = BJ.mul_base([Fr(k) for k in secrets + [x % BJ.L for x in nonces]], engine=engine)
    A, R8 = pts[:len(msgs)], pts[len(msgs):]
    hm = eddsa_poseidon_challenge_batch(A, R8, [Fr(m) for m in msgs], engine=engine)
    ss = [(rho + 8 * h.v * s) % BJ.L for rho, h, s in zip(nonces, hm, secrets)]
    if packed:
        return [r + s.to_bytes(32, "little") for r, s in zip(BJ.pack_batch(R8, engine=engine), ss)]
    return list(zip(R8, ss))


def sign(secret, msg, nonce=None, engine=None, packed=False):
    return sign_batch([secret], [msg], None if nonce is None else [nonce], engine=engine, packed=packed)[0]


def pack_signature(sig):
    """(R8, S) -> 64 bytes: the packed R8 (babyjub.pack_host), then S as 32 little-endian bytes; S must fit 256 bits"""
    return BJ.pack_host(sig[0]) + _int(sig[1]).to_bytes(32, "little")


def unpack_signature(b):
    """64 bytes -> ((R8 as an (x, y) pair, S), status of the point) in host integers; nothing about S is checked"""
    b = bytes(b)
    if len(b) != 64:
        raise ValueError("a packed signature is 64 bytes")
    r8, st = BJ.unpack_host(b[:32])
    return (r8, int.from_bytes(b[32:], "little")), st


def _sig_arrays(pks, msgs, sigs):
    pks, msgs, sigs = list(pks), list(msgs), list(sigs)
    if not len(pks) == len(msgs) == len(sigs):
        raise ValueError(f"{len(pks)} keys, {len(msgs)} messages, {len(sigs)} signatures")
    for _, s in sigs:
        if not 0 <= _int(s) < 1 << 256:
            raise ValueError("S does not fit 256 bits")
    A = BJ._point_array(pks); R8 = BJ._point_array([r8 for r8, _ in sigs])
    # S travels as the Fr whose canonical integer it is; an S at or above r cannot, and travels as its own words (status 1: not below r)
    S = np.stack([Fr(_int(s)).limbs if _int(s) < R_MOD else BJ._limbs(_int(s)) for _, s in sigs]) if sigs else np.zeros((0, 4), np.uint64)
    M = np.stack([Fr(_int(m)).limbs for m in msgs]) if msgs else np.zeros((0, 4), np.uint64)
    return A, R8, S, M


def verify_status_batch(pks, msgs, sigs, engine=None):
    """(n,) int32 per (key, message, (R8, S)): the statuses of eddsa_poseidon_verify_batch (0 valid, 1 range, 4 curve, 6 equation)"""
    A, R8, S, M = _sig_arrays(pks, msgs, sigs)
    return eddsa_poseidon_verify_batch(A, R8, S, M, engine=engine)


def verify_batch(pks, msgs, sigs, engine=None):
    """list of bool: signature i is valid for message i under key i (one call, one lane per signature)"""
    return [int(s) == 0 for s in verify_status_batch(pks, msgs, sigs, engine=engine)]


def verify(pk, msg, sig, engine=None):
    return verify_batch([pk], [msg], [sig], engine=engine)[0]


def _msg_array(msgs):
    return np.stack([Fr(_int(m)).limbs for m in msgs]) if len(msgs) else np.zeros((0, 4), np.uint64)


def verify_packed_status_batch(pks32, msgs, sigs64, engine=None):
    """(n,) int32 per (packed key, message, packed signature): the statuses of eddsa_poseidon_verify_packed_batch (0 valid, 1 range, 4 a point
    has no x, 3 a non-canonical sign, 6 equation).  Keys and signatures: sequences of 32- and 64-byte strings, or uint8 arrays"""
    msgs = list(msgs)
    if not len(pks32) == len(msgs) == len(sigs64):
        raise ValueError(f"{len(pks32)} keys, {len(msgs)} messages, {len(sigs64)} signatures")
    return eddsa_poseidon_verify_packed_batch(pks32, sigs64, _msg_array(msgs), engine=engine)


def verify_packed_batch(pks32, msgs, sigs64, engine=None):
    """list of bool: packed signature i is valid for message i under packed key i (one call, one lane per signature)"""
    return [int(s) == 0 for s in verify_packed_status_batch(pks32, msgs, sigs64, engine=engine)]


def verify_packed(pk32, msg, sig64, engine=None):
    return verify_packed_batch([pk32], [msg], [sig64], engine=engine)[0]


def verify_packed_status_host(pk32, msg, sig64):
    """the status of one packed signature in host integers, in the order of the device's checks"""
    (r8, s), st_r = unpack_signature(sig64)
    a, st_a = BJ.unpack_host(pk32)
    m = _int(msg)
    if 1 in (st_a, st_r) or not (0 <= s < BJ.L and 0 <= m < R_MOD):
        return 1
    for st in (4, 3):
        if st in (st_a, st_r):
            return st
    return verify_status_host(a, m, (r8, s))


def challenge_host(a, r8, msg):
    """Poseidon5(r8.x, r8.y, a.x, a.y, msg) in host integers; a, r8: (x, y) pairs or babyjub.Point"""
    ax, ay = (a.x, a.y) if isinstance(a, BJ.Point) else a
    rx, ry = (r8.x, r8.y) if isinstance(r8, BJ.Point) else r8
    return poseidon.permute_host([0, rx, ry, ax, ay, _int(msg)])[0]


def verify_status_host(pk, msg, sig):
    """the status of one signature in host integers, in the order of the device's checks"""
    a = (pk.x, pk.y) if isinstance(pk, BJ.Point) else tuple(pk)
    r8 = (sig[0].x, sig[0].y) if isinstance(sig[0], BJ.Point) else tuple(sig[0])
    s, m = _int(sig[1]), _int(msg)
    if not (all(0 <= v < R_MOD for v in a + r8 + (m,)) and 0 <= s < BJ.L):
        return 1
    if not (BJ.on_curve_host(r8) and BJ.on_curve_host(a)):
        return 4
    hm = challenge_host(a, r8, m)
    return 0 if BJ.mul_host(BJ.B8, s) == BJ.add_host(r8, BJ.mul_host(a, 8 * hm)) else 6


def verify_host(pk, msg, sig):
    """circomlib's verifyPoseidon in host integers -> bool"""
    return verify_status_host(pk, msg, sig) == 0
