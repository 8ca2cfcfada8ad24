"""Host side of hash-to-curve for G1 and G2 (RFC 9380): expand_message_xmd over SHA-256 with hashlib, hash_to_field with L = 48 (m = 1 for G1,
m = 2 for G2) and the default tags.  The device computes the same expansion for messages of one length (Engine.g1_hash_to_curve_batch,
Engine.g2_hash_to_curve_batch); messages of mixed lengths are expanded here and take Engine.g{1,2}_hash_to_curve_uniform_batch - the bytes are
the same either way.  The maps' constants (Z = 1 and c1 .. c4 of the Shallue-van de Woestijne map over Fq and over Fq2,
tools/gen_device_constants.py) were derived from the RFC's formulas and are not checked against gnark-crypto or any other library; G2's
cofactor clearing is the one step the RFC defines no suite for, and neither its constants nor its outputs are checked against gnark-crypto or
any other library either."""
import hashlib

import numpy as np

from .api import Q_MOD
from .engine import H2C_FIELD_BYTES, H2C_UNIFORM_BYTES, H2C_G2_UNIFORM_BYTES, h2c_dst

L = H2C_FIELD_BYTES
SUITE = "BN254G1_XMD:SHA-256_SVDW_RO_"
DEFAULT_DST = b"BN_AMD-V01-CS01-with-" + SUITE.encode()                 # applications should pass a tag of their own
BLS_DST = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"
SUITE_G2 = "BN254G2_XMD:SHA-256_SVDW_RO_"
DEFAULT_G2_DST = b"BN_AMD-V01-CS01-with-" + SUITE_G2.encode()
BLS_G2_DST = b"BLS_SIG_BN254G2_XMD:SHA-256_SVDW_RO_NUL_"


def expand_message_xmd(msg, dst, length):
    """RFC 9380 section 5.3.1 over SHA-256: `length` uniform bytes from msg under the tag dst (1 .. 255 bytes; longer tags are not built)"""
    dst = h2c_dst(dst)
    ell = (length + 31) // 32
    if not 0 < length <= 65535 or ell > 255:
        raise ValueError(f"expand_message_xmd yields 1 .. {255 * 32} bytes, asked for {length}")
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(b"\0" * 64 + bytes(msg) + length.to_bytes(2, "big") + b"\0" + dst_prime).digest()
    blocks = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        blocks.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, blocks[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(blocks)[:length]


def hash_to_field(msg, dst=DEFAULT_DST, count=2, m=1):
    """`count` elements as integers mod q.  m = 1 (Fq): element i is bytes [48 i, 48 i + 48) of the uniform string, big endian.  m = 2 (Fq2):
    element i is the pair (c0, c1) from bytes [96 i, 96 i + 48) and [96 i + 48, 96 i + 96)."""
    if m not in (1, 2):
        raise ValueError(f"hash_to_field is built for m = 1 (Fq) and m = 2 (Fq2), got {m}")
    uniform = expand_message_xmd(msg, dst, L * m * count)
    v = [int.from_bytes(uniform[L * i:L * i + L], "big") % Q_MOD for i in range(m * count)]
    return v if m == 1 else [(v[2 * i], v[2 * i + 1]) for i in range(count)]


def uniform_bytes(msgs, dst=DEFAULT_DST, length=H2C_UNIFORM_BYTES):
    """(n, length) uint8: the uniform bytes of hash_to_curve for every message, expanded on the host (96 for G1, 192 for G2)"""
    rows = [np.frombuffer(expand_message_xmd(m, dst, length), np.uint8) for m in msgs]
    return np.stack(rows) if rows else np.zeros((0, length), np.uint8)


def uniform_bytes_g2(msgs, dst=DEFAULT_G2_DST):
    return uniform_bytes(msgs, dst, H2C_G2_UNIFORM_BYTES)


def message_array(msgs):
    """an (n, msg_len) uint8 array when the messages have one length (a 2-d uint8 array passes through), else None"""
    if isinstance(msgs, np.ndarray):
        if msgs.ndim != 2:
            raise ValueError(f"messages as an array are (n, msg_len) uint8, got shape {msgs.shape}")
        return np.ascontiguousarray(msgs, np.uint8)
    lens = {len(m) for m in msgs}
    if len(lens) > 1:
        return None
    ml = lens.pop() if lens else 0
    return np.frombuffer(b"".join(bytes(m) for m in msgs), np.uint8).reshape(len(msgs), ml)
