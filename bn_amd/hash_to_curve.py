"""Host side of hash-to-curve for G1 (RFC 9380): expand_message_xmd over SHA-256 with hashlib, hash_to_field with L = 48 and the default tags.
The device computes the same expansion for messages of one length (Engine.g1_hash_to_curve_batch); messages of mixed lengths are expanded here
and take Engine.g1_hash_to_curve_uniform_batch - the bytes are the same either way.  The map's constants (Z = 1 and c1 .. c4 of the
Shallue-van de Woestijne map, tools/gen_device_constants.py) were derived from the RFC's formulas and are not checked against gnark-crypto or
any other library."""
import hashlib

import numpy as np

from .api import Q_MOD
from .engine import H2C_FIELD_BYTES, H2C_UNIFORM_BYTES, h2c_dst

L = H2C_FIELD_BYTES
SUITE = "BN254G1_XMD:SHA-256_SVDW_RO_"
DEFAULT_DST = b"BN_AMD-V01-CS01-with-" + SUITE.encode()                 # applications should pass a tag of their own
BLS_DST = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"


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


def hash_to_field(msg, dst=DEFAULT_DST, count=2):
    """`count` elements of Fq as integers: element i is bytes [48 i, 48 i + 48) of the uniform string, big endian, mod q"""
    uniform = expand_message_xmd(msg, dst, L * count)
    return [int.from_bytes(uniform[L * i:L * i + L], "big") % Q_MOD for i in range(count)]


def uniform_bytes(msgs, dst=DEFAULT_DST):
    """(n, 96) uint8: the uniform bytes of hash_to_curve for every message, expanded on the host"""
    rows = [np.frombuffer(expand_message_xmd(m, dst, H2C_UNIFORM_BYTES), np.uint8) for m in msgs]
    return np.stack(rows) if rows else np.zeros((0, H2C_UNIFORM_BYTES), np.uint8)


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
