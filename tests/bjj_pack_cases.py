"""TEST INFRASTRUCTURE - the integer model and the inputs of the tests of the square root in Fr, of Baby Jubjub point packing and of the packed
EdDSA-Poseidon verifier (tests/test_bjj_pack_model.py, tests/test_hostsim_bjj_pack.py and tests/test_bjj_pack_abi.py on the CPU,
tests/test_gpu_fr_sqrt.py, tests/test_gpu_bjj_pack.py and tests/test_gpu_eddsa_packed.py on the GPU).

The model is written independently of the package: the data-dependent Tonelli-Shanks of tests/babyjub_cases.py for the root, Python integers
and bytes for the records.  A packed point is 32 bytes: the canonical integer of y little endian, bit 7 of byte 31 set iff the canonical
integer of x is above (r - 1) / 2.  A packed signature is the packed R8 followed by S as 32 little-endian bytes."""
import functools

import numpy as np

import babyjub_cases as BC
import fr_cases as FC

R = BC.R
HALF = (R - 1) // 2
S2, T_ODD = 28, (R - 1) >> 28
C28 = pow(5, T_ODD, R)                       # a generator of the subgroup of order 2^28
ST_OK, ST_RANGE, ST_SIGN, ST_NO_POINT, ST_EQUATION = 0, 1, 3, 4, 6


# ---- the model
def sqrt(v):
    """the root of v that is not above (r - 1) / 2, None for a non-residue"""
    x = BC.sqrt(v)
    return None if x is None else min(x, R - x)


def pack(p):
    x, y = p
    return (y | (1 << 255 if x > HALF else 0)).to_bytes(32, "little")


def unpack(b):
    """32 bytes -> (point, status); a rejected record is O"""
    v = int.from_bytes(b, "little")
    sign, y = v >> 255, v & ((1 << 255) - 1)
    if y >= R:
        return BC.O, ST_RANGE
    x = sqrt((1 - y * y) * BC.inv(BC.A_COEFF - BC.D_COEFF * y * y))
    if x is None:
        return BC.O, ST_NO_POINT
    if x == 0 and sign:
        return BC.O, ST_SIGN
    return ((R - x if sign else x), y), ST_OK


def pack_signature(r8, s):
    return pack(r8) + s.to_bytes(32, "little")


def verify_packed_status(a32, sig64, m):
    """a32, sig64 bytes; m a 256-bit integer as the words of msg hold it"""
    (a, sa), (r8, sr) = unpack(a32), unpack(sig64[:32])
    s = int.from_bytes(sig64[32:], "little")
    if ST_RANGE in (sa, sr) or s >= BC.L or m >= R:
        return ST_RANGE
    if ST_NO_POINT in (sa, sr):
        return ST_NO_POINT
    if ST_SIGN in (sa, sr):
        return ST_SIGN
    return BC.verify_status(a, r8, s, m)


def byte_rows(records):
    """[bytes of equal length] -> (n, len) uint8"""
    return np.frombuffer(b"".join(records), np.uint8).reshape(len(records), -1).copy() if records else np.zeros((0, 32), np.uint8)


def model_sqrt(vals):
    """(rows, ok): Option<Fr> with None as Fr::zero() and ok = 0"""
    roots = [sqrt(v) for v in vals]
    return FC.rows([0 if x is None else x for x in roots]), np.array([0 if x is None else 1 for x in roots], np.int32)


# ---- square-root inputs
@functools.lru_cache(maxsize=None)
def sqrt_values():
    rng = np.random.default_rng(2601)
    vals = [0, 1, 4, R - 1, 5, HALF * HALF % R]
    vals += [pow(C28, 1 << k, R) for k in range(S2)]                   # one element of every exact 2-power order
    vals += [pow(C28, k, R) for k in range(16)] + [pow(C28, 16 * k, R) for k in range(16)]
    vals += [pow(v, T_ODD, R) for v in (2, 3, 7, 11)]                  # t-th powers: elements of the 2-power subgroup
    vals += [pow(v, 1 << S2, R) for v in (2, 3)]                       # and elements of odd order
    rand = [FC.rand(rng) for _ in range(64)]
    kinds = [sqrt(v) is None for v in rand]
    assert any(kinds) and not all(kinds)
    return tuple(vals + rand)


# ---- unpack inputs
@functools.lru_cache(maxsize=None)
def unpack_records():
    """[(bytes, point, status)]"""
    sm = BC.small_order_points()
    y0 = (BC.inv(BC.sqrt(BC.A_COEFF)), 0)
    o8 = sm["order8"]
    eight = [BC.mul(o8, k) for k in range(8)]
    assert len(set(eight)) == 8
    pts = [BC.O, (0, R - 1), y0, BC.neg(y0)] + eight + [BC.G, BC.B8, BC.KAT_A, BC.KAT_R8, BC.neg(BC.G), BC.neg(BC.B8)]
    recs = [pack(p) for p in pts]
    flag = 1 << 255
    recs += [(1 | flag).to_bytes(32, "little"), ((R - 1) | flag).to_bytes(32, "little")]        # x = 0 with the sign bit set
    recs += [v.to_bytes(32, "little") for v in (R, R + 1, (1 << 255) - 1, R | flag)] + [b"\xff" * 32]
    rng = np.random.default_rng(2602)
    recs += [(FC.rand(rng) | (flag if i % 2 else 0)).to_bytes(32, "little") for i in range(48)]
    out = [(b,) + unpack(b) for b in recs]
    for p, (b, q, st) in zip(pts, out):
        assert st == ST_OK and q == p
    st = [o[2] for o in out]
    assert st.count(ST_SIGN) == 2 and st.count(ST_RANGE) == 5 and ST_NO_POINT in st[-48:] and ST_OK in st[-48:]
    return tuple(out)


# ---- signatures
@functools.lru_cache(maxsize=None)
def packed_signature_rows():
    """[(name, a32, sig64, m, status)]: the known answer, valid signatures, the failing rows of babyjub_cases translated where they can be packed,
    and one row for each precedence of the statuses"""
    rows = [("kat", pack(BC.KAT_A), pack_signature(BC.KAT_R8, BC.KAT_S), BC.KAT_M)]
    rows += [("valid%d" % i, pack(a), pack_signature(r8, s), m) for i, (a, r8, s, m) in enumerate(BC.signatures(6, 5))]
    for name, (a, r8, s, m), _ in BC.failing_rows():
        if BC.on_curve(a) and BC.on_curve(r8):                                     # a point off the curve has no packing
            rows.append((name, pack(a), pack_signature(r8, s), m))
    _, (a, r8, s, m), _ = BC.failing_rows()[0]
    flag = 1 << 255
    no_point = next(b for b, _, st in unpack_records()[-48:] if st == ST_NO_POINT)
    bad_sign = (1 | flag).to_bytes(32, "little")
    y_at_r = R.to_bytes(32, "little")
    rows += [("A: y at r", y_at_r, pack_signature(r8, s), m), ("R8: y at r", pack(a), y_at_r + s.to_bytes(32, "little"), m),
             ("S with the top bit", pack(a), pack(r8) + (s | flag).to_bytes(32, "little"), m), ("msg at 2^256 - 1", pack(a), pack_signature(r8, s), (1 << 256) - 1),
             ("A: no point", no_point, pack_signature(r8, s), m), ("R8: no point", pack(a), no_point + s.to_bytes(32, "little"), m),
             ("A: sign", bad_sign, pack_signature(r8, s), m), ("R8: sign", pack(a), bad_sign + s.to_bytes(32, "little"), m),
             ("range over no point", no_point, pack_signature(r8, BC.L), m), ("range over sign", bad_sign, pack_signature(r8, s), R),
             ("no point over sign", bad_sign, no_point + s.to_bytes(32, "little"), m), ("sign over equation", bad_sign, pack_signature(r8, s), m + 1),
             ("equation: -R8", pack(a), pack_signature(BC.neg(r8), s), m), ("A = O packed", pack(BC.O), pack_signature(BC.mul(BC.B8, s), s), m)]
    out = tuple(r + (verify_packed_status(r[1], r[2], r[3]),) for r in rows)
    want = {"kat": 0, "valid": 0, "wrong message": 6, "-A": 6, "S + l": 1, "S = l": 1, "msg at r": 1, "A = O": 0, "A of order 2": 0, "A of order 8": 0,
            "A: y at r": 1, "R8: y at r": 1, "S with the top bit": 1, "msg at 2^256 - 1": 1, "A: no point": 4, "R8: no point": 4, "A: sign": 3, "R8: sign": 3,
            "range over no point": 1, "range over sign": 1, "no point over sign": 4, "sign over equation": 3, "equation: -R8": 6, "A = O packed": 0}
    got = {r[0]: r[4] for r in out}
    assert all(got[n] == st for n, st in want.items()) and all(got["valid%d" % i] == 0 for i in range(6))
    return out


def signature_arrays(rows):
    """rows of packed_signature_rows() -> (a32 (n,32) uint8, sig64 (n,64) uint8, msg (n,4) uint64)"""
    return byte_rows([r[1] for r in rows]), byte_rows([r[2] for r in rows]), BC.raw_rows([r[3] for r in rows])
