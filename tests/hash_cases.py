"""TEST INFRASTRUCTURE - the integer model of hash-to-curve for G1 (include/bn254_hip.h bn254_g1_map_to_curve_batch,
bn254_g1_hash_to_curve_uniform_batch, bn254_g1_hash_to_curve_batch) over bn_model and hashlib, written from RFC 9380's definitions, and the
case lists every test of the family shares.  Points are affine tuples of canonical integers, None is the point at infinity; `words` turns one
into the ABI's (x, y, 1) Montgomery image.  The constants are derived here from the formulas (Z by the RFC's find_z_svdw search); they are not
checked against gnark-crypto or any other library."""
import functools
import hashlib
import random

import numpy as np

import bn_model as M

Q = M.Q
L = 48                                     # bytes per field element of hash_to_field
UNIFORM = 2 * L
DST_MAX = 255
BLS_DST = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"


# ------------------------------------------------------------------------------------------------------------------ field helpers
def g(x):
    return (x * x * x + M.G1_B) % Q


def is_square(a):
    """zero counts as a square"""
    return a % Q == 0 or pow(a % Q, (Q - 1) // 2, Q) == 1


def sqrt(a):
    r = pow(a % Q, (Q + 1) // 4, Q)
    assert r * r % Q == a % Q
    return r


def sgn0(a):
    return (a % Q) & 1


def inv0(a):
    return pow(a % Q, Q - 2, Q)


# ------------------------------------------------------------------------------------------------------------------ the constants
def find_z_svdw():
    """RFC 9380 appendix H.1 for A = 0, B = 3"""
    ctr = 1
    while True:
        for z in (ctr % Q, -ctr % Q):
            if g(z) == 0:
                continue
            h = -(3 * z * z) * M.inv(4 * g(z)) % Q
            if h == 0 or not is_square(h):
                continue
            if is_square(g(z)) or is_square(g(-z * M.TWO_INV % Q)):
                return z
        ctr += 1


Z = find_z_svdw()
C1 = g(Z)
C2 = -Z * M.TWO_INV % Q
C3 = sqrt(-g(Z) * 3 * Z * Z % Q)
if sgn0(C3):
    C3 = Q - C3
C4 = -4 * g(Z) * M.inv(3 * Z * Z) % Q
assert (Z, C1, C2) == (1, 4, (Q - 1) // 2) and sgn0(C3) == 0
assert C3 == 0x16789af3a83522eb353c98fc6b36d713d5d8d1cc5dffffffa
assert C4 == 0x10216f7ba065e00de81ac1e7808072c9dd2b2385cd7b438469602eb24829a9bd


# ------------------------------------------------------------------------------------------------------------------ the algorithms
def map_branch(u):
    """-> ((x, y), branch 1 / 2 / 3, both) - `both`: g(x1) and g(x2) are squares, so the `and not e1` decides"""
    u %= Q
    tv1 = u * u * C1 % Q
    tv2 = (1 + tv1) % Q
    tv1 = (1 - tv1) % Q
    tv3 = inv0(tv1 * tv2)
    tv4 = u * tv1 * tv3 * C3 % Q
    x1 = (C2 - tv4) % Q
    x2 = (C2 + tv4) % Q
    x3 = (pow(tv2 * tv2 * tv3, 2, Q) * C4 + Z) % Q
    e1 = is_square(g(x1))
    sq2 = is_square(g(x2))
    e2 = sq2 and not e1
    x, branch = (x1, 1) if e1 else (x2, 2) if e2 else (x3, 3)
    y = sqrt(g(x))
    if sgn0(y) != sgn0(u):
        y = -y % Q
    assert y * y % Q == g(x)                                   # every mapped point is on the curve
    return (x, y), branch, e1 and sq2


def map_to_curve(u):
    return map_branch(u)[0]


def expand_message_xmd(msg, dst, length):
    assert 0 < len(dst) <= DST_MAX and length <= 255 * 32
    dst_prime = bytes(dst) + bytes([len(dst)])
    ell = (length + 31) // 32
    b0 = hashlib.sha256(b"\0" * 64 + bytes(msg) + length.to_bytes(2, "big") + b"\0" + dst_prime).digest()
    b = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:length]


_XMD_DST = b"QUUX-V01-CS02-with-expander-SHA256-128"
assert expand_message_xmd(b"", _XMD_DST, 32).hex() == "68a985b87eb6b46952128911f2a4412bbc302a9d759667f87f7a21d803f07235"
assert expand_message_xmd(b"abc", _XMD_DST, 32).hex() == "d8ccab23b5985ccea865c6c97b6e5b8350e794e603b4b97902f53a8a0d605615"


def hash_to_field(msg, dst, count=2):
    uniform = expand_message_xmd(msg, dst, L * count)
    return [int.from_bytes(uniform[L * i:L * i + L], "big") % Q for i in range(count)]


def add_affine(p, q):
    """the complete addition on affine tuples: equal points double, opposite points give None"""
    o = M.FQ_OPS
    s = M.g_add(o, (p[0], p[1], 1), (q[0], q[1], 1))
    return M.g_to_affine(o, s)


def hash_uniform(uniform):
    assert len(uniform) == UNIFORM
    u0, u1 = (int.from_bytes(uniform[L * i:L * i + L], "big") for i in range(2))
    return add_affine(map_to_curve(u0), map_to_curve(u1))


def hash_to_curve(msg, dst):
    return hash_uniform(expand_message_xmd(msg, dst, UNIFORM))


def words(pt):
    """the ABI image: (x, y, 1) in Montgomery form as 12 uint64, G::zero() = (0, 1, 0) for None"""
    cs = [0, 1, 0] if pt is None else [pt[0], pt[1], 1]
    return np.array([l for c in cs for l in M.to_mont_limbs(c)], np.uint64)


def affine_of(row):
    v = [M.from_mont_limbs(row[4 * i:4 * i + 4]) for i in range(3)]
    return M.g_to_affine(M.FQ_OPS, tuple(v))


# ------------------------------------------------------------------------------------------------------------------ the case lists
@functools.lru_cache(maxsize=None)
def u_cases():
    """[(name, 48-byte integer)]"""
    both = next(u for u in range(4, 400) if map_branch(u)[2])
    assert 60 <= sum(map_branch(u)[2] for u in range(1, 400)) <= 100           # about a fifth
    half = M.TWO_INV
    rows = [("0", 0), ("2", 2), ("3", 3), ("both=%d" % both, both), ("+1/2", half), ("-1/2", Q - half), ("q-1", Q - 1),
            ("q", Q), ("q+1", Q + 1), ("2^256-1", (1 << 256) - 1), ("2^256", 1 << 256), ("2^384-1", (1 << 384) - 1)]
    rng = random.Random(2200)
    rows += [("rand%d" % i, rng.getrandbits(384)) for i in range(6)]
    return rows


def _check_u_cases():
    by = {n: map_branch(u) for n, u in u_cases()}
    assert by["0"][1] == 1 and by["2"][1] == 2 and by["3"][1] == 3
    assert {b for _, b, _ in by.values()} == {1, 2, 3}
    assert {sgn0(p[1]) for p, _, _ in by.values()} == {0, 1}
    for n in ("+1/2", "-1/2"):                                                   # the exceptional inputs: tv3 = 0, x1 = x2 = c2
        assert (by[n][0][0], by[n][1]) == ((C2, 1) if is_square(g(C2)) else (Z, 3))
    assert by["+1/2"][0][1] == -by["-1/2"][0][1] % Q
    assert by["q"][0] == by["0"][0] and by["q+1"][0] == map_to_curve(1)


_check_u_cases()


def u_bytes(us):
    """(n, 48) uint8"""
    return np.stack([np.frombuffer(int(u).to_bytes(L, "big"), np.uint8) for u in us])


@functools.lru_cache(maxsize=None)
def map_batch(n, start=0):
    """n inputs cycling the case list from `start`: ((n, 48) uint8, (n, 12) uint64)"""
    cs = u_cases()
    us = [cs[(start + i) % len(cs)][1] for i in range(n)]
    return u_bytes(us), np.stack([words(map_to_curve(u)) for u in us])


@functools.lru_cache(maxsize=None)
def uniform_cases():
    """[(name, 96 bytes)]: u1 = u0 (the sum doubles), u1 = -u0 (the sum is G::zero()), random pairs"""
    rng = random.Random(2201)
    a = rng.getrandbits(380)
    rows = [("double", (a, a)), ("double-congruent", (a % Q, a % Q + Q)), ("cancel", (a % Q, Q - a % Q)), ("cancel-small", (5, Q - 5)), ("zero-zero", (0, 0))]
    rows += [("rand%d" % i, (rng.getrandbits(384), rng.getrandbits(384))) for i in range(6)]
    rows += [("case-%s" % n, (u, rng.getrandbits(384))) for n, u in u_cases()[:12]]
    return [(n, u0.to_bytes(L, "big") + u1.to_bytes(L, "big")) for n, (u0, u1) in rows]


def _check_uniform_cases():
    by = {n: hash_uniform(b) for n, b in uniform_cases()}
    assert by["cancel"] is None and by["cancel-small"] is None
    o = M.FQ_OPS
    u = int.from_bytes(dict(uniform_cases())["double"][:L], "big")
    p = map_to_curve(u)
    assert by["double"] == by["double-congruent"] == M.g_to_affine(o, M.g_double(o, (p[0], p[1], 1)))
    assert all(v is not None for n, v in by.items() if not n.startswith("cancel"))


_check_uniform_cases()


@functools.lru_cache(maxsize=None)
def uniform_batch(n, start=0):
    cs = uniform_cases()
    rows = [cs[(start + i) % len(cs)][1] for i in range(n)]
    return np.stack([np.frombuffer(b, np.uint8) for b in rows]), np.stack([words(hash_uniform(b)) for b in rows])


DST_LENS = (1, 21, 22, 43, 255)            # 21 / 22 put b_i's input (32 + 1 + dst_len + 1) at 55 / 56 bytes; 255 makes it multi-block


def dst_of(n):
    return (b"BN254G1_XMD:SHA-256_SVDW_RO_" + bytes(range(32, 127)) * 3)[:n]


def msg_lens(dst_len):
    """0, 1, 32 and the lengths that put b_0's input (64 + msg_len + 3 + dst_len + 1) at 55, 56, 63, 64 and 65 mod 64: its padding seams"""
    fixed = 64 + 3 + dst_len + 1
    return sorted({0, 1, 32} | {(r - fixed) % 64 for r in (55, 56, 63, 64, 65)})


def messages(n, msg_len, seed=0):
    """(n, msg_len) uint8"""
    rng = np.random.default_rng(2202 + 1000 * seed + msg_len)
    return rng.integers(0, 256, (n, msg_len), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def message_cases(per=2):
    """[(dst, (per, msg_len) uint8 messages, (per, 96) uint8 uniform bytes, (per, 12) uint64 points)] for every DST length and message length"""
    out = []
    for dl in DST_LENS:
        dst = dst_of(dl)
        for ml in msg_lens(dl):
            msgs = messages(per, ml, dl)
            uni = [expand_message_xmd(m.tobytes(), dst, UNIFORM) for m in msgs]
            out.append((dst, msgs, np.stack([np.frombuffer(b, np.uint8) for b in uni]), np.stack([words(hash_uniform(b)) for b in uni])))
    return out


assert all(len(dst_of(n)) == n for n in DST_LENS)
assert {(68 + ml + 21) % 64 for ml in msg_lens(21)} >= {55, 56, 63, 0, 1}
