"""TEST INFRASTRUCTURE - the integer model of hash-to-curve for G2 and of the cofactor clearing (include/bn254_hip.h
bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch, bn254_g2_hash_to_curve_uniform_batch, bn254_g2_hash_to_curve_batch) over bn_model
and hashlib, written from RFC 9380's definitions, and the case lists every test of the family shares.  Field elements are pairs (c0, c1) of
canonical integers, points are affine tuples (x, y) of such pairs, None is the point at infinity; `words` turns one into the ABI's (x, y, 1)
Montgomery image.  The constants are derived here from the formulas (Z by the RFC's find_z_svdw search) and the clearing is
clear(P) = [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P) (Fuentes-Castaneda et al., section 6.1): the one step the RFC defines no suite for.
Neither the constants nor the outputs are checked against gnark-crypto or any other library."""
import functools
import random

import numpy as np

import bn_model as M
from hash_cases import expand_message_xmd

Q, R, U = M.Q, M.R_ORD, M.U
L = 48                                     # bytes per Fq component of hash_to_field
FIELD = 2 * L                              # an Fq2 element: c0 then c1
UNIFORM = 2 * FIELD
DST_MAX = 255
BLS_G2_DST = b"BLS_SIG_BN254G2_XMD:SHA-256_SVDW_RO_NUL_"
O2 = M.FQ2_OPS
B2 = M.G2_B
ONE, ZERO = (1, 0), (0, 0)


# ------------------------------------------------------------------------------------------------------------------ field helpers
def f2(a):
    return (a[0] % Q, a[1] % Q)


def g(x):
    return M.f2_add(M.f2_mul(M.f2_sqr(x), x), B2)


def norm(a):
    return (a[0] * a[0] + a[1] * a[1]) % Q


def is_square(a):
    """the character of the norm; zero counts as a square"""
    n = norm(a)
    return n == 0 or pow(n, (Q - 1) // 2, Q) == 1


def _fq_sqrt(a):
    r = pow(a % Q, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def sqrt(a):
    """some root of a square (the caller fixes the sign)"""
    a = f2(a)
    if a[1] == 0:
        r = _fq_sqrt(a[0])
        root = (r, 0) if r is not None else (0, _fq_sqrt(-a[0]))
    else:
        n = _fq_sqrt(norm(a))
        assert n is not None
        w = _fq_sqrt((a[0] + n) * M.TWO_INV)
        if w is None:
            w = _fq_sqrt((a[0] - n) * M.TWO_INV)
        root = (w, a[1] * M.inv(2 * w) % Q)
    assert M.f2_sqr(root) == a
    return root


def sgn0(a):
    """RFC 9380 section 4.1 for m = 2: sign_0 | (zero_0 & sign_1)"""
    a = f2(a)
    return (a[0] & 1) | ((a[0] == 0) & (a[1] & 1))


def inv0(a):
    return ZERO if f2(a) == ZERO else M.f2_inv(f2(a))


# ------------------------------------------------------------------------------------------------------------------ the constants
def find_z_svdw():
    """RFC 9380 appendix H.1 for A = 0, B = b' over Fq2: the candidates are F(ctr) and F(-ctr)"""
    ctr = 1
    while True:
        for z in ((ctr % Q, 0), (-ctr % Q, 0)):
            if g(z) == ZERO:
                continue
            h = M.f2_neg(M.f2_mul(M.f2_scale(M.f2_sqr(z), 3), M.f2_inv(M.f2_scale(g(z), 4))))
            if h == ZERO or not is_square(h):
                continue
            if is_square(g(z)) or is_square(g(M.f2_scale(z, -M.TWO_INV % Q))):
                return z
        ctr += 1


Z = find_z_svdw()
C1 = g(Z)
C2 = M.f2_scale(Z, -M.TWO_INV % Q)
C3 = sqrt(M.f2_neg(M.f2_mul(g(Z), M.f2_scale(M.f2_sqr(Z), 3))))
if sgn0(C3):
    C3 = M.f2_neg(C3)
C4 = M.f2_mul(M.f2_scale(g(Z), -4 % Q), M.f2_inv(M.f2_scale(M.f2_sqr(Z), 3)))
assert Z == ONE and C1 == M.f2_add(ONE, B2) and C2 == ((Q - 1) // 2, 0) and sgn0(C3) == 0
assert C3 == (18992192239972082890849143911285057164064277369389217330423471574879236301292,
              21819008332247140148575583693947636719449476128975323941588917397607662637108)
assert C4 == (10499238450719652342378357227399831140106360636427411350395554762472100376473,
              6940174569119770192419592065569379906172001098655407502803841283667998553941)


# ------------------------------------------------------------------------------------------------------------------ the algorithms
def map_branch(u):
    """u = (c0, c1), any integers -> ((x, y), branch 1 / 2 / 3, both) - `both`: g(x1) and g(x2) are squares, so the `and not e1` decides"""
    u = f2(u)
    tv1 = M.f2_mul(M.f2_sqr(u), C1)
    tv2 = M.f2_add(ONE, tv1)
    tv1 = M.f2_sub(ONE, tv1)
    tv3 = inv0(M.f2_mul(tv1, tv2))
    tv4 = M.f2_mul(M.f2_mul(u, tv1), M.f2_mul(tv3, C3))
    x1 = M.f2_sub(C2, tv4)
    x2 = M.f2_add(C2, tv4)
    x3 = M.f2_add(M.f2_mul(M.f2_sqr(M.f2_mul(M.f2_sqr(tv2), tv3)), C4), Z)
    e1 = is_square(g(x1))
    sq2 = is_square(g(x2))
    e2 = sq2 and not e1
    x, branch = (x1, 1) if e1 else (x2, 2) if e2 else (x3, 3)
    y = sqrt(g(x))
    if sgn0(y) != sgn0(u):
        y = M.f2_neg(y)
    assert M.f2_sqr(y) == g(x)                                 # every mapped point is on the twist
    return (x, y), branch, e1 and sq2


def map_to_curve(u):
    return map_branch(u)[0]


def jac(p):
    return M.g_zero(O2) if p is None else (p[0], p[1], ONE)


def aff(p):
    return M.g_to_affine(O2, p)


def psi(p):
    """on Jacobian coordinates: (conj(X) gx, conj(Y) gy, conj(Z))"""
    return (M.f2_mul(M.f2_conj(p[0]), M.TWIST_MUL_BY_Q_X), M.f2_mul(M.f2_conj(p[1]), M.TWIST_MUL_BY_Q_Y), M.f2_conj(p[2]))


def mul_plain(p, k):
    """double-and-add, MSB first, with the complete addition: valid off the subgroup"""
    acc = M.g_zero(O2)
    for bit in bin(k)[2:] if k else "":
        acc = M.g_double(O2, acc)
        if bit == "1":
            acc = M.g_add(O2, acc, p)
    return acc


def clear_jac(p):
    up = mul_plain(p, U)
    u3p = M.g_add(O2, M.g_double(O2, up), up)
    acc = M.g_add(O2, up, psi(u3p))
    acc = M.g_add(O2, acc, psi(psi(up)))
    return M.g_add(O2, acc, psi(psi(psi(p))))


def clear(p):
    """affine or None -> affine or None"""
    return aff(clear_jac(jac(p)))


LAMBDA = 6 * U * U % R
CLEAR_K = (U + 3 * U * LAMBDA + U * LAMBDA * LAMBDA + LAMBDA ** 3) % R          # clear(Q) = [k]Q on G2
assert CLEAR_K != 0
COFACTOR = 2 * Q - R


def add_affine(p, q):
    return aff(M.g_add(O2, jac(p), jac(q)))


def in_g2(p):
    return p is None or M.g_is_zero(O2, mul_plain(jac(p), R))


def split_uniform(uniform):
    assert len(uniform) == UNIFORM
    v = [int.from_bytes(uniform[L * i:L * i + L], "big") for i in range(4)]
    return (v[0], v[1]), (v[2], v[3])


def hash_uniform(uniform):
    u0, u1 = split_uniform(uniform)
    return clear(add_affine(map_to_curve(u0), map_to_curve(u1)))


def hash_to_field(msg, dst, count=2):
    uniform = expand_message_xmd(msg, dst, FIELD * count)
    return [tuple(int.from_bytes(uniform[FIELD * i + L * j:FIELD * i + L * j + L], "big") % Q for j in range(2)) for i in range(count)]


def hash_to_curve(msg, dst):
    return hash_uniform(expand_message_xmd(msg, dst, UNIFORM))


def words(pt):
    """the ABI image: (x, y, 1) in Montgomery form as 24 uint64, G2::zero() = (0, 1, 0) for None"""
    cs = [ZERO, ONE, ZERO] if pt is None else [pt[0], pt[1], ONE]
    return np.array([l for c in cs for h in c for l in M.to_mont_limbs(h)], np.uint64)


def jac_words(p):
    """any Jacobian triple as it stands"""
    return np.array([l for c in p for h in c for l in M.to_mont_limbs(h)], np.uint64)


def affine_of(row):
    v = [M.from_mont_limbs(row[4 * i:4 * i + 4]) for i in range(6)]
    return aff(((v[0], v[1]), (v[2], v[3]), (v[4], v[5])))


# ------------------------------------------------------------------------------------------------------------------ the case lists
def _exceptional():
    """u with u^2 c1 = +1 / -1 (tv1 tv2 = 0, so tv3 = inv0(0) = 0 and x1 = x2 = c2), where the root exists in Fq2"""
    out = []
    for name, s in (("u^2c1=+1", ONE), ("u^2c1=-1", M.f2_neg(ONE))):
        t = M.f2_mul(s, M.f2_inv(C1))
        if is_square(t):
            out.append((name, sqrt(t)))
    return out


@functools.lru_cache(maxsize=None)
def u_cases():
    """[(name, (c0, c1))], the halves any integers below 2^384"""
    edge = [("q-1", Q - 1), ("q", Q), ("q+1", Q + 1), ("2^256-1", (1 << 256) - 1), ("2^256", 1 << 256), ("2^384-1", (1 << 384) - 1)]
    rows = [("0", (0, 0)), ("1", (1, 0)), ("i", (0, 1)), ("2", (2, 0)), ("3", (3, 0)), ("c0=0,c1-odd", (0, 7)), ("c0=q,c1-odd", (Q, Q + 5))]
    rows += [("%s|%s" % (edge[j][0], edge[(j + 1) % 6][0]), (edge[j][1], edge[(j + 1) % 6][1])) for j in range(6)]
    rng = random.Random(2300)
    rows += [("rand%d" % j, (rng.getrandbits(384), rng.getrandbits(384))) for j in range(6)]
    rows += _exceptional()
    return rows


def _check_u_cases():
    by = {n: map_branch(u) for n, u in u_cases()}
    assert (by["0"][1], by["1"][1], by["3"][1]) == (3, 1, 3)
    assert by["i"][2] and by["2"][2]                                            # both g(x1) and g(x2) are squares: x1 wins
    assert {b for _, b, _ in by.values()} == {1, 2, 3}
    assert {sgn0(p[1]) for p, _, _ in by.values()} == {0, 1}
    assert sgn0(by["c0=0,c1-odd"][0][1]) == 1 and sgn0(by["c0=q,c1-odd"][0][1]) == 1      # decided by c1
    exc = _exceptional()
    assert exc                                                                   # at least one of the two roots exists
    for n, _ in exc:                                                             # tv3 = 0: x1 = x2 = c2, else x3 = Z
        assert (by[n][0][0], by[n][1]) == ((C2, 1) if is_square(g(C2)) else (Z, 3))
    assert by["q|q+1"][0] == map_to_curve((0, 1)) and by["q-1|q"][0] == map_to_curve((Q - 1, 0))
    pts = [p for p, _, _ in by.values()]
    assert not any(in_g2(p) for p in pts[:8])                                    # a mapped point is not in G2
    cl = [clear(p) for p in pts]
    assert all(c is not None and in_g2(c) for c in cl)
    assert any(cl[j] != aff(mul_plain(jac(pts[j]), COFACTOR)) for j in range(4))           # clear is not [2q - r]
    for kk in (1, 2, 3, 0xdeadbeef):                                             # on G2 the clearing is the scalar k
        qq = mul_plain(M.G2_ONE, kk)
        assert aff(clear_jac(qq)) == aff(mul_plain(qq, CLEAR_K)) == aff(M.g_mul(O2, qq, CLEAR_K))
    assert clear(None) is None


_check_u_cases()


def u_bytes(us):
    """(n, 96) uint8"""
    return np.stack([np.frombuffer(int(u[0]).to_bytes(L, "big") + int(u[1]).to_bytes(L, "big"), np.uint8) for u in us])


@functools.lru_cache(maxsize=None)
def _mapped(u):
    return map_to_curve(u)


@functools.lru_cache(maxsize=None)
def map_batch(n, start=0):
    """n inputs cycling the case list from `start`: ((n, 96) uint8, (n, 24) uint64)"""
    cs = u_cases()
    us = [cs[(start + i) % len(cs)][1] for i in range(n)]
    return u_bytes(us), np.stack([words(_mapped(u)) for u in us])


@functools.lru_cache(maxsize=None)
def uniform_cases():
    """[(name, 192 bytes)]: u1 = u0 (the sum doubles), u1 = u0 mod q, u1 = -u0 (the sum is infinity: G2::zero()), (0, 0), random pairs and
    every map case against a random partner"""
    rng = random.Random(2301)
    a = (rng.getrandbits(380), rng.getrandbits(380))
    am = f2(a)
    rows = [("double", (a, a)), ("double-congruent", (am, (am[0] + Q, am[1] + 2 * Q))), ("cancel", (am, M.f2_neg(am))),
            ("cancel-small", ((5, 0), (Q - 5, 0))), ("zero-zero", ((0, 0), (0, 0)))]
    rows += [("rand%d" % i, ((rng.getrandbits(384), rng.getrandbits(384)), (rng.getrandbits(384), rng.getrandbits(384)))) for i in range(4)]
    rows += [("case-%s" % n, (u, (rng.getrandbits(384), rng.getrandbits(384)))) for n, u in u_cases()]
    return [(n, b"".join(int(c).to_bytes(L, "big") for c in (u0[0], u0[1], u1[0], u1[1]))) for n, (u0, u1) in rows]


@functools.lru_cache(maxsize=None)
def _hashed(b):
    return hash_uniform(b)


def _check_uniform_cases():
    by = {n: _hashed(b) for n, b in uniform_cases()}
    assert by["cancel"] is None and by["cancel-small"] is None
    u0, _ = split_uniform(dict(uniform_cases())["double"])
    p = map_to_curve(u0)
    assert by["double"] == by["double-congruent"] == clear(aff(M.g_double(O2, jac(p))))
    assert all(v is not None for n, v in by.items() if not n.startswith("cancel"))


_check_uniform_cases()


@functools.lru_cache(maxsize=None)
def uniform_batch(n, start=0):
    cs = uniform_cases()
    rows = [cs[(start + i) % len(cs)][1] for i in range(n)]
    return np.stack([np.frombuffer(b, np.uint8) for b in rows]), np.stack([words(_hashed(b)) for b in rows])


@functools.lru_cache(maxsize=None)
def clear_cases():
    """[(name, Jacobian triple, affine result or None)]: mapped points (off the subgroup), G2 points with z != 1, infinity in three spellings"""
    rows = [("mapped-%s" % n, jac(_mapped(u))) for n, u in u_cases()[:8]]
    rows += [("g2-%d" % kk, M.g_mul(O2, M.G2_ONE, kk)) for kk in (1, 2, 3, R - 1, 0x1234567890abcdef)]
    p = _mapped(u_cases()[-1][1])
    rows += [("mapped-z", M.g_double(O2, M.g_double(O2, jac(p)))), ("zero", M.g_zero(O2)), ("z=0-xy", (p[0], p[1], ZERO)), ("all-zero", (ZERO, ZERO, ZERO))]
    return [(n, pt, aff(clear_jac(pt))) for n, pt in rows]


assert all((c is None) == (pt[2] == ZERO) for _, pt, c in clear_cases())


@functools.lru_cache(maxsize=None)
def clear_batch(n, start=0):
    """((n, 24) uint64 points, (n, 24) uint64 cleared and normalised)"""
    cs = clear_cases()
    rows = [cs[(start + i) % len(cs)] for i in range(n)]
    return np.stack([jac_words(pt) for _, pt, _ in rows]), np.stack([words(c) for _, _, c in rows])


DST_LENS = (1, 21, 22, 43, 255)            # 21 / 22 put b_i's input (32 + 1 + dst_len + 1) at 55 / 56 bytes; 255 makes it multi-block


def dst_of(n):
    return (b"BN254G2_XMD:SHA-256_SVDW_RO_" + bytes(range(32, 127)) * 3)[:n]


def msg_lens(dst_len):
    """0, 1, 32 and the lengths that put b_0's input (64 + msg_len + 3 + dst_len + 1) at 55, 56, 63, 64 and 65 mod 64: its padding seams"""
    fixed = 64 + 3 + dst_len + 1
    return sorted({0, 1, 32} | {(r - fixed) % 64 for r in (55, 56, 63, 64, 65)})


def messages(n, msg_len, seed=0):
    """(n, msg_len) uint8"""
    rng = np.random.default_rng(2302 + 1000 * seed + msg_len)
    return rng.integers(0, 256, (n, msg_len), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def message_cases(per=1):
    """[(dst, (per, msg_len) uint8 messages, (per, 192) uint8 uniform bytes, (per, 24) uint64 points)] for every DST length and message length"""
    out = []
    for dl in DST_LENS:
        dst = dst_of(dl)
        for ml in msg_lens(dl):
            msgs = messages(per, ml, dl)
            uni = [expand_message_xmd(m.tobytes(), dst, UNIFORM) for m in msgs]
            out.append((dst, msgs, np.stack([np.frombuffer(b, np.uint8) for b in uni]), np.stack([words(_hashed(b)) for b in uni])))
    return out


assert all(len(dst_of(n)) == n for n in DST_LENS)
assert {(68 + ml + 21) % 64 for ml in msg_lens(21)} >= {55, 56, 63, 0, 1}
assert len(expand_message_xmd(b"", dst_of(21), UNIFORM)) == UNIFORM == 192
