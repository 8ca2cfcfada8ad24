"""TEST INFRASTRUCTURE - the integer model of point validation (include/bn254_hip.h bn254_g1_validate_batch, bn254_g2_validate_batch) over bn_model
and hash_g2_cases, and the case lists every test of the family shares.  A case is (name, the ABI record as uint64 words - 12 for G1, 24 for G2 -,
the expected status).  The model reads a record the way the header says: 1 when the words of a coordinate, as they stand, are not below q;
0 for z == 0; 4 unless Y^2 == X^3 + b Z^6; 5 (G2) unless the point is in the subgroup - and membership is decided by [r]P == 0 through
hash_g2_cases.mul_plain alone, never by the endomorphism identity the device runs.  The three integer facts the identity's soundness and
completeness rest on are asserted at import."""
import functools
import math

import numpy as np

import bn_model as M
import hash_g2_cases as HC

Q, R, U = M.Q, M.R_ORD, M.U
O1, O2 = M.FQ_OPS, M.FQ2_OPS
OK, E_RANGE, E_CURVE, E_SUBGROUP = 0, 1, 4, 5
COFACTOR = HC.COFACTOR
SMALL_ORDERS = (10069, 5864401)            # the two small prime factors of the cofactor 2q - r

# ------------------------------------------------------------------------------------------------------------------ the identity, on integers
# P in G2  <=>  [u + 1]P + psi([u]P) + psi^2([u]P) == psi^3([2u]P), i.e. g(psi) P = 0 with g(X) = (u + 1) + uX + uX^2 - 2uX^3.
# psi satisfies X^2 - tX + q = 0 on E'(Fq2), t = 6u^2 + 1:  X^2 = tX - q,  X^3 = (t^2 - q) X - tq,  so g = A + B X with
T = 6 * U * U + 1
A = (U + 1) - U * Q + 2 * U * T * Q
B = U + U * T - 2 * U * (T * T - Q)
N = A * A + A * B * T + B * B * Q          # the norm of A + B psi: an integer that kills every point g(psi) kills
LAMBDA = HC.LAMBDA                         # psi on G2
assert COFACTOR % SMALL_ORDERS[0] == 0 and COFACTOR % SMALL_ORDERS[1] == 0
assert N % R == 0                                                                    # soundness: the order of such a point divides gcd(N, r (2q - r)) ...
assert math.gcd(N, COFACTOR) == 1                                                    # ... = r
assert ((U + 1) + U * LAMBDA + U * LAMBDA ** 2 - 2 * U * LAMBDA ** 3) % R == 0       # completeness: g(lambda) = 0 mod r
assert (LAMBDA * LAMBDA - T * LAMBDA + Q) % R == 0                                   # lambda is a root of psi's polynomial mod r


def endo_accepts(p):
    """the identity itself in the integer model (a Jacobian triple over Fq2): only for the self-check below, never for an expected status"""
    up = HC.mul_plain(p, U)
    lhs = M.g_add(O2, M.g_add(O2, M.g_add(O2, up, p), HC.psi(up)), HC.psi(HC.psi(up)))
    rhs = HC.psi(HC.psi(HC.psi(M.g_double(O2, up))))
    return M.g_is_zero(O2, M.g_add(O2, lhs, M.g_neg(O2, rhs)))


# ------------------------------------------------------------------------------------------------------------------ the model
def _ints(row, coords):
    """the 256-bit integers of the record's words as they stand"""
    row = [int(v) for v in row]
    return [sum(row[4 * i + j] << (64 * j) for j in range(4)) for i in range(coords)]


def _unmont(v):
    return v * M.inv(M.MONT_R) % Q


def g1_status(row):
    v = _ints(row, 3)
    if any(c >= Q for c in v):
        return E_RANGE
    x, y, z = (_unmont(c) for c in v)
    if z == 0:
        return OK
    return OK if (y * y - x * x * x - M.G1_B * pow(z, 6, Q)) % Q == 0 else E_CURVE


def g2_point(row):
    v = [_unmont(c) for c in _ints(row, 6)]
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def g2_on_curve(p):
    x, y, z = p
    z2 = M.f2_sqr(z)
    return M.f2_sqr(y) == M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.f2_mul(M.G2_B, M.f2_mul(M.f2_sqr(z2), z2)))


def g2_status(row):
    if any(c >= Q for c in _ints(row, 6)):
        return E_RANGE
    p = g2_point(row)
    if p[2] == HC.ZERO:
        return OK
    if not g2_on_curve(p):
        return E_CURVE
    return OK if M.g_is_zero(O2, HC.mul_plain(p, R)) else E_SUBGROUP


# ------------------------------------------------------------------------------------------------------------------ records
def g1_words(p):
    return np.array([l for c in p for l in M.to_mont_limbs(c % Q)], np.uint64)


g2_words = HC.jac_words


def _raw(v):
    """a 256-bit integer as four words, as it stands (no Montgomery change)"""
    return [(v >> (64 * j)) & 0xffffffffffffffff for j in range(4)]


def _with(row, coord, words):
    out = row.copy()
    out[4 * coord:4 * coord + 4] = np.array(words, np.uint64)
    return out


def _flip(row, coord):
    """one limb of a coordinate with its lowest bit flipped"""
    out = row.copy()
    out[4 * coord] ^= np.uint64(1)
    return out


def _unreduced(row, coord):
    """the coordinate's words plus q: the same residue, not below q (q < 2^254: the sum fits 256 bits)"""
    v = _ints(row, len(row) // 4)[coord] + Q
    assert Q <= v < 1 << 256
    return _with(row, coord, _raw(v))


def _scaled(o, p, lam):
    """the same point with z multiplied by lam"""
    l2 = o.mul(lam, lam)
    return (o.mul(p[0], l2), o.mul(p[1], o.mul(l2, lam)), o.mul(p[2], lam))


@functools.lru_cache(maxsize=None)
def _small_order_points():
    """[(l, a Jacobian point of order exactly l)] for the two small prime factors of the cofactor: [n / l] * mapped, n = r (2q - r)"""
    out = []
    n = R * COFACTOR
    for l in SMALL_ORDERS:
        for _, u in HC.u_cases():
            p = HC.mul_plain(HC.jac(HC._mapped(u)), n // l)
            if not M.g_is_zero(O2, p):
                break
        assert not M.g_is_zero(O2, p) and M.g_is_zero(O2, HC.mul_plain(p, l))
        out.append((l, p))
    return out


@functools.lru_cache(maxsize=None)
def g2_cases():
    """[(name, (24,) uint64 record, status)]"""
    lam = (0x1234567, 0x89abcde)
    cleared = [(n, pt, c) for n, pt, c in HC.clear_cases() if c is not None]
    members = [("cleared-%s" % n, HC.jac(c)) for n, _, c in cleared[:3]]
    members += [("cleared-z-%s" % n, HC.clear_jac(pt)) for n, pt, _ in cleared[3:5]]                   # as the chain leaves them: z != 1
    members += [("neg-" + n, M.g_neg(O2, p)) for n, p in members[:2] + members[3:4]]
    members += [("generator", M.G2_ONE), ("[r-1]G", M.g_mul(O2, M.G2_ONE, R - 1)), ("[r-1]G-affine", HC.jac(HC.aff(M.g_mul(O2, M.G2_ONE, R - 1))))]
    members += [(n, pt) for n, pt, c in HC.clear_cases() if c is None]                                 # infinity in three spellings
    assert sum(1 for _, p in members if p[2] == HC.ZERO) == 3 and any(p[2] not in (HC.ONE, HC.ZERO) for _, p in members)
    mapped = [(n, HC.jac(HC._mapped(u))) for n, u in HC.u_cases()[:4]]
    outside = [("mapped-%s" % n, p) for n, p in mapped]
    outside += [("[r]mapped-%s" % n, HC.mul_plain(p, R)) for n, p in mapped[:2]]
    small = _small_order_points()
    outside += [("order-%d" % l, p) for l, p in small]
    outside += [("order-%d-affine" % l, HC.jac(HC.aff(p))) for l, p in small]
    g2pt = M.g_mul(O2, M.G2_ONE, 0xfeedface)
    outside += [("g2+order-%d" % l, M.g_add(O2, g2pt, p)) for l, p in small]
    outside += [("mapped-z", _scaled(O2, mapped[1][1], lam))]
    rows = [(n, g2_words(p), OK) for n, p in members] + [(n, g2_words(p), E_SUBGROUP) for n, p in outside]
    m1, mz = g2_words(members[0][1]), g2_words(members[3][1])
    rows += [("y-flipped", _flip(m1, 2), E_CURVE), ("y.c1-flipped", _flip(m1, 3), E_CURVE), ("z-flipped", _flip(mz, 4), E_CURVE),
             ("mapped-x-flipped", _flip(g2_words(mapped[0][1]), 0), E_CURVE)]
    ones = _raw((1 << 256) - 1)
    rows += [("z.c1=q", _with(m1, 5, _raw(Q)), E_RANGE),                                               # congruent to the member itself
             ("x.c0=q", _with(m1, 0, _raw(Q)), E_RANGE), ("y.c1=all-ones", _with(m1, 3, ones), E_RANGE), ("z.c0=all-ones", _with(mz, 4, ones), E_RANGE)]
    rows += [("%s-unreduced" % c, _unreduced(mz, j), E_RANGE) for j, c in enumerate(("x.c0", "x.c1", "y.c0", "y.c1", "z.c0", "z.c1"))]
    rows += [("infinity-x=q", _with(g2_words(M.g_zero(O2)), 0, _raw(Q)), E_RANGE),                     # the range check comes before z == 0
             ("range-and-curve", _with(_flip(m1, 2), 1, ones), E_RANGE), ("range-and-subgroup", _unreduced(g2_words(mapped[2][1]), 2), E_RANGE)]
    return rows


@functools.lru_cache(maxsize=None)
def g1_cases():
    """[(name, (12,) uint64 record, status)]: the analogue without the subgroup class (cofactor 1)"""
    g = M.G1_ONE
    members = [("generator", g), ("[2]G", M.g_double(O1, g)), ("[r-1]G", M.g_mul(O1, g, R - 1)), ("[k]G", M.g_mul(O1, g, 0xdeadbeefcafe)),
               ("[k]G-affine", M.g_normalize(O1, M.g_mul(O1, g, 0xdeadbeefcafe))), ("neg-[k]G", M.g_neg(O1, M.g_mul(O1, g, 0xdeadbeefcafe))),
               ("scaled", _scaled(O1, g, 0x123456789)), ("zero", M.g_zero(O1)), ("z=0-xy", (5, 7, 0)), ("all-zero", (0, 0, 0))]
    assert any(p[2] not in (0, 1) for _, p in members)
    rows = [(n, g1_words(p), OK) for n, p in members]
    m1, mz = g1_words(g), g1_words(members[3][1])
    ones = _raw((1 << 256) - 1)
    rows += [("x-flipped", _flip(m1, 0), E_CURVE), ("y-flipped", _flip(mz, 1), E_CURVE), ("z-flipped", _flip(mz, 2), E_CURVE), ("off-(1,1,1)", g1_words((1, 1, 1)), E_CURVE)]
    rows += [("x=q", _with(m1, 0, _raw(Q)), E_RANGE), ("y=all-ones", _with(m1, 1, ones), E_RANGE), ("z=q", _with(mz, 2, _raw(Q)), E_RANGE)]
    rows += [("%s-unreduced" % c, _unreduced(mz, j), E_RANGE) for j, c in enumerate("xyz")]
    rows += [("infinity-y=q", _with(g1_words(M.g_zero(O1)), 1, _raw(Q)), E_RANGE), ("range-and-curve", _with(_flip(m1, 1), 0, ones), E_RANGE)]
    return rows


def _check():
    g2, g1 = g2_cases(), g1_cases()
    for name, row, st in g2:
        assert g2_status(row) == st, name
        if st in (OK, E_SUBGROUP):                             # on the twist: the identity and [r]P == 0 agree
            assert endo_accepts(g2_point(row)) == (st == OK), name
    for name, row, st in g1:
        assert g1_status(row) == st, name
    assert {st for _, _, st in g2} == {OK, E_RANGE, E_CURVE, E_SUBGROUP} and {st for _, _, st in g1} == {OK, E_RANGE, E_CURVE}
    assert len({n for n, _, _ in g2}) == len(g2) and len({n for n, _, _ in g1}) == len(g1)


_check()


@functools.lru_cache(maxsize=None)
def g2_batch(n, start=0):
    """n records cycling the case list from `start`: ((n, 24) uint64, (n,) int32)"""
    cs = g2_cases()
    rows = [cs[(start + i) % len(cs)] for i in range(n)]
    return np.stack([r for _, r, _ in rows]) if rows else np.zeros((0, 24), np.uint64), np.array([s for _, _, s in rows], np.int32)


@functools.lru_cache(maxsize=None)
def g1_batch(n, start=0):
    cs = g1_cases()
    rows = [cs[(start + i) % len(cs)] for i in range(n)]
    return np.stack([r for _, r, _ in rows]) if rows else np.zeros((0, 12), np.uint64), np.array([s for _, _, s in rows], np.int32)
