"""TEST INFRASTRUCTURE - the integer model of the compressed G1 / G2 encodings (include/bn254_hip.h bn254_g{1,2}_compress_batch /
_decompress_batch) and the case lists every test of the family shares: both byte layouts, the sign rule, the order of the checks, the square
roots by pow(a, (q + 1) / 4, q).  Points are affine tuples of canonical integers ((x, y) for G1, ((x0, x1), (y0, y1)) for G2), None is the
point at infinity; `words` turns one into the ABI's (x, y, 1) Montgomery image."""
import functools

import numpy as np

import bn_model as M

Q = M.Q
ARK, GNARK = 0, 1
FORMATS = {"ark": ARK, "gnark": GNARK}
BYTES = {1: 32, 2: 64}
OK, E_RANGE, E_FLAGS, E_CURVE, E_SUBGROUP = 0, 1, 3, 4, 5


# ------------------------------------------------------------------------------------------------------------------ field arithmetic
def fq_sqrt(a):
    r = pow(a % Q, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def fq_is_square(a):
    return a % Q == 0 or pow(a % Q, (Q - 1) // 2, Q) == 1


def f2_sqrt(a):
    """a root of a in Fq2 = Fq[u] / (u^2 + 1), or None (the complex method; which of the two roots is not specified)"""
    a = (a[0] % Q, a[1] % Q)
    if a[1] == 0:
        r = fq_sqrt(a[0])
        if r is not None:
            return (r, 0)
        return (0, fq_sqrt(-a[0]))                     # -1 is a non-residue: exactly one of a0, -a0 is a square
    n = fq_sqrt(a[0] * a[0] + a[1] * a[1])
    if n is None:
        return None
    for s in (n, -n % Q):
        x0 = fq_sqrt((a[0] + s) * M.TWO_INV)
        if x0:
            x1 = a[1] * M.inv(2 * x0) % Q
            assert M.f2_sqr((x0, x1)) == a
            return (x0, x1)
    raise AssertionError("a square norm without a root")


def f2_is_square(a):
    return fq_is_square(a[0] * a[0] + a[1] * a[1])


def fq_sign(y):
    """1 iff y > -y as canonical integers"""
    return int(y % Q > (Q - 1) // 2)


def f2_sign(y):
    return fq_sign(y[1]) if y[1] % Q else fq_sign(y[0])


def rhs(g, x):
    return (x * x * x + M.G1_B) % Q if g == 1 else M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.G2_B)


@functools.lru_cache(maxsize=None)
def g2_in_subgroup(x, y):
    return M.g_is_zero(M.FQ2_OPS, M.g_mul(M.FQ2_OPS, (x, y, M.F2_ONE), M.R_ORD))


# ------------------------------------------------------------------------------------------------------------------ the two layouts
def render(g, comps, flags, fmt):
    """comps: the integers of x (G1: [x]; G2: [c0, c1]), each below 2^256 and the last below 2^254; flags: 'sign0', 'sign1', 'inf' or 'bad'"""
    assert len(comps) == g and comps[-1] < 1 << 254 and all(c < 1 << 256 for c in comps)
    if fmt == ARK:
        b = bytearray(b"".join(c.to_bytes(32, "little") for c in comps))
        b[-1] |= {"sign0": 0, "inf": 1, "sign1": 2, "bad": 3}[flags] << 6
    else:
        b = bytearray(b"".join(c.to_bytes(32, "big") for c in reversed(comps)))
        b[0] |= {"bad": 0, "inf": 1, "sign0": 2, "sign1": 3}[flags] << 6
    return bytes(b)


def parse(g, b, fmt):
    """-> (comps, flags_ok, inf, sign)"""
    assert len(b) == BYTES[g]
    if fmt == ARK:
        comps = [int.from_bytes(b[32 * j:32 * j + 32], "little") for j in range(g)]
    else:
        comps = [int.from_bytes(b[32 * (g - 1 - j):32 * (g - j)], "big") for j in range(g)]
    f = comps[-1] >> 254
    comps[-1] &= (1 << 254) - 1
    if fmt == ARK:
        return comps, f != 3, bool(f & 1), bool(f >> 1)
    return comps, f != 0, f == 1, f == 3


def compress(g, pt, fmt):
    """canonical bytes of an affine point (None: infinity)"""
    if pt is None:
        return render(g, [0] * g, "inf", fmt)
    x, y = pt
    return render(g, [x] if g == 1 else list(x), "sign%d" % (fq_sign(y) if g == 1 else f2_sign(y)), fmt)


def decompress(g, b, fmt):
    """-> (status, point): the checks in the order flags, range, curve, subgroup; a rejected record is the point at infinity"""
    comps, ok, inf, sign = parse(g, bytes(b), fmt)
    if not ok or (inf and any(comps)):
        return E_FLAGS, None
    if inf:
        return OK, None
    if any(c >= Q for c in comps):
        return E_RANGE, None
    x = comps[0] if g == 1 else tuple(comps)
    y = fq_sqrt(rhs(1, x)) if g == 1 else f2_sqrt(rhs(2, x))
    if y is None:
        return E_CURVE, None
    if g == 1:
        y = y if fq_sign(y) == sign else -y % Q
    else:
        y = y if f2_sign(y) == sign else M.f2_neg(y)
    if g == 2 and not g2_in_subgroup(x, y):
        return E_SUBGROUP, None
    return OK, (x, y)


def words(g, pt):
    """the ABI image: (x, y, 1) in Montgomery form as 12 / 24 uint64, G::zero() = (0, 1, 0) for None"""
    if g == 1:
        cs = [0, 1, 0] if pt is None else [pt[0], pt[1], 1]
    else:
        cs = [0, 0, 1, 0, 0, 0] if pt is None else [pt[0][0], pt[0][1], pt[1][0], pt[1][1], 1, 0]
    return np.array([l for c in cs for l in M.to_mont_limbs(c)], np.uint64)


def jacobian_words(g, p):
    """a Jacobian model point (x, y, z) as the ABI image, unnormalised"""
    cs = list(p) if g == 1 else [c for two in p for c in two]
    return np.array([l for c in cs for l in M.to_mont_limbs(c)], np.uint64)


def affine(g, p):
    """Jacobian model point -> affine tuple or None"""
    return M.g_to_affine(M.FQ_OPS if g == 1 else M.FQ2_OPS, p)


# ------------------------------------------------------------------------------------------------------------------ the case lists
@functools.lru_cache(maxsize=None)
def multiples(g, count=8):
    """[k]G for k = 1 .. count and their negatives, affine"""
    o, one = (M.FQ_OPS, M.G1_ONE) if g == 1 else (M.FQ2_OPS, M.G2_ONE)
    out = []
    for k in range(1, count + 1):
        p = M.g_mul(o, one, k)
        out += [affine(g, p), affine(g, M.g_neg(o, p))]
    return out


@functools.lru_cache(maxsize=None)
def x_without_point(g, count=4):
    """the first x values with x^3 + b not a square (of x = 1 .. 200, 87 have no point on G1: found by search)"""
    if g == 1:
        xs = [x for x in range(1, 201) if not fq_is_square(rhs(1, x))]
        assert len(xs) == 87
        return xs[:count]
    xs = [(a, b) for a in range(1, 12) for b in range(0, 3) if not f2_is_square(rhs(2, (a, b)))]
    return xs[:count]


@functools.lru_cache(maxsize=None)
def g2_outside_subgroup():
    """a point on the twist that is not in the order-r subgroup, found as tests/conftest.py finds its own: x = (5, 1), (6, 1), ..."""
    x = (5, 1)
    while True:
        y = f2_sqrt(rhs(2, x))
        if y is not None and not g2_in_subgroup(x, y):
            return (x, y)
        x = (x[0] + 1, x[1])


@functools.lru_cache(maxsize=None)
def abstract_cases(g):
    """(name, comps, flags) rows, rendered per format by `records`"""
    rows = []
    comps = (lambda x: [x]) if g == 1 else (lambda x: list(x))
    for i, pt in enumerate(multiples(g)):
        x, y = pt
        rows.append(("mult%d%s" % (i // 2 + 1, "-" if i % 2 else "+"), comps(x), "sign%d" % (fq_sign(y) if g == 1 else f2_sign(y))))
    rows.append(("infinity", [0] * g, "inf"))
    for x in x_without_point(g):
        rows += [("nopoint%s/0" % (x,), comps(x), "sign0"), ("nopoint%s/1" % (x,), comps(x), "sign1")]
    gx = multiples(g)[0][0]
    for j in range(g):                                     # a component out of range, each component on its own
        for name, v in (("q", Q), ("q+1", Q + 1), ("2^254-1", (1 << 254) - 1)):
            c = comps(gx); c[j] = v
            rows.append(("range[%d]=%s" % (j, name), c, "sign0"))
    if g == 2:                                             # c0 has no flag bits: all 256 of them are the integer
        rows.append(("range[0]=2^256-1", [(1 << 256) - 1, gx[1]], "sign1"))
    for fl in ("sign0", "sign1", "inf", "bad"):            # all four flag patterns on the generator's x (the first two are the point and its negative)
        rows.append(("flags=%s" % fl, comps(gx), fl))
    stray = [0] * g; stray[0] = 1 << 77
    rows.append(("infinity+stray", stray, "inf"))
    if g == 2:
        rows.append(("infinity+stray-c1", [0, 1], "inf"))
    bad_range = comps(gx); bad_range[-1] = Q + 5           # flags come before range, range before curve
    rows.append(("bad+range", bad_range, "bad"))
    rows.append(("bad+nopoint", comps(x_without_point(g)[0]), "bad"))
    nopoint_range = comps(x_without_point(g)[0]); nopoint_range[0] += Q
    rows.append(("range+nopoint", nopoint_range, "sign0"))
    if g == 2:
        x, y = g2_outside_subgroup()
        rows += [("outside/%d" % s, list(x), "sign%d" % s) for s in (0, 1)]
    return rows


@functools.lru_cache(maxsize=None)
def records(g, fmt):
    """[(name, bytes, status, point)]: every case in one layout with what the model decodes it to"""
    out = []
    for name, comps, flags in abstract_cases(g):
        b = render(g, list(comps), flags, fmt)
        st, pt = decompress(g, b, fmt)
        out.append((name, b, st, pt))
    return out


def batch(g, fmt, n, start=0):
    """n records cycling the case list from `start`: (uint8 (n, bytes), int32 statuses, uint64 points)"""
    recs = records(g, fmt)
    rows = [recs[(start + i) % len(recs)] for i in range(n)]
    return (np.stack([np.frombuffer(r[1], np.uint8) for r in rows]), np.array([r[2] for r in rows], np.int32),
            np.stack([words(g, r[3]) for r in rows]))


def accepted(g, fmt):
    return [r for r in records(g, fmt) if r[2] == OK]


def rejected(g, fmt):
    return [r for r in records(g, fmt) if r[2] != OK]
