"""TEST INFRASTRUCTURE - the integer model of the wire format (include/bn254_hip.h bn254_{fr,g1,g2}_{encode,decode}_batch and
bn254_g{1,2}_{encode,decode}_stream) and the case lists every test of the family shares (tests/test_wire_model.py and tests/test_wire_abi.py on
the CPU, tests/test_gpu_wire.py on the GPU).

Plain Python integers; neither the library nor the oracle is imported.  A G1 point is an affine pair (x, y), a G2 point ((x0, x1), (y0, y1)),
None is the point at infinity; the group law is affine chord and tangent with Fermat inverses.  A record is checked by a PRIORITY list: every
check is evaluated on its own (on the coordinates reduced into the field where they are out of range), and the first check of the list that
fails names the status.  Membership of the order-r subgroup is [r]P == O."""
import collections
import functools
import itertools

import numpy as np

_U = 4965661367192848881
Q = 36 * _U**4 + 36 * _U**3 + 24 * _U**2 + 6 * _U + 1
R = 36 * _U**4 + 36 * _U**3 + 18 * _U**2 + 6 * _U + 1
MONT = 1 << 256
RS = {1: 65, 2: 129}                     # bytes of a fixed record
WORDS = {1: 12, 2: 24}                   # uint64 words of a point
OK, E_RANGE, E_RANGE_SQUARED, E_TAG, E_CURVE, E_SUBGROUP = 0, 1, 2, 3, 4, 5
# the order in which a decoder of the reference crate meets its errors: the leading byte, then x and y as integers, then the curve equation, then
# (G2 only) the order of the point.  (name of the check, status it answers with)
PRIORITY = {1: (("tag", E_TAG), ("range", E_RANGE), ("curve", E_CURVE)),
            2: (("tag", E_TAG), ("range", E_RANGE_SQUARED), ("curve", E_CURVE), ("subgroup", E_SUBGROUP))}


# ------------------------------------------------------------------------------------------------------------------ field arithmetic
def _inv(v):
    return pow(v % Q, Q - 2, Q)


class _Fq:
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b % Q)
    inv = staticmethod(_inv)


class _Fq2:                              # Fq[u] / (u^2 + 1)
    zero, one = (0, 0), (1, 0)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q))
    mul = staticmethod(lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q))

    @staticmethod
    def inv(a):
        n = _inv(a[0] * a[0] + a[1] * a[1])
        return (a[0] * n % Q, -a[1] * n % Q)


F = {1: _Fq, 2: _Fq2}
B = {1: 3, 2: _Fq2.mul((3, 0), _Fq2.inv((9, 1)))}          # y^2 = x^3 + 3 and its twist y^2 = x^3 + 3 / (9 + u)
GEN = {1: (1, 2),
       2: ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
           (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))}


def scale(g, a, k):
    return a * k % Q if g == 1 else (a[0] * k % Q, a[1] * k % Q)


def rhs(g, x):
    f = F[g]
    return f.add(f.mul(f.mul(x, x), x), B[g])


def on_curve(g, pt):
    return pt is None or F[g].mul(pt[1], pt[1]) == rhs(g, pt[0])


def fq_sqrt(a):
    r = pow(a % Q, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def f2_sqrt(a):
    """a root of a in Fq2 or None (the complex method)"""
    if a[1] == 0:
        r = fq_sqrt(a[0])
        return (r, 0) if r is not None else (0, fq_sqrt(-a[0]))
    n = fq_sqrt(a[0] * a[0] + a[1] * a[1])
    if n is None:
        return None
    for s in (n, -n % Q):
        x0 = fq_sqrt((a[0] + s) * _inv(2))
        if x0:
            r = (x0, a[1] * _inv(2 * x0) % Q)
            assert _Fq2.mul(r, r) == a
            return r
    raise AssertionError("a square norm without a root")


# ------------------------------------------------------------------------------------------------------------------ the group law
def add(g, p, s):
    """chord and tangent on y^2 = x^3 + b for ANY b (the formulas do not name it): a pair off the curve is a point of a curve of its own"""
    f = F[g]
    if p is None:
        return s
    if s is None:
        return p
    (x1, y1), (x2, y2) = p, s
    if x1 == x2:
        if f.add(y1, y2) == f.zero:
            return None
        lam = f.mul(scale(g, f.mul(x1, x1), 3), f.inv(scale(g, y1, 2)))
    else:
        lam = f.mul(f.sub(y2, y1), f.inv(f.sub(x2, x1)))
    x3 = f.sub(f.sub(f.mul(lam, lam), x1), x2)
    return (x3, f.sub(f.mul(lam, f.sub(x1, x3)), y1))


@functools.lru_cache(maxsize=None)
def mul(g, p, k):
    acc = None
    while k:
        if k & 1:
            acc = add(g, acc, p)
        p = add(g, p, p)
        k >>= 1
    return acc


def neg(g, p):
    return None if p is None else (p[0], F[g].sub(F[g].zero, p[1]))


def in_subgroup(g, pt):
    return mul(g, pt, R) is None


def jacobian(g, pt, z):
    """the Jacobian image (x z^2, y z^3, z) of an affine point"""
    f = F[g]
    z2 = f.mul(z, z)
    return (f.mul(pt[0], z2), f.mul(pt[1], f.mul(z2, z)), z)


def normalize(g, jac):
    """Jacobian (x, y, z) -> affine point, None for z = 0 whatever x and y are"""
    f = F[g]
    x, y, z = jac
    if z == f.zero:
        return None
    zi = f.inv(z)
    zi2 = f.mul(zi, zi)
    return (f.mul(x, zi2), f.mul(y, f.mul(zi2, zi)))


# ------------------------------------------------------------------------------------------------------------------ words of the ABI
def _limbs(v, mod=Q):
    m = v * MONT % mod
    return [(m >> (64 * j)) & ((1 << 64) - 1) for j in range(4)]


def coords_words(g, cs):
    """three coordinates (any Jacobian point) as 12 / 24 uint64 Montgomery words"""
    flat = list(cs) if g == 1 else [c for two in cs for c in two]
    return np.array([l for c in flat for l in _limbs(c)], np.uint64)


def words(g, pt):
    """(x, y, 1) of an affine point, G::zero() = (0, 1, 0) for None"""
    f = F[g]
    return coords_words(g, (f.zero, f.one, f.zero) if pt is None else (pt[0], pt[1], f.one))


def fr_words(v):
    """a scalar below r as 4 uint64 Montgomery words; None (a rejected record) is Fr::zero()"""
    return np.array(_limbs(v or 0, R), np.uint64)


# ------------------------------------------------------------------------------------------------------------------ records
def coord_int(g, c):
    """a coordinate as the integer the record carries: Fq2 is c1 * q + c0"""
    return c if g == 1 else c[1] * Q + c[0]


def record(g, tag, xv, yv):
    """a fixed record of a tag and two integers below 2^256 (G1) / 2^512 (G2)"""
    w = 32 * g
    return bytes([tag]) + xv.to_bytes(w, "big") + yv.to_bytes(w, "big")


def encode(g, pt):
    """the fixed record of an affine point: infinity is tag 0 and zero padding"""
    if pt is None:
        return bytes(RS[g])
    return record(g, 4, coord_int(g, pt[0]), coord_int(g, pt[1]))


def g1_encode(pt): return encode(1, pt)
def g2_encode(pt): return encode(2, pt)


def fr_encode(v):
    assert 0 <= v < R
    return v.to_bytes(32, "big")


def _coord(g, v):
    """an integer of a record -> (in range, the element it is taken for)"""
    if g == 1:
        return v < Q, v % Q
    return v < Q * Q, (v % Q, v // Q % Q)


def parse(g, rec):
    rec = bytes(rec)
    assert len(rec) == RS[g]
    w = 32 * g
    return rec[0], int.from_bytes(rec[1:1 + w], "big"), int.from_bytes(rec[1 + w:], "big")


def failed_checks(g, rec):
    """the names of ALL the checks of PRIORITY[g] the record fails, each on its own"""
    tag, xv, yv = parse(g, rec)
    (xok, x), (yok, y) = _coord(g, xv), _coord(g, yv)
    result = {"tag": tag in (0, 4), "range": xok and yok, "curve": on_curve(g, (x, y)), "subgroup": in_subgroup(g, (x, y))}
    return frozenset(name for name, _ in PRIORITY[g] if not result[name])


def decode(g, rec):
    """-> (status, point): tag 0 is infinity whatever follows it; else the first failed check of the priority list; a rejected record is infinity"""
    tag, xv, yv = parse(g, rec)
    if tag == 0:
        return OK, None
    failed = failed_checks(g, rec)
    for name, status in PRIORITY[g]:
        if name in failed:
            return status, None
    return OK, (_coord(g, xv)[1], _coord(g, yv)[1])


def g1_decode(rec): return decode(1, rec)
def g2_decode(rec): return decode(2, rec)


def fr_decode(rec):
    v = int.from_bytes(bytes(rec), "big")
    assert len(bytes(rec)) == 32
    return (OK, v) if v < R else (E_RANGE, None)


# ------------------------------------------------------------------------------------------------------------------ the case lists
Case = collections.namedtuple("Case", "name rec status point failed")      # failed: frozenset of check names, empty for tag 0
TAGS = (0, 4, 1, 9, 255)


def _case(g, name, tag, xv, yv):
    rec = record(g, tag, xv, yv)
    st, pt = decode(g, rec)
    return Case(name, rec, st, pt, failed_checks(g, rec) if tag else frozenset())


@functools.lru_cache(maxsize=None)
def valid_points(g, count=12):
    """[k]G for k = 2 .. count + 1 and, alternating, their negatives"""
    out = []
    for k in range(2, count + 2):
        p = mul(g, GEN[g], k)
        out.append(neg(g, p) if k % 2 else p)
    assert all(on_curve(g, p) and in_subgroup(g, p) for p in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def g2_full_order_point():
    """a point of the twist outside the order-r subgroup: x = (1, 1), (2, 1), ... until x^3 + b is a square; no cofactor is cleared"""
    for a in itertools.count(1):
        x = (a, 1)
        y = f2_sqrt(rhs(2, x))
        if y is not None and not in_subgroup(2, (x, y)):
            assert on_curve(2, (x, y))
            return (x, y)


@functools.lru_cache(maxsize=None)
def g1_collision_cases():
    """the product tag x (x valid | q | 2^256 - 1) x (y valid | q | q + valid y) x (on | off the curve where both are in range)"""
    vx, vy = valid_points(1)[3]
    out = []
    for tag, (xn, xv), (yn, yv) in itertools.product(TAGS, (("valid", vx), ("q", Q), ("2^256-1", (1 << 256) - 1)), (("valid", vy), ("q", Q), ("q+valid", Q + vy))):
        out.append(_case(1, f"tag{tag}/x={xn}/y={yn}", tag, xv, yv))
        if xn == yn == "valid":
            out.append(_case(1, f"tag{tag}/x=valid/y=valid+1", tag, xv, (vy + 1) % Q))
    assert Q + vy < 1 << 256
    return tuple(out)


@functools.lru_cache(maxsize=None)
def g2_collision_cases():
    """the product tag x (x in range | + q^2) x (y in range | + q^2) x (on | off the twist) x (in | outside the subgroup), the 512-bit extremes in
    x and in y, and the coordinates (q - 1, 0) and (0, q - 1)"""
    q2 = Q * Q
    inside, outside = valid_points(2)[2], g2_full_order_point()
    out = []
    for tag, xhi, yhi, off, sub in itertools.product(TAGS, (0, 1), (0, 1), (0, 1), (0, 1)):
        x, y = outside if sub else inside
        if off:                                             # (4 x, 8 y) lies on y^2 = x^3 + 64 b, and the map is a homomorphism of the chord-and-tangent
            x, y = scale(2, x, 4), scale(2, y, 8)           # law: the pair is off the twist and of the same order as the point it came from
        name = f"tag{tag}/x{'+q^2' if xhi else ''}/y{'+q^2' if yhi else ''}/{'off' if off else 'on'}/{'outside' if sub else 'inside'}"
        out.append(_case(2, name, tag, coord_int(2, x) + xhi * q2, coord_int(2, y) + yhi * q2))
    gx, gy = GEN[2]
    for axis, (c0, c1), other in (("x", gx, coord_int(2, gy)), ("y", gy, coord_int(2, gx))):
        extremes = (("q^2", q2), ("q^2+q-1", q2 + Q - 1), ("2^512-1", (1 << 512) - 1), ("q*2^256", Q << 256), ("q*2^256+c0", (Q << 256) + c0),
                    ("q*(2^256+c1)+c0", Q * ((1 << 256) + c1) + c0), ("(q-1)*q+q", (Q - 1) * Q + Q))
        for name, v in extremes:
            assert q2 <= v < 1 << 512
            c = _case(2, f"extreme/{axis}={name}", 4, *((v, other) if axis == "x" else (other, v)))
            assert c.status == E_RANGE_SQUARED
            out.append(c)
    for name, x in (("c1=0,c0=q-1", (Q - 1, 0)), ("c1=q-1,c0=0", (0, Q - 1))):
        y = f2_sqrt(rhs(2, x))
        xv = coord_int(2, x)
        out.append(_case(2, f"limit/{name}/tag0", 0, xv, coord_int(2, y) if y is not None else xv))
        assert out[-1].status == OK
        if y is not None:                                   # a point of the twist: accepted where it is of order r, else rejected for that alone
            out.append(_case(2, f"limit/{name}/tag4", 4, xv, coord_int(2, y)))
            assert out[-1].status in (OK, E_SUBGROUP)
        out.append(_case(2, f"limit/{name}/y", 4, coord_int(2, GEN[2][0]), xv))          # the same integer as y under the generator's x: in range, off the twist
        assert out[-1].status == E_CURVE
    return tuple(out)


def collision_cases(g):
    return g1_collision_cases() if g == 1 else g2_collision_cases()


@functools.lru_cache(maxsize=None)
def fr_cases():
    """(name, 32 bytes, status, value or None)"""
    top = int.from_bytes(b"\0" + R.to_bytes(32, "big")[1:], "big")
    vals = (("0", 0), ("1", 1), ("r-1", R - 1), ("r", R), ("r+1", R + 1), ("2^256-1", (1 << 256) - 1), ("2^255", 1 << 255), ("r, top byte zeroed", top))
    assert top < R
    return tuple((name, v.to_bytes(32, "big")) + fr_decode(v.to_bytes(32, "big")) for name, v in vals)


def separating_cases(g):
    """{(check, next check): [cases that fail exactly these two]} for every adjacent pair of the priority list"""
    names = [n for n, _ in PRIORITY[g]]
    return {(a, b): [c for c in collision_cases(g) if c.failed == {a, b}] for a, b in zip(names, names[1:])}


# ------------------------------------------------------------------------------------------------------------------ batches
def decode_batch(g, n, start=0):
    """n records: valid points and the collision cases in turn -> (uint8 (n, rs), int32 statuses, uint64 points)"""
    cases, good = collision_cases(g), valid_points(g)
    rows = []
    for i in range(n):
        j = start + i
        rows.append((encode(g, good[(j // 2) % len(good)]), OK, good[(j // 2) % len(good)]) if j % 2 == 0 else cases[(j // 2) % len(cases)][1:4])
    return (np.stack([np.frombuffer(r[0], np.uint8) for r in rows]), np.array([r[1] for r in rows], np.int32), np.stack([words(g, r[2]) for r in rows]))


def encode_batch(g, n, start=0):
    """n Jacobian points - normalised, with z = 2, q - 1 and a large z, infinity as (0, 1, 0) and as (x, y, 0) with x, y != 0
    -> (uint64 (n, words), uint8 records, uint64 normalised points)"""
    f, good = F[g], valid_points(g)
    big = (Q - 12345) if g == 1 else (Q - 2, 0x1234567 << 200)
    zs = (f.one, scale(g, f.one, 2), None, scale(g, f.one, Q - 1), big, "dirty")
    rows = []
    for i in range(n):
        j = start + i
        pt, z = good[j % len(good)], zs[j % len(zs)]
        if z is None:
            rows.append(((f.zero, f.one, f.zero), None))
        elif z == "dirty":
            rows.append(((pt[0], pt[1], f.zero), None))
        else:
            rows.append((jacobian(g, pt, z), pt))
        assert normalize(g, rows[-1][0]) == rows[-1][1]
    return (np.stack([coords_words(g, r[0]) for r in rows]), np.stack([np.frombuffer(encode(g, r[1]), np.uint8) for r in rows]),
            np.stack([words(g, r[1]) for r in rows]))


def fr_batch(n, start=0):
    """n Fr records: the edge cases and small multiples of a large value in turn -> (uint8 (n, 32), int32 statuses, uint64 words)"""
    cases = fr_cases()
    rows = []
    for i in range(n):
        j = start + i
        if j % 2:
            rows.append(cases[(j // 2) % len(cases)][1:])
        else:
            v = (j + 1) * 0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251f86c6a11d0c18e95 % R
            rows.append((fr_encode(v), OK, v))
    return (np.stack([np.frombuffer(r[0], np.uint8) for r in rows]), np.array([r[1] for r in rows], np.int32), np.stack([fr_words(r[2]) for r in rows]))


# ------------------------------------------------------------------------------------------------------------------ streams
def stream_encode(g, points):
    """the crate's stream: infinity is the lone byte 0"""
    return b"".join(b"\0" if p is None else encode(g, p) for p in points)


def stream_decode(g, data, max_points=None, stop=False):
    """-> (count, statuses, consumed, points): record after record - tag 4 takes a full record, any other tag its one byte; a record cut short by
    the end of the stream ends the call in front of it; with `stop` the first record that is not accepted is the last one of the call"""
    data = bytes(data)
    pos, statuses, points = 0, [], []
    while pos < len(data) and (max_points is None or len(statuses) < max_points):
        size = RS[g] if data[pos] == 4 else 1
        if pos + size > len(data):
            break
        st, pt = decode(g, data[pos:pos + size].ljust(RS[g], b"\0"))
        statuses.append(st); points.append(pt)
        pos += size
        if stop and st != OK:
            break
    return len(statuses), statuses, pos, points


StreamCase = collections.namedtuple("StreamCase", "name data max_points default stop")       # default, stop: (count, statuses, consumed, points)


@functools.lru_cache(maxsize=None)
def stream_cases(g):
    rs = RS[g]
    good = [encode(g, p) for p in valid_points(g)[:4]]
    curve = next(c.rec for c in collision_cases(g) if c.status == E_CURVE and c.rec[0] == 4)
    rows = [("empty", b"", None), ("lone 00", b"\0", None), ("lone 04", b"\4", None), ("lone 09", b"\t", None)]
    offsets = range(1, rs) if g == 1 else (1, 2, 32, 33, 64, 65, rs - 1)
    for at in offsets:
        rows.append((f"one record cut at {at}", good[0][:at], None))
        rows.append((f"second record cut at {at}", good[1] + good[0][:at], None))
    rows.append(("00 00 04..", b"\0\0" + good[2], None))
    rows.append(("00 00 04.. cut", b"\0\0" + good[2][:rs - 1], None))
    rows.append(("bad tag in the middle", good[0] + b"\t" + good[1] + b"\0" + good[2], None))
    rows.append(("off the curve in the middle", good[0] + b"\0" + curve + good[1] + b"\xff" + good[3], None))
    recs = [good[0], b"\0", good[1], b"\t", good[2], b"\0", curve, good[3]]        # k = 8 records; the first bad one is record 3
    k, data = len(recs), b"".join(recs)
    for m in (0, 3, 4, 5, k - 1, k, k + 1):
        rows.append((f"max_points={m} of {k}", data, m))
    rows.append((f"max_points={k} and a cut tail", data + good[0][:7], k))
    return tuple(StreamCase(name, d, m, stream_decode(g, d, m, False), stream_decode(g, d, m, True)) for name, d, m in rows)
