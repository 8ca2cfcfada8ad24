"""TEST INFRASTRUCTURE - the integer model and the inputs of the Grumpkin tests (tests/test_grumpkin_model.py, tests/test_hostsim_grumpkin.py and
tests/test_grumpkin_abi.py on the CPU, tests/test_gpu_grumpkin.py and tests/test_gpu_pedersen_ipa.py on the GPU).

The model is written independently of bn_amd/grumpkin.py: affine chord and tangent with Fermat inverses and a right-to-left scalar
multiplication (the package goes left to right).  O is (0, 0).  The expected bytes of a point are the Montgomery images of its coordinates,
unique because every result is canonical; a scalar is its plain little-endian words."""
import functools

import numpy as np

import fr_cases as FC

R = FC.R
_U = 4965661367192848881
Q = 36 * _U**4 + 36 * _U**3 + 24 * _U**2 + 6 * _U + 1
B_COEFF = R - 17
B3 = 3 * B_COEFF % R
O = (0, 0)
G = (1, 17631683881184975370165255887551781615748388533673675138860)
ST_OK, ST_RANGE, ST_CURVE = 0, 1, 4


def inv(v):
    return pow(v % R, R - 2, R)


def on_curve(p):
    x, y = p
    return p == O or (y * y - x * x * x - B_COEFF) % R == 0


def neg(p):
    return (p[0], (R - p[1]) % R)


def add(p, q):
    if p == O:
        return q
    if q == O:
        return p
    x1, y1 = p; x2, y2 = q
    if x1 == x2:
        if (y1 + y2) % R == 0:
            return O
        lam = 3 * x1 * x1 % R * inv(2 * y1) % R
    else:
        lam = (y2 - y1) * inv(x2 - x1) % R
    x3 = (lam * lam - x1 - x2) % R
    return (x3, (lam * (x1 - x3) - y1) % R)


_DOUBLINGS = {}            # G -> [G, 2G, 4G, ..]: the many multiples of G the cases need share their doublings


def mul(p, k):
    """[k]p, right to left"""
    runs = _DOUBLINGS.setdefault(p, [p]) if p == G else [p]
    acc, i = O, 0
    while k:
        if i == len(runs):
            runs.append(add(runs[-1], runs[-1]))
        if k & 1:
            acc = add(acc, runs[i])
        k >>= 1; i += 1
    return acc


def msm(points, ks):
    acc = O
    for p, k in zip(points, ks):
        acc = add(acc, mul(p, k))
    return acc


# ---- the projective formulas of the device (Renes-Costello-Batina 2016, a = 0), in Python integers on (X : Y : Z), O = (0 : 1 : 0)
def to_proj(p):
    return (0, 1, 0) if p == O else (p[0], p[1], 1)


def from_proj(P):
    X, Y, Z = P
    zi = inv(Z) if Z % R else 0
    return (X * zi % R, Y * zi % R)


def proj_add(P, S):
    X1, Y1, Z1 = P; X2, Y2, Z2 = S
    t0, t1, t2 = X1 * X2 % R, Y1 * Y2 % R, Z1 * Z2 % R
    t3 = ((X1 + Y1) * (X2 + Y2) - t0 - t1) % R
    t4 = ((Y1 + Z1) * (Y2 + Z2) - t1 - t2) % R
    t5 = ((X1 + Z1) * (X2 + Z2) - t0 - t2) % R
    x3, u = 3 * t0 % R, B3 * t2 % R
    z3, w, y3 = (t1 + u) % R, (t1 - u) % R, B3 * t5 % R
    return ((t3 * w - t4 * y3) % R, (w * z3 + y3 * x3) % R, (z3 * t4 + x3 * t3) % R)


def proj_double(P):
    X, Y, Z = P
    t0 = Y * Y % R
    z8 = 8 * t0 % R
    t1, t2 = Y * Z % R, B3 * Z * Z % R
    xa, ya, z3 = t2 * z8 % R, (t0 + t2) % R, t1 * z8 % R
    t0b = (t0 - 3 * t2) % R
    return (2 * t0b * (X * Y % R) % R, (xa + t0b * ya) % R, z3)


def proj_eq(P, S):
    return all((P[i] * S[j] - P[j] * S[i]) % R == 0 for i, j in ((0, 1), (0, 2), (1, 2)))


# ---- edge points
@functools.lru_cache(maxsize=None)
def edge_points():
    """[(name, point)]: O, G, -G, [2]G, [q-1]G, a multiple of G - and a point whose y is r - 1 if a short search finds one (x^3 = 18)"""
    out = [("O", O), ("G", G), ("negG", neg(G)), ("2G", mul(G, 2)), ("(q-1)G", mul(G, Q - 1)), ("P", mul(G, 0x123456789abcdef))]
    x = cube_root(18)
    if x is not None:
        out.append(("y=r-1", (x, R - 1)))
    assert all(on_curve(p) for _, p in out) and mul(G, Q - 1) == neg(G)
    return out


def cube_root(v):
    """a cube root of v mod r or None: r = 1 mod 3, so a third of the residues have one; 3 does not divide (r - 1) / 3, so the inverse of 3
    mod (r - 1) / 3 gives the root directly"""
    m = (R - 1) // 3
    if pow(v, m, R) != 1 or m % 3 == 0:
        return None
    x = pow(v, pow(3, -1, m), R)
    return x if pow(x, 3, R) == v % R else None


OFF_CURVE = (G[0], (G[1] + 1) % R)
RAW_OUT_OF_RANGE = [(R, 1), (0, R), (R + 1, G[1]), (G[0], (1 << 256) - 1), ((1 << 256) - 1, (1 << 256) - 1)]

# ---- edge scalars: small ones, the seams of the 4-bit windows, around q, r (which is below q), the top of the 256-bit range, all nibbles 15
# (every window adds [15]P), only the top nibble set (the chain starts from a table entry and adds O sixty-three times)
EDGE_SCALARS = [0, 1, 2, 15, 16, Q - 1, Q, Q + 1, R, 1 << 255, (1 << 256) - 1, int("f" * 64, 16), 0xf << 252, 0x8 << 252, (1 << 128) + 1, 0xf << 100]
assert R < Q < 1 << 254 and all(0 <= k < 1 << 256 for k in EDGE_SCALARS)


def raw_rows(vals):
    """256-bit integers -> (n, 4) uint64: the Montgomery image for a value below r, the value's own words (never below r) otherwise"""
    out = np.zeros((len(vals), 4), np.uint64)
    for i, v in enumerate(vals):
        m = v * FC.MONT % R if v < R else v
        out[i] = [(m >> (64 * j)) & ((1 << 64) - 1) for j in range(4)]
    return out


def point_rows(points):
    """[(x, y)] of 256-bit integers -> (n, 2, 4) uint64"""
    return raw_rows([c for p in points for c in p]).reshape(len(points), 2, 4)


def scalar_rows(ks):
    """integers below 2^256 -> (n, 4) uint64: the plain words"""
    return np.array([[(k >> (64 * j)) & ((1 << 64) - 1) for j in range(4)] for k in ks], np.uint64).reshape(len(ks), 4)


def validate_status(x, y):
    """of two 256-bit integers as the words of a record hold them"""
    if x >= R or y >= R:
        return ST_RANGE
    return ST_OK if on_curve((x, y)) else ST_CURVE


def validate_cases():
    """(points as raw integer pairs, expected statuses)"""
    pts = [p for _, p in edge_points()] + [OFF_CURVE, (0, 1), (1, 0)] + RAW_OUT_OF_RANGE
    st = [validate_status(*p) for p in pts]
    assert set(st) == {0, 1, 4}
    return pts, st


def rand256(rng):
    return int.from_bytes(rng.bytes(32), "little")


@functools.lru_cache(maxsize=None)
def curve_points(n, seed):
    """n points of the curve: the edge points first, then random multiples of G"""
    rng = np.random.default_rng(seed)
    out = [p for _, p in edge_points()]
    while len(out) < n:
        out.append(mul(G, rand256(rng) % Q))
    return tuple(out[:n])


@functools.lru_cache(maxsize=None)
def scalars(n, seed):
    """n scalars: the edge scalars first, then random 256-bit integers (most are above q)"""
    rng = np.random.default_rng(seed)
    return tuple(EDGE_SCALARS[i] if i < len(EDGE_SCALARS) else rand256(rng) for i in range(n))


@functools.lru_cache(maxsize=None)
def msm_cases():
    """(points, scalars, offsets, expected points): ONE call whose segments have 0, 1, 2, 15, 16, 17, 256 and 257 terms (16 and 17 straddle
    one fold lane, 257 forces two fold levels), then a segment whose terms cancel to O, a segment of equal points (the fold doubles), a segment
    of O points and zero scalars, and a last empty one.  The scalars of the long segments are small, so that the model stays quick; the
    short ones take the edge scalars."""
    rng = np.random.default_rng(2025)
    base = curve_points(24, 7)
    pts, ks, offs = [], [], [0]
    def seg(p, k):
        pts.extend(p); ks.extend(k); offs.append(len(pts))
    for L in (0, 1, 2, 15, 16, 17, 256, 257):
        p = [base[(i * 5 + L) % len(base)] for i in range(L)]
        k = [EDGE_SCALARS[(i + L) % len(EDGE_SCALARS)] for i in range(L)] if L <= 17 else [int(rng.integers(0, 1 << 16)) for _ in range(L)]
        seg(p, k)
    P = base[9]
    seg([P, neg(P), G, G, neg(G)], [5, 5, 3, Q - 2, 1])                       # 5P - 5P + 3G - 2G - G = O
    seg([P] * 4, [7] * 4)                                                     # four equal partial sums: every fold addition is a doubling
    seg([O, O, G, P], [9, 0, 0, Q])                                           # O points, zero scalars and a multiple of q
    seg([], [])
    want = [msm(pts[a:b], ks[a:b]) for a, b in zip(offs, offs[1:])]
    assert want[8] == O and want[10] == O and want[0] == O and want[9] == mul(P, 28)
    return tuple(pts), tuple(ks), tuple(offs), tuple(want)
