"""Grumpkin: the curve y^2 = x^3 - 17 over the scalar field Fr of BN254, the other half of the BN254 curve cycle - its constants, the group law
in host integers, a small Point type, and the batch calls on the GPU (bn_amd.grumpkin_validate_batch / grumpkin_add_batch /
grumpkin_mul_batch / grumpkin_msm_batch).

    base field Fr (modulus r);  order q, the base field modulus of BN254: prime, so the cofactor is 1 and every point of the curve but O generates
    the group;  O = the point at infinity, written (0, 0) - which is not on the curve: -17 is a non-residue mod r, so no point has x = 0;
    -(x, y) = (x, -y);  G = (1, sqrt(-16)), the root that is not above (r - 1) / 2

A point travels as two consecutive Fr (x then y, Montgomery words, affine): (n, 2, 4) uint64 in numpy, the same as Baby Jubjub; infinity is
sixteen zero words.  A SCALAR is a plain integer below 2^256 as 32 little-endian bytes - (n, 4) uint64, NOT a Montgomery image: the scalar
field of this curve is Fq, which the library has no type for.  [k]P is computed for the integer k as it stands, so k and k mod q give the same
point.  Nothing here is downloaded or pasted: the constants are the integers below and tools/gen_grumpkin_constants.py derives the device
header from them."""
import numpy as np

from .api import Q_MOD, R_MOD, Fr, _limbs, _mont, grumpkin_validate_batch, grumpkin_add_batch, grumpkin_mul_batch, grumpkin_msm_batch

Q = Q_MOD                       # the group order: scalars live mod q
R = R_MOD                       # the base field: coordinates live mod r
B = -17
IDENTITY = (0, 0)
G = (1, 17631683881184975370165255887551781615748388533673675138860)
STATUS = {0: "valid", 1: "a coordinate is out of range", 4: "not on the curve"}


def on_curve_host(p):
    """a point of the curve, O = (0, 0) included"""
    x, y = p
    return 0 <= x < R and 0 <= y < R and (p == IDENTITY or (y * y - x * x * x - B) % R == 0)


def neg_host(p):
    return (p[0], -p[1] % R)


def add_host(p, q):
    """the sum of two points of the curve by chord and tangent, in host integers"""
    if p == IDENTITY:
        return q
    if q == IDENTITY:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % R == 0:
            return IDENTITY
        lam = 3 * x1 * x1 * pow(2 * y1, -1, R) % R
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, R) % R
    x3 = (lam * lam - x1 - x2) % R
    return (x3, (lam * (x1 - x3) - y1) % R)


def mul_host(p, k):
    """[k]p for any integer k >= 0, in host integers"""
    acc = IDENTITY
    for bit in bin(int(k))[2:]:
        acc = add_host(acc, acc)
        if bit == "1":
            acc = add_host(acc, p)
    return acc


def point_limbs(p):
    """(x, y) integers -> (2, 4) uint64 Montgomery words; O = (0, 0) gives zeros"""
    return np.stack([_mont(p[0], R), _mont(p[1], R)])


def scalar_rows(ks):
    """integers below 2^256 -> (n, 4) uint64, the plain little-endian words (no Montgomery form, no reduction)"""
    ks = [int(k.v) if isinstance(k, Fr) else int(k) for k in ks]
    if any(not 0 <= k < 1 << 256 for k in ks):
        raise ValueError("a scalar is an integer in [0, 2^256)")
    return np.stack([_limbs(k) for k in ks]) if ks else np.zeros((0, 4), np.uint64)


def _point_array(points):
    if isinstance(points, np.ndarray):
        return np.asarray(points, np.uint64).reshape(-1, 2, 4)
    points = list(points)
    return np.stack([p.limbs if isinstance(p, Point) else point_limbs(p) for p in points]) if points else np.zeros((0, 2, 4), np.uint64)


def _scalar_array(scalars):
    if isinstance(scalars, np.ndarray):
        return np.asarray(scalars, np.uint64).reshape(-1, 4)
    return scalar_rows(scalars)


class Point:
    """an affine point (x, y) as two integers mod r, O = (0, 0).  + - * run on the GPU (one lane each; arrays have the batch calls), == compares
    coordinates"""
    __slots__ = ("x", "y")

    def __init__(self, x, y):
        self.x, self.y = int(x) % R, int(y) % R

    @staticmethod
    def identity(): return Point(*IDENTITY)
    @staticmethod
    def generator(): return Point(*G)
    @staticmethod
    def from_limbs(l):
        l = np.asarray(l, np.uint64).reshape(2, 4)
        return Point(Fr.from_limbs(l[0]).v, Fr.from_limbs(l[1]).v)
    @property
    def limbs(self): return point_limbs((self.x, self.y))
    def is_valid(self):
        """on the curve, O included (status 0 of grumpkin_validate_batch); the cofactor is 1, so there is nothing else to check"""
        return int(grumpkin_validate_batch([self])[0]) == 0
    def __add__(self, o): return grumpkin_add_batch([self], [o])[0]
    def __neg__(self): return Point(self.x, -self.y)
    def __sub__(self, o): return self + (-o)
    def __mul__(self, k): return grumpkin_mul_batch([self], [k])[0]
    __rmul__ = __mul__
    def __eq__(self, o): return isinstance(o, Point) and (self.x, self.y) == (o.x, o.y)
    def __hash__(self): return hash((self.x, self.y))
    def __repr__(self): return f"Point({self.x}, {self.y})"


def msm(points, scalars, engine=None):
    """sum of [scalars[i]] points[i] -> Point: one grumpkin_msm_batch of one segment; no terms give O"""
    P, K = _point_array(points), _scalar_array(scalars)
    if P.shape[0] != K.shape[0]:
        raise ValueError(f"{P.shape[0]} points, {K.shape[0]} scalars")
    return grumpkin_msm_batch(P, K, [0, P.shape[0]], engine=engine)[0]
