"""Baby Jubjub: the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over the scalar field Fr of BN254 (a = 168700, d = 168696) that circomlib,
iden3 and the Hermez-style rollups sign on - its constants, the group law in host integers, a small Point type, and the batch calls on the GPU
(bn_amd.bjj_validate_batch / bjj_add_batch / bjj_mul_batch).

    identity O = (0, 1);  -(x, y) = (-x, y);  order 8 l, l a 251-bit prime;  G of order 8 l, B8 = [8]G of order l
    (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2))

a is a square mod r and d is not, so the law is complete: no exceptional inputs, doubling is the same formula.  A point travels as two
consecutive Fr (x then y, Montgomery words, affine): (n, 2, 4) uint64 in numpy.  Nothing here is downloaded or pasted: the constants are the
integers below and tools/gen_babyjub_constants.py derives the device header from them."""
import numpy as np

from .api import R_MOD, Fr, _limbs, _mont, _scalar_array, bjj_validate_batch, bjj_add_batch, bjj_mul_batch

A = 168700
D = 168696
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041            # the prime order of B8 (251 bits)
ORDER = 8 * L
IDENTITY = (0, 1)
G = (995203441582195749578291179787384436505546430278305826713579947235728471134, 5472060717959818805561601436314318772137091100104008585924551046643952123905)
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553, 16950150798460657717958625567821834550301663161624707787222815936182638968203)
STATUS = {0: "valid", 1: "a coordinate or scalar is out of range", 4: "not on the curve", 5: "on the curve but not of an order dividing l", 6: "the signature equation fails"}


def on_curve_host(p):
    x, y = p
    return 0 <= x < R_MOD and 0 <= y < R_MOD and (A * x * x + y * y - 1 - D * x * x * y * y) % R_MOD == 0


def add_host(p, q):
    """the complete affine sum of two points of the curve, in host integers"""
    (x1, y1), (x2, y2) = p, q
    k = D * x1 * x2 * y1 * y2 % R_MOD
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, R_MOD) % R_MOD, (y1 * y2 - A * x1 * x2) * pow(1 - k, -1, R_MOD) % R_MOD)


def neg_host(p):
    return (-p[0] % R_MOD, p[1])


def mul_host(p, k):
    """[k]p for any integer k >= 0 and any point of the curve, in host integers"""
    acc = IDENTITY
    for bit in bin(int(k))[2:]:
        acc = add_host(acc, acc)
        if bit == "1":
            acc = add_host(acc, p)
    return acc


def point_limbs(p):
    """(x, y) integers -> (2, 4) uint64 Montgomery words"""
    return np.stack([_mont(p[0], R_MOD), _mont(p[1], R_MOD)])


def raw_limbs(x, y):
    """two 256-bit integers as Montgomery images that are NOT reduced: the words are (v * 2^256 mod r) only for v < r, and v's own otherwise"""
    return np.stack([_mont(v, R_MOD) if v < R_MOD else _limbs(v) for v in (x, y)])


def _point_array(points):
    if isinstance(points, np.ndarray):
        return np.asarray(points, np.uint64).reshape(-1, 2, 4)
    points = list(points)
    return np.stack([p.limbs if isinstance(p, Point) else point_limbs(p) for p in points]) if points else np.zeros((0, 2, 4), np.uint64)


class Point:
    """an affine point (x, y) as two integers mod r.  + - * run on the GPU (one lane each; arrays have the batch calls), == compares coordinates"""
    __slots__ = ("x", "y")

    def __init__(self, x, y):
        self.x, self.y = int(x) % R_MOD, int(y) % R_MOD

    @staticmethod
    def identity(): return Point(*IDENTITY)
    @staticmethod
    def generator(): return Point(*G)
    @staticmethod
    def base(): return Point(*B8)
    @staticmethod
    def from_limbs(l):
        l = np.asarray(l, np.uint64).reshape(2, 4)
        return Point(Fr.from_limbs(l[0]).v, Fr.from_limbs(l[1]).v)
    @property
    def limbs(self): return point_limbs((self.x, self.y))
    def is_valid(self):
        """on the curve and [l]P == O (status 0 of bjj_validate_batch)"""
        return int(bjj_validate_batch([self])[0]) == 0
    def __add__(self, o): return bjj_add_batch([self], [o])[0]
    def __neg__(self): return Point(-self.x, self.y)
    def __sub__(self, o): return self + (-o)
    def __mul__(self, k): return bjj_mul_batch([self], [k if isinstance(k, Fr) else Fr(k)])[0]
    def __eq__(self, o): return isinstance(o, Point) and (self.x, self.y) == (o.x, o.y)
    def __hash__(self): return hash((self.x, self.y))
    def __repr__(self): return f"Point({self.x}, {self.y})"


def mul_base(ks, engine=None):
    """[[k] B8 for k in ks]: bjj_mul_batch on the tiled base point (no fixed-base table)"""
    K = _scalar_array(ks)
    return bjj_mul_batch(np.tile(point_limbs(B8), (K.shape[0], 1, 1)), K, engine=engine)
