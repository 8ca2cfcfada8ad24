"""Baby Jubjub: the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over the scalar field Fr of BN254 (a = 168700, d = 168696) that circomlib,
iden3 and the Hermez-style rollups sign on - its constants, the group law in host integers, a small Point type, and the batch calls on the GPU
(bn_amd.bjj_validate_batch / bjj_add_batch / bjj_mul_batch).

    identity O = (0, 1);  -(x, y) = (-x, y);  order 8 l, l a 251-bit prime;  G of order 8 l, B8 = [8]G of order l
    (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2))

a is a square mod r and d is not, so the law is complete: no exceptional inputs, doubling is the same formula.  A point travels as two
consecutive Fr (x then y, Montgomery words, affine): (n, 2, 4) uint64 in numpy.  Nothing here is downloaded or pasted: the constants are the
integers below and tools/gen_babyjub_constants.py derives the device header from them.

Packed points (pack_batch / unpack_batch on the GPU, pack_host / unpack_host in host integers): 32 bytes, the canonical integer of y little
endian with bit 7 of the last byte set iff the canonical integer of x is above (r - 1) / 2 - circomlibjs' packPoint as its documentation
describes it, written from memory: NO packed test vector of circomlibjs has been checked.  Unpacking solves x^2 = (1 - y^2) / (a - d y^2)
(a square root in Fr, whose 2-adicity is 28) and takes the root with the sign asked for.  It does not check the subgroup (circomlib does not
either; is_valid / bjj_validate_batch do).  x == 0 is accepted with the sign bit clear and rejected (status 3) with it set: that is this
project's decision and may differ from circomlibjs."""
import numpy as np

from .api import R_MOD, Fr, _limbs, _mont, _scalar_array, bjj_validate_batch, bjj_add_batch, bjj_mul_batch, bjj_pack_batch, bjj_unpack_batch

A = 168700
D = 168696
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041            # the prime order of B8 (251 bits)
ORDER = 8 * L
IDENTITY = (0, 1)
G = (995203441582195749578291179787384436505546430278305826713579947235728471134, 5472060717959818805561601436314318772137091100104008585924551046643952123905)
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553, 16950150798460657717958625567821834550301663161624707787222815936182638968203)
STATUS = {0: "valid", 1: "a coordinate or scalar is out of range", 4: "not on the curve", 5: "on the curve but not of an order dividing l", 6: "the signature equation fails"}

# the statuses of the packed forms (unpack_batch, eddsa.verify_packed_status_batch): those of STATUS, with 4 read as "no point has this y", and 3
PACK_STATUS = {0: "valid", 1: "y or a scalar is out of range", 3: "x is zero and the sign bit is set: not the canonical encoding", 4: "no point of the curve has this y",
               6: STATUS[6]}


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


def sqrt_host(v):
    """the square root of v mod r that is not above (r - 1) / 2, None for a non-residue: Tonelli-Shanks in host integers (r - 1 = 2^28 t)"""
    v %= R_MOD
    if v == 0:
        return 0
    if pow(v, (R_MOD - 1) // 2, R_MOD) != 1:
        return None
    s, t = 28, (R_MOD - 1) >> 28
    c, b, x = pow(5, t, R_MOD), pow(v, t, R_MOD), pow(v, (t + 1) // 2, R_MOD)
    while b != 1:
        i, u = 0, b
        while u != 1:
            u, i = u * u % R_MOD, i + 1
        g = pow(c, 1 << (s - i - 1), R_MOD)
        x, c, s = x * g % R_MOD, g * g % R_MOD, i
        b = b * c % R_MOD
    return min(x, R_MOD - x)


def pack_host(p):
    """(x, y) -> 32 bytes, in host integers; no validation"""
    x, y = (p.x, p.y) if isinstance(p, Point) else p
    return (y | (1 << 255 if x > (R_MOD - 1) // 2 else 0)).to_bytes(32, "little")


def unpack_host(b):
    """32 bytes -> ((x, y), status) in host integers, in the order of the device's checks; a rejected record gives IDENTITY"""
    b = bytes(b)
    if len(b) != 32:
        raise ValueError("a packed point is 32 bytes")
    v = int.from_bytes(b, "little")
    sign, y = v >> 255, v & ((1 << 255) - 1)
    if y >= R_MOD:
        return IDENTITY, 1
    x = sqrt_host((1 - y * y) * pow(A - D * y * y, -1, R_MOD))
    if x is None:
        return IDENTITY, 4
    if x == 0 and sign:
        return IDENTITY, 3
    return ((R_MOD - x if sign else x), y), 0


def pack_batch(points, engine=None):
    """[32 bytes per point] on the GPU (bn_amd.bjj_pack_batch)"""
    return bjj_pack_batch(points, engine=engine)


def unpack_batch(records, engine=None):
    """(list of Point, (n,) int32 status) on the GPU (bn_amd.bjj_unpack_batch): 0, or 1 / 4 / 3 and the identity"""
    return bjj_unpack_batch(records, engine=engine)


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
    def pack(self):
        """the 32-byte record (on the GPU)"""
        return bjj_pack_batch([self])[0]
    @staticmethod
    def unpack(b):
        """the point of a 32-byte record (on the GPU); ValueError with the status' text for a rejected one"""
        pts, st = bjj_unpack_batch([b])
        if int(st[0]):
            raise ValueError(f"not a packed point: {PACK_STATUS[int(st[0])]}")
        return pts[0]
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
