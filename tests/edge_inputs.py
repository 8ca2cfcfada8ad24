"""TEST INFRASTRUCTURE - edge inputs for the group kernels (G1/G2 mul, group addition, Gt::pow, the wire decoders) and the Fq12 tower.

Plain Python on oracle/bn_model.py and the oracle's limb format (numpy uint64 Montgomery limbs, the reference's #[repr(C)] layouts).
Four families:
  * edge REPRESENTATIONS: the same group element as (X z^2, Y z^3, Z z) for z at the edges of Fq / Fq2 (rescale_g1 / rescale_g2);
  * edge POINTS: the G1 points with the smallest and largest x, k G2 for k in {1, r - 1, q mod r};
  * crafted SCALARS that drive the GLV split of G1 mul (curve.hpp glv_decompose) and the GLS split of G2 mul and Gt::pow
    (gls_decompose) to their largest parts and through their sign patterns, built from the lattice bases that
    tools/gen_device_constants.py wrote into bn_amd/csrc/bn254_constants.hpp;
  * edge Fq12 ELEMENTS (edge_fq12) with their images in the cyclotomic subgroup and in the order-r subgroup: coefficients 0, q - 1 and
    equal ones, subfield elements, single slots - what the tower, the final exponentiation and the Gt operations are fed.
"""
import pathlib
import re

import numpy as np

import bn_model as M
from bn_oracle import FQ, FR

Q, R = M.Q, M.R_ORD
HEADER = pathlib.Path(__file__).resolve().parents[1] / "bn_amd" / "csrc" / "bn254_constants.hpp"


# ---------------------------------------------------------------------------------------------- constants of the device's splits
def _words(name):
    """the 32-bit words of `uint32_t NAME[...] = {...};` in bn254_constants.hpp, flattened in declaration order"""
    m = re.search(r"uint32_t %s(?:\[\d+\])+ = \{(.*?)\};" % name, HEADER.read_text(), re.S)
    return [int(x, 16) for x in re.findall(r"0x[0-9a-f]+", m.group(1))]


def _int(words):
    return sum(w << (32 * i) for i, w in enumerate(words))


GLV_LAMBDA = _int(_words("GLV_LAMBDA"))                # the eigenvalue of phi(x, y) = (beta x, y) on G1
GLV_A1, GLV_A2 = _int(_words("GLV_A1")), _int(_words("GLV_A2"))
GLV_B1, GLV_B2 = -_int(_words("GLV_B1N")), _int(_words("GLV_B2"))
GLV_G1, GLV_G2 = _int(_words("GLV_G1")), _int(_words("GLV_G2"))   # floor(2^256 b2 / r), floor(2^256 |b1| / r)
GLS_LAMBDA = Q % R                                     # the eigenvalue of psi (the reference's mul_by_q) on G2 and of pi on Gt
_gw = _words("GLS_G")
GLS_G = [_int(_gw[8 * j:8 * j + 8]) for j in range(4)]           # |row 0 of the inverse basis| * 2^288
GLS_GNEG = [int(x) for x in re.search(r"GLS_GNEG\[4\] = \{(.*?)\}", HEADER.read_text()).group(1).split(",")]
_bw = _words("GLS_B")
_M96 = 1 << 96
GLS_B = [[(lambda v: v - _M96 if v >> 95 else v)(_int(_bw[12 * j + 3 * i:12 * j + 3 * i + 3])) for i in range(4)] for j in range(4)]
GLV_WINDOWS, GLS_WINDOWS = 33, 18                      # curve.hpp

assert (GLV_LAMBDA ** 2 + GLV_LAMBDA + 1) % R == 0 and GLV_A1 * GLV_B2 - GLV_A2 * GLV_B1 == R
assert all(sum(b * pow(GLS_LAMBDA, i, R) for i, b in enumerate(row)) % R == 0 for row in GLS_B)


def glv_split(k):
    """glv_decompose (curve.hpp) in integers, the model tools/gen_device_constants.py asserts: (|k1|, neg1, |k2|, neg2)"""
    c1, c2 = (k * GLV_G1) >> 256, (k * GLV_G2) >> 256
    m = 1 << 192
    k1 = (k - c1 * GLV_A1 - c2 * GLV_A2) % m
    k2 = (c1 * -GLV_B1 - c2 * GLV_B2) % m
    s1, s2 = k1 >> 191, k2 >> 191
    return (m - k1 if s1 else k1), s1, (m - k2 if s2 else k2), s2


def gls_split(k):
    """gls_decompose (curve.hpp) in integers: [(|k_i|, neg_i)] for i = 0..3"""
    c = [((k * g) >> 288) % _M96 for g in GLS_G]
    out = []
    for i in range(4):
        v = k % _M96 if i == 0 else 0
        for j in range(4):
            t = c[j] * (GLS_B[j][i] % _M96) % _M96
            v = (v + t) % _M96 if GLS_GNEG[j] else (v - t) % _M96
        out.append((_M96 - v if v >> 95 else v, v >> 95))
    return out


def booth_digits(mag, windows):
    """radix-16 Booth digits of a magnitude, least significant window first (curve.hpp booth_digit)"""
    return [-8 * (mag >> (4 * i + 3) & 1) + 4 * (mag >> (4 * i + 2) & 1) + 2 * (mag >> (4 * i + 1) & 1) + (mag >> (4 * i) & 1)
            + (mag >> (4 * i - 1) & 1 if i else 0) for i in range(windows)]


def top_window(mag, windows):
    """index of the highest non-zero Booth window, -1 for 0"""
    d = booth_digits(mag, windows)
    return max((i for i in range(windows) if d[i]), default=-1)


# ---------------------------------------------------------------------------------------------- edge representations
# The 9 x 29-bit internal image of x (fe_from_u32x8: the reference's limbs x 2^256 times C_IN = 2^266 mod q in a Montgomery product of
# radix 2^261) is x 2^261 mod q.  So the Fq element whose internal image is a chosen m < q is m 2^-261 mod q:
#   FE_LIMBS_MAX: m = (2^232 - 1) + (q >> 232 - 1) 2^232 - limbs 0..7 all 2^29 - 1, the top limb one below q's;
#   FE_LIMBS_MIN: m = (q >> 232) 2^232 - limbs 0..7 all zero, the top limb equal to q's (m < q: q's low 232 bits are not zero).
# (a Montgomery product may leave m + q instead of m: both are < 2q and normalized; the value is what is pinned)
_TOP = Q >> 232
FE_LIMBS_MAX = ((1 << 232) - 1 + (_TOP - 1) * (1 << 232)) * pow(2, -261, Q) % Q
FE_LIMBS_MIN = (_TOP << 232) * pow(2, -261, Q) % Q
R_INV = pow(1 << 256, -1, Q)                          # its Montgomery image (the oracle's limbs) is 1

FQ_Z = [1, Q - 1, 2, (Q + 1) // 2, 1 << 29, 1 << 64, 1 << 128, 1 << 253, R_INV, FE_LIMBS_MAX, FE_LIMBS_MIN]
FQ2_Z = [(0, 1), (1, 0), (Q - 1, Q - 1), (0, Q - 1), (1, 1), (FE_LIMBS_MAX, 0), ((Q + 1) // 2, 0), (R_INV, R_INV)]


def fq(oracle, v):
    return oracle.fp_from_int(FQ, v % Q)


def fr(oracle, vals):
    return np.stack([oracle.fp_from_int(FR, v % R) for v in vals])


def g1_ints(oracle, p):
    return [oracle.fp_to_int(FQ, p[4 * i:4 * i + 4]) for i in range(3)]


def g2_ints(oracle, p):
    v = [oracle.fp_to_int(FQ, p[4 * i:4 * i + 4]) for i in range(6)]
    return [(v[0], v[1]), (v[2], v[3]), (v[4], v[5])]


def rescale_g1(oracle, p, z):
    """(X, Y, Z) -> (X z^2, Y z^3, Z z): the same G1 element (infinity stays infinity: Z z = 0)"""
    x, y, zz = g1_ints(oracle, p)
    z2 = z * z % Q
    return np.concatenate([fq(oracle, x * z2), fq(oracle, y * z2 * z), fq(oracle, zz * z)])


def rescale_g2(oracle, p, z):
    """(X, Y, Z) -> (X z^2, Y z^3, Z z) over Fq2, z = (c0, c1)"""
    x, y, zz = g2_ints(oracle, p)
    z2 = M.f2_sqr(z)
    return np.concatenate([fq(oracle, c) for c in (*M.f2_mul(x, z2), *M.f2_mul(y, M.f2_mul(z2, z)), *M.f2_mul(zz, z))])


def _fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)                       # q = 3 mod 4
    return r if r * r % Q == a % Q else None


def edge_g1_affine():
    """[(x, y)]: the points of y^2 = x^3 + 3 with the smallest and the largest x that have a square x^3 + 3, each with y and q - y
    (G1 has cofactor 1: every curve point is in the group)"""
    out = []
    for xs in (range(0, 64), range(Q - 1, Q - 64, -1)):
        x = next(x for x in xs if _fq_sqrt(x ** 3 + 3) is not None)
        y = _fq_sqrt(x ** 3 + 3)
        out += [(x, y), (x, Q - y)]
    return out


def edge_g1_points(oracle):
    return [np.concatenate([fq(oracle, x), fq(oracle, y), fq(oracle, 1)]) for x, y in edge_g1_affine()]


G2_EDGE_SCALARS = [1, R - 1, GLS_LAMBDA]


def edge_g2_points(oracle):
    return [oracle.g2_mul(oracle.g2_one(), oracle.fp_from_int(FR, k)) for k in G2_EDGE_SCALARS]


# ---------------------------------------------------------------------------------------------- crafted scalars
def _pattern(nibble_hex, bits):
    """the hex pattern repeated to `bits` bits (whole nibbles)"""
    s = (nibble_hex * (bits // 4 // len(nibble_hex) + 1))[:bits // 4]
    return int(s, 16)


# 0x88..8: Booth digits -8, -7, ..., -7, +1; 0x77..7: +7 everywhere; 0x7878..78: -8, +8, -8, ... (every digit at the extreme)
_BOOTH_PATTERNS = ("8", "7", "78", "87", "f0", "0f")


def special_scalars(lam):
    return [lam, R - lam, lam + 1, lam - 1, (R - 1) // 2, (R + 1) // 2, lam * lam % R, pow(lam, 3, R), R - lam * lam % R,
            (1 << 253) + 1, (1 << 253) + 17, (1 << 253) - 1, 1, 2, R - 1, R - 2]


def _glv_domain_extremes():
    """k whose GLV split sits at the far edge of the reduction domain.  (k, 0) = a1' v1 + a2' v2 with a1' = k b2 / r, a2' = k |b1| / r;
    the device takes c_i = floor(k G_i / 2^256) with G_i rounded DOWN, so c_i is floor(a_i') or one less, and the parts are
    (k1, k2) = s v1 + t v2, s = a1' - c1, t = a2' - c2 in [0, 1 + k/2^256).  The largest s (t) is reached at the last k before
    c1 (c2) steps to the next integer: k = ceil(n 2^256 / G) - 1 while c = n - 1."""
    out = []
    for g, top in ((GLV_G2, -GLV_B1), (GLV_G1, GLV_B2)):
        for j in range(1, 48):
            n = top - j
            k = -(-(n << 256) // g) - 1
            if 0 < k < R:
                out.append(k)
    # s close to 0 and t close to 1 (the sign pattern k2 >= 0 needs s |b1| <= t b2), and t close to 0
    out += [-(-(m * R) // GLV_B2) for m in (1, 2, 3, 1 << 20)] + [-(-(n * R) // -GLV_B1) for n in (1, 2, 1 << 40, -GLV_B1 - 1)]
    return out


def glv_crafted():
    """crafted scalars for bn254_g1_mul_M: the domain's edges, Booth-pattern parts (k1, k2) in all four sign combinations
    mapped to k = k1 + k2 lambda mod r, and the eigenvalue's neighbourhood"""
    ks = _glv_domain_extremes()
    for p in _BOOTH_PATTERNS:
        for bits in (124, 126):
            m = _pattern(p, bits) & ((1 << 126) - 1)
            for s1 in (1, -1):
                for s2 in (1, -1):
                    ks.append((s1 * m + s2 * m * GLV_LAMBDA) % R)
            ks.append(m % R)
    ks += special_scalars(GLV_LAMBDA)
    return sorted({k % R for k in ks if k % R})


def _gls_domain_extremes():
    """k whose GLS split sits at an edge of its domain: for each row j of the inverse basis, the last k before c_j steps to the next
    integer (c_j one below its true floor: the largest remainder along B_j), over a spread of quotients"""
    out = []
    for j, g in enumerate(GLS_G):
        top = (R * g) >> 288
        for n in [top - i for i in range(1, 24)] + [top * f // 16 for f in range(1, 16)]:
            k = -(-(n << 288) // g) - 1
            if 0 < k < R:
                out += [k, k + 1]
    return out


def gls_crafted():
    """crafted scalars for bn254_g2_mul_M and bn254_gt_pow_B: the domain's edges, Booth-pattern parts in all 16 sign combinations
    mapped to k = sum k_i lambda^i mod r, and the eigenvalue's powers"""
    ks = _gls_domain_extremes()
    lp = [pow(GLS_LAMBDA, i, R) for i in range(4)]
    for p in ("8", "7", "78"):
        m = _pattern(p, 64)
        for signs in range(16):
            ks.append(sum((-m if signs >> i & 1 else m) * lp[i] for i in range(4)) % R)
    ks += special_scalars(GLS_LAMBDA)
    return sorted({k % R for k in ks if k % R})


def crafted_gls_by_sign():
    """one crafted scalar per sign pattern (neg_0 .. neg_3) of the device's split that the crafted set reaches, the one with the
    largest part: a small set that still covers every pattern"""
    best = {}
    for k in gls_crafted():
        parts = gls_split(k)
        key = tuple(n for _, n in parts)
        mx = max(m for m, _ in parts)
        if key not in best or mx > best[key][0]:
            best[key] = (mx, k)
    return [k for _, k in best.values()]


# ---------------------------------------------------------------------------------------------- wire records at the limits
def _fq_cbrt(a):
    """a cube root of a mod q, or None (q - 1 = 3^2 t, 3 does not divide t: a^(3^-1 mod t) is a root up to a factor of order 9)"""
    t = (Q - 1) // 9
    x0 = pow(a, pow(3, -1, t), Q)
    z = next(z for z in range(2, 100) if pow(z, (Q - 1) // 3, Q) != 1)
    g = pow(z, t, Q)                                  # generates the 3-Sylow subgroup (order 9)
    return next((x0 * pow(g, e, Q) % Q for e in range(9) if pow(x0 * pow(g, e, Q), 3, Q) == a % Q), None)


def g1_points_with_y_one():
    """[(x, 1), (x, q - 1)] with x^3 + 3 = 1: the curve points whose y is 1 and q - 1"""
    x = _fq_cbrt(Q - 2)
    return [(x, 1), (x, Q - 1)]


def g1_record(x, y, tag=4):
    """65-byte G1 record with arbitrary 256-bit integers as coordinates"""
    return np.frombuffer(bytes([tag]) + x.to_bytes(32, "big") + y.to_bytes(32, "big"), np.uint8).copy()


def g2_record(x, y, tag=4):
    """129-byte G2 record with arbitrary 512-bit integers as coordinates (the reference packs an Fq2 as c1 q + c0)"""
    return np.frombuffer(bytes([tag]) + x.to_bytes(64, "big") + y.to_bytes(64, "big"), np.uint8).copy()


def fq2_packed(c):
    return c[1] * Q + c[0]


# ---------------------------------------------------------------------------------------------- edge Fq12 elements
# the coefficient pool of tests/test_hostsim.py's EDGE: 0 and q - 1, their neighbours, the middle, a single high bit, a full low 29-bit
# limb, the lowest bit of the top limb of the 9 x 29-bit form, and R mod q
FQ12_POOL = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, 1 << 253, (1 << 29) - 1, 1 << 232, M.MONT_R % Q]
GT_EDGE_SCALARS = [0, 1, 2, 15, 16, R - 1, (1 << 253) + 12345]
_FQ12_CACHE = {}


def edge_fq12_ints():
    """ordered {name: [12 integers]} - 64 NON-ZERO Fq12 elements, coefficients in the order oracle.fq12_from_ints takes (slots 0..5 are
    c0 = three Fq2, slots 6..11 are c1).  Equal coefficients make the signed Karatsuba differences of the tower vanish, 0 against q - 1
    drives them to either extreme, subfield elements and single slots leave most partial products zero.  (-1 is there twice: under its
    own name and as the first of the twelve single slots.)"""
    z, m = 0, Q - 1
    e = {"one": [1] + [z] * 11, "-1": [m] + [z] * 11, "all q-1": [m] * 12, "all 1": [1] * 12,
         "0,q-1 x6": [z, m] * 6, "q-1,0 x6": [m, z] * 6, "c0 only": [m] * 6 + [z] * 6, "c1 only": [z] * 6 + [m] * 6,
         "w": [z] * 6 + [1] + [z] * 5}
    for s in range(12):
        e["q-1 in slot %d" % s] = [m if i == s else z for i in range(12)]
    e["fq2 subfield"] = [m, Q - 2] + [z] * 10
    e["all (q-1)/2"] = [(Q - 1) // 2] * 12
    e["all 2^253"] = [1 << 253] * 12
    rng = np.random.default_rng(20260)
    while len(e) < 64:
        c = [FQ12_POOL[i] for i in rng.integers(0, len(FQ12_POOL), 12)]
        if any(c):
            e["pool draw %d" % (len(e) - 24)] = c
    return e


def edge_fq12(oracle):
    """ordered {name: (48,) uint64}: edge_fq12_ints() as the oracle's Montgomery limbs"""
    if "fq12" not in _FQ12_CACHE:
        _FQ12_CACHE["fq12"] = {k: oracle.fq12_from_ints(v) for k, v in edge_fq12_ints().items()}
    return _FQ12_CACHE["fq12"]


def edge_cyclotomic(oracle):
    """the easy part of the final exponentiation of every edge element, in order: elements of the cyclotomic subgroup, generally NOT of
    order r"""
    if "cyc" not in _FQ12_CACHE:
        _FQ12_CACHE["cyc"] = [oracle.fq12_final_exp_first_chunk(a) for a in edge_fq12(oracle).values()]
    return _FQ12_CACHE["cyc"]


def edge_gt(oracle):
    """the final exponentiation of every edge element, in order: elements whose order divides r"""
    if "gt" not in _FQ12_CACHE:
        _FQ12_CACHE["gt"] = [oracle.fq12_final_exponentiation(a) for a in edge_fq12(oracle).values()]
    return _FQ12_CACHE["gt"]


def edge_partners(n=64):
    """the index of the second operand for every edge element: a fixed seeded draw, never the element itself (a * b is not the square)"""
    idx = np.random.default_rng(20261).integers(0, n, n)
    return [int(j) if int(j) != i else (i + 1) % n for i, j in enumerate(idx)]


def oracle_is_cyclotomic(oracle, a):
    """a^(q^4 - q^2 + 1) == 1 as frob^4(a) * a == frob^2(a), computed with the oracle: what pairing.hpp gt_is_cyclotomic evaluates"""
    f2 = oracle.fq12_frobenius_map(a, 2)
    f4 = oracle.fq12_frobenius_map(f2, 2)
    return np.array_equal(oracle.fq12_mul(f4, a), f2)
