"""TEST INFRASTRUCTURE - the integer model, the known answers and the inputs of the Baby Jubjub and EdDSA-Poseidon tests
(tests/test_babyjub_model.py, tests/test_hostsim_babyjub.py and tests/test_babyjub_abi.py on the CPU, tests/test_gpu_babyjub.py and
tests/test_gpu_eddsa.py on the GPU).

The model is written independently of bn_amd/babyjub.py and bn_amd/eddsa.py: the affine formulas with Fermat inverses, a right-to-left
scalar multiplication (the package goes left to right), its own Poseidon through tests/poseidon_cases.py with the width-6 round number set
here.  The expected bytes of a value are tests/fr_cases.py rows(): the Montgomery image, unique because every result is canonical."""
import functools

import numpy as np

import fr_cases as FC
import poseidon_cases as PC

PC.PARTIAL.setdefault(6, 60)              # circomlib's R_P at width 6 (poseidon_cases.py holds the four public widths)

R = FC.R
A_COEFF, D_COEFF = 168700, 168696
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ORDER = 21888242871839275222246405745257275088614511777268538073601725287587578984328
O = (0, 1)
G = (995203441582195749578291179787384436505546430278305826713579947235728471134, 5472060717959818805561601436314318772137091100104008585924551046643952123905)
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553, 16950150798460657717958625567821834550301663161624707787222815936182638968203)

# ---- known answers (the issue that introduced the family: iden3's Poseidon5 values and circomlibjs' published signature)
KNOWN_POSEIDON5 = {
    (1, 2, 0, 0, 0): 1018317224307729531995786483840663576608797660851238720571059489595066344487,
    (3, 4, 0, 0, 0): 5811595552068139067952687508729883632420015185677766880877743348592482390548,
}
KAT_A = (13277427435165878497778222415993513565335242147425444199013288855685581939618, 13622229784656158136036771217484571176836296686641868549125388198837476602820)
KAT_R8 = (11384336176656855268977457483345535180380036354188103142384839473266348197733, 15383486972088797283337779941324724402501462225528836549661220478783371668959)
KAT_S = 1672775540645840396591609181675628451599263765380031905495115170613215233181
KAT_M = 42649378395939397566720                  # the bytes 00 01 .. 09 00 00, little endian

ST_OK, ST_RANGE, ST_CURVE, ST_ORDER, ST_EQUATION = 0, 1, 4, 5, 6


def inv(v):
    return pow(v % R, -1, R)


def on_curve(p):
    x, y = p
    return (A_COEFF * x * x + y * y) % R == (1 + D_COEFF * x * x * y * y) % R


def add(p, q):
    x1, y1 = p; x2, y2 = q
    t = D_COEFF * x1 % R * x2 % R * y1 % R * y2 % R
    i = inv((1 + t) * (1 - t))                       # one inverse for both denominators; never zero on the curve: the law is complete
    return ((x1 * y2 + y1 * x2) % R * (1 - t) % R * i % R, (y1 * y2 - A_COEFF * x1 * x2) % R * (1 + t) % R * i % R)


def neg(p):
    return ((R - p[0]) % R, p[1])


_DOUBLINGS = {}            # point -> [p, 2p, 4p, ..]: the many multiples of B8 and G the cases need share their doublings


def mul(p, k):
    """[k]p, right to left"""
    runs = _DOUBLINGS.setdefault(p, [p]) if p in (B8, G) else [p]
    acc, i = O, 0
    while k:
        if i == len(runs):
            runs.append(add(runs[-1], runs[-1]))
        if k & 1:
            acc = add(acc, runs[i])
        k >>= 1; i += 1
    return acc


def sqrt(v):
    """a square root mod r (Tonelli-Shanks: r - 1 = 2^28 m), None for a non-residue"""
    v %= R
    if v == 0:
        return 0
    if pow(v, (R - 1) // 2, R) != 1:
        return None
    s, m = 28, (R - 1) >> 28
    z = 5                                          # 5 is a non-residue mod r
    c, t, x = pow(z, m, R), pow(v, m, R), pow(v, (m + 1) // 2, R)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u = u * u % R; i += 1
        b = pow(c, 1 << (s - i - 1), R)
        x, c = x * b % R, b * b % R
        t, s = t * c % R, i
    return x


def poseidon5(inputs):
    assert len(inputs) == 5
    return PC.permute([0] + [v % R for v in inputs])[0]


def challenge(a, r8, m):
    return poseidon5([r8[0], r8[1], a[0], a[1], m])


def validate_status(x, y):
    """of two 256-bit integers as the words of a record hold them"""
    if x >= R or y >= R:
        return ST_RANGE
    if not on_curve((x, y)):
        return ST_CURVE
    return ST_OK if mul((x, y), L) == O else ST_ORDER


def verify_status(a, r8, s, m):
    """a, r8: pairs of 256-bit integers, s and m 256-bit integers, as the words hold them"""
    if any(v >= R for v in tuple(a) + tuple(r8) + (s, m)) or s >= L:
        return ST_RANGE
    if not (on_curve(r8) and on_curve(a)):
        return ST_CURVE
    return ST_OK if mul(B8, s) == add(r8, mul(a, 8 * challenge(a, r8, m))) else ST_EQUATION


def sign(secret, m, rho):
    """(A, R8, S) for the integer secret and nonce"""
    a, r8 = mul(B8, secret), mul(B8, rho % L)
    return a, r8, (rho + 8 * challenge(a, r8, m) * secret) % L


# ---- edge points
@functools.lru_cache(maxsize=None)
def small_order_points():
    """{name: point}: O, the point of order 2, the two of order 4, one of order 8"""
    ra = sqrt(A_COEFF)
    assert ra is not None and sqrt(D_COEFF) is None
    o4 = (inv(ra), 0)
    o8 = mul(G, L)
    assert mul(o8, 4) == (0, R - 1) and mul(o8, 8) == O
    return {"O": O, "order2": (0, R - 1), "order4": o4, "order4neg": neg(o4), "order8": o8}


@functools.lru_cache(maxsize=None)
def edge_points():
    """[(name, point)]: every point of the curve the issue names"""
    sm = small_order_points()
    P = mul(B8, 0x123456789abcdef)
    out = list(sm.items()) + [("G", G), ("B8", B8), ("P", P), ("negP", neg(P))]
    out += [("B8+" + n, add(B8, p)) for n, p in sm.items() if n != "O"]
    return out


OFF_CURVE = (B8[0], (B8[1] + 1) % R)
RAW_OUT_OF_RANGE = [(R, 1), (0, R), (R + 1, B8[1]), (B8[0], (1 << 256) - 1), ((1 << 256) - 1, (1 << 256) - 1)]

# ---- edge scalars: small ones, around l and 8 l, the top of the range, single bits at the seams of the 4-bit windows of [k]P and of the 1- and 2-bit
# joint windows, long zero runs.  8 l is ABOVE r (the curve has r + 1 + 2^127.6.. points), so as an Fr it is only its residue 8 l - r; the chain itself
# takes it whole (test_hostsim_babyjub.py), and on the GPU [8 l]P is [8]([l]P)
EDGE_SCALARS = [0, 1, 2, 3, 4, 15, 16, L - 1, L, L + 1, ORDER % R, R - 1, 1 << 253,
                1 << 3, 1 << 4, 1 << 127, 1 << 128, 1 << 251, 1 << 252, (1 << 252) + 1, (1 << 253) + (1 << 4), (1 << 200) + 1, 0xf << 100, (1 << 253) - 1]
assert ORDER == 8 * L and R < ORDER < 1 << 254 and all(0 <= k < R for k in EDGE_SCALARS)


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


def validate_cases():
    """(points as raw integer pairs, expected statuses)"""
    pts = [p for _, p in edge_points()] + [OFF_CURVE] + RAW_OUT_OF_RANGE
    return pts, [validate_status(*p) for p in pts]


def curve_points(n, seed):
    """n points of the curve: the edge points first, then multiples of G (full order) and of B8"""
    rng = np.random.default_rng(seed)
    out = [p for _, p in edge_points()]
    while len(out) < n:
        out.append(mul(G if len(out) % 2 else B8, FC.rand(rng)))
    return out[:n]


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    return [EDGE_SCALARS[i] if i < len(EDGE_SCALARS) else FC.rand(rng) for i in range(n)]


@functools.lru_cache(maxsize=None)
def signatures(n, seed):
    """n valid signatures as (A, R8, S, M) from the model: msg = 0 and r - 1, a nonce that makes S = l - 1 and one that makes S = 0 among them"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        secret = FC.rand(rng) % L or 1
        m = 0 if i == 0 else R - 1 if i == 1 else FC.rand(rng)
        rho = FC.rand(rng) % L
        a, r8, s = sign(secret, m, rho)
        if i in (2, 3):                              # S = rho + 8 hm s with hm a hash of R8 = [rho]B8: only the secret 0 (A = O) lets a nonce fix S
            a, r8, s = sign(0, m, L - 1 if i == 2 else 0)
            assert s == (L - 1 if i == 2 else 0)
        out.append((a, r8, s, m))
    return tuple(out)


def signature_arrays(sigs):
    """[(A, R8, S, M)] of raw integers -> the four arrays of the C ABI"""
    return (point_rows([s[0] for s in sigs]), point_rows([s[1] for s in sigs]), raw_rows([s[2] for s in sigs]), raw_rows([s[3] for s in sigs]))


@functools.lru_cache(maxsize=None)
def failing_rows():
    """[(name, (A, R8, S, M), status)]: one row of each class the issue lists"""
    secret, m, rho = 0x1f2e3d4c5b6a79881726354453627180, 123456789, 0x0123456789abcdef0123456789abcdef
    a, r8, s = sign(secret, m, rho)
    assert verify_status(a, r8, s, m) == ST_OK
    rows = [("valid", (a, r8, s, m)), ("wrong message", (a, r8, s, m + 1)), ("-A", (neg(a), r8, s, m)), ("S + l", (a, r8, s + L, m)),
            ("S = l", (a, mul(B8, 0), L, m)), ("a coordinate at r", ((R, a[1]), r8, s, m)), ("msg at r", (a, r8, s, R)), ("R8 off the curve", (a, OFF_CURVE, s, m)),
            ("A off the curve", (OFF_CURVE, r8, s, m)), ("range and curve", (OFF_CURVE, (r8[0], R + 5), s, m)),
            ("A = O", (O, mul(B8, s), s, m)), ("A of order 2", ((0, R - 1), mul(B8, s), s, m)), ("A of order 8", (small_order_points()["order8"], mul(B8, s), s, m))]
    out = [(name, row, verify_status(*row)) for name, row in rows]
    want = {"valid": 0, "wrong message": 6, "-A": 6, "S + l": 1, "S = l": 1, "a coordinate at r": 1, "msg at r": 1, "R8 off the curve": 4, "A off the curve": 4,
            "range and curve": 1, "A = O": 0, "A of order 2": 0, "A of order 8": 0}
    assert {n: st for n, _, st in out} == want
    return tuple(out)
