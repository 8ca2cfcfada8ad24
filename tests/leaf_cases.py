"""TEST INFRASTRUCTURE - the case sets of the leaf tests and an integer model of every leaf, in plain Python: shared by the CPU test
(tests/test_hostsim_leaf.py, the bounds-checked twins) and the GPU test (tests/test_gpu_leaf.py, the inline-asm leaves), seeded, so both see the
same cases.  Nothing here calls compiled code, and the model shares no code with the twins: it knows a leaf only by what fe.hpp PROMISES of it.

A case is (name, operands, bounds, flag): the operands as lists of 9 or 18 limbs (uint32 values), the claimed bounds (lb, vb, signed) per Fe and
(lb, wb, 0) per FeW, and the leaf's boolean (fe_wred's `neg`, the fused reductions' `neg2`).  Every case lies inside the leaf's BN_REQUIRE contract;
the twin aborts otherwise, so a green CPU run proves it.

Classes per leaf:  hot limb (one limb of each factor at the largest value the contract allows, everything else zero - every (i, j) of every
operand pair; for the reductions every limb of every operand, both signs),  ceilings (limbs 0..7 at lb (2^29 - 1), the value just below vb q, at the
extreme points of the contract, every sign pattern where operands are signed),  degenerate (zero, q - 1, one operand zero),  256 random."""
import random

import numpy as np

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MASK29 = (1 << 29) - 1
R261 = 1 << 261
RINV = pow(R261, -1, Q)


# ---------------------------------------------------------------------------------------------------------------- limbs
def at_bound(lb, vb):
    """nine limbs with limbs 0..7 at lb (2^29 - 1) and the value just below vb q"""
    low = sum((lb * MASK29) << (29 * i) for i in range(8))
    top = (vb * Q - low) >> 232
    assert top >= 0
    return np.array([lb * MASK29] * 8 + [top], np.uint32)


def sdiff(x, y):
    """limb-wise difference of two normalized nine-limb values: every limb an int32 of magnitude below 2^29 (fe_sdiff)"""
    return ((x.astype(np.int64) - y.astype(np.int64)) & 0xffffffff).astype(np.uint32)


def wide_raw(lb, wb, sign):
    """18 limbs at the claimed bounds: limbs 0..16 at lb (2^29 - 1), the top limb at +- wb q^2 / 2^493"""
    top = sign * ((wb * Q * Q) >> (29 * 17))
    return np.array([lb * MASK29] * 17 + [top & 0xffffffff], np.uint32)


# (xi, sub, bounds of n, bounds of x) of the combinations the tower forms; the value bounds are those of the cross term of f12_mul_src, whose
# operands are carry-propagated sums below 6q:  v_i <= 6*6 + 6*9 = 90 q^2,  m_ij <= 72,  X_ij = m_ij + v_i + v_j <= 252
COMBOS = [("c0 = v0 + xi X12", True, (1, 90), (3, 252)), ("c1 = X01 + xi v2", True, (3, 252), (1, 90)), ("c2 = X02 + v1", False, (4, 342), (1, 0))]
D_BOUND = (2, 6)                # aa + bb, each in standard form


def norm9(v):
    assert 0 <= v < (1 << 264)
    return [(v >> (29 * i)) & MASK29 for i in range(8)] + [v >> 232]


def norm18(v):
    """a signed integer in the wide form: limbs 0..16 in [0, 2^29), the sign in the top limb"""
    top = v >> (29 * 17)
    assert -(1 << 31) <= top < (1 << 31)
    return [(v >> (29 * i)) & MASK29 for i in range(17)] + [top & 0xffffffff]


def neg_limbs(l):
    return [(-x) & 0xffffffff for x in l]


def s32(x):
    return x - (1 << 32) if x >> 31 else x


def value(l, signed=False, top_signed=False):
    """sum l[i] 2^(29 i); `signed`: every limb an int32; `top_signed`: only the top one"""
    n = len(l)
    return sum((s32(int(x)) if (signed or (top_signed and i == n - 1)) else int(x)) << (29 * i) for i, x in enumerate(l))


def _ints(a):
    return [int(x) for x in a]


ZERO9, ZERO18 = [0] * 9, [0] * 18
QM1 = norm9(Q - 1)


# ---------------------------------------------------------------------------------------------------------------- the leaves
def _lc(cs, wide=False, sign2=False, flag=False):
    return {"family": "lc", "C": tuple(cs) + (0,) * (4 - len(cs)), "WIDE": wide, "SIGN2": sign2, "flag": flag}


# (name, operand kinds, output limbs, description) in the order - the ids - of tests/leafprobe/leaf_list.hpp
LEAVES = [
    ("fe_mul", "ff", 9, {"family": "mont", "bound": 2}),
    ("fe_sqr", "f", 9, {"family": "sqr", "bound": 2}),
    ("fe_mul2", "ffff", 9, {"family": "mont"}),
    ("fe_mul2s", "ffff", 9, {"family": "mont", "signed": True, "bound": 2}),
    ("fe_mul6", "f" * 12, 9, {"family": "mont"}),
    ("fe_mul5", "f" * 10, 9, {"family": "mont"}),
    ("fe_wmul2", "ffff", 18, {"family": "wide"}),
    ("fe_wmul2s", "ffff", 18, {"family": "wide", "signed": True}),
    ("fe_wred_ff", "wwwf", 9, {"family": "wred", "xi": False, "sub": False}),
    ("fe_wred_ft", "wwwf", 9, {"family": "wred", "xi": False, "sub": True}),
    ("fe_wred_tf", "wwwf", 9, {"family": "wred", "xi": True, "sub": False}),
    ("fe_wred_tt", "wwwf", 9, {"family": "wred", "xi": True, "sub": True}),
    ("lc3_1_1_0", "fff", 9, _lc((1, 1, 0))),
    ("lc3_1_m1_0", "fff", 9, _lc((1, -1, 0))),
    ("lc3_1_m1_m2", "fff", 9, _lc((1, -1, -2))),
    ("lc3_1_0_0", "fff", 9, _lc((1, 0, 0))),
    ("lc3_0_0_0", "fff", 9, _lc((0, 0, 0))),
    ("lc3_m1_0_0", "fff", 9, _lc((-1, 0, 0))),
    ("lc3_9_0_0", "fff", 9, _lc((9, 0, 0))),
    ("lc3_4_0_0", "fff", 9, _lc((4, 0, 0))),
    ("lc3_9_m1_1", "fff", 9, _lc((9, -1, 1))),
    ("lc3_9_1_1", "fff", 9, _lc((9, 1, 1))),
    ("lc3_1_m3_0", "fff", 9, _lc((1, -3, 0))),
    ("lc3_27_3_0", "fff", 9, _lc((27, 3, 0))),
    ("lc3_27_m3_0", "fff", 9, _lc((27, -3, 0))),
    ("lc3_9_m1_0", "fff", 9, _lc((9, -1, 0))),
    ("lc3_54_m6_2", "fff", 9, _lc((54, -6, 2))),
    ("lc3c_m1_1_0_s", "fff", 9, _lc((-1, 1, 0), sign2=True, flag=True)),
    ("lc3c_9_1_1_s", "fff", 9, _lc((9, 1, 1), sign2=True, flag=True)),
    ("lc4c_9_1_1_0_s", "ffff", 9, _lc((9, 1, 1, 0), sign2=True, flag=True)),
    ("lc4c_27_3_3_2_s", "ffff", 9, _lc((27, 3, 3, 2), sign2=True, flag=True)),
    ("lc4c_27_m3_1_1", "ffff", 9, _lc((27, -3, 1, 1), flag=True)),
    ("lc4c_27_3_3_1", "ffff", 9, _lc((27, 3, 3, 1), flag=True)),
    ("lc4c_m27_3_3_m2", "ffff", 9, _lc((-27, 3, 3, -2), flag=True)),
    ("lc4c_m27_m3_3_m2", "ffff", 9, _lc((-27, -3, 3, -2), flag=True)),
    ("lc4w_9_m1_1_m1", "ffff", 9, _lc((9, -1, 1, -1), wide=True, flag=True)),
    ("lc4w_9_1_1_m1", "ffff", 9, _lc((9, 1, 1, -1), wide=True, flag=True)),
    ("lc4w_1_m1_0_0", "ffff", 9, _lc((1, -1, 0, 0), wide=True, flag=True)),
    ("lc3w_9_m1_3", "fff", 9, {"family": "lc3w", "C": (9, -1, 3)}),
    ("lc3w_1_m1_m1", "fff", 9, {"family": "lc3w", "C": (1, -1, -1)}),
]
LEAF_ID = {l[0]: i for i, l in enumerate(LEAVES)}


def lc_branch(d):
    """(NWIDE, a narrow sum exists, which operands are narrow) of a fused reduction: the selection rules of fe_lc4_core, restated"""
    C = d["C"]
    K = [(not d["WIDE"]) and c != 0 and abs(c) <= 2 and not (d["SIGN2"] and i == 1) for i, c in enumerate(C)]
    lone = sum(K) == 1
    N = [k and not (lone and c != 1) for k, c in zip(K, C)]
    return sum(1 for c, n in zip(C, N) if c != 0 and not n), any(N), N


# ---------------------------------------------------------------------------------------------------------------- operand makers
def hot(i, lb, vb, sign=1, spare=0):
    """nine limbs, all zero but limb i at the largest magnitude (lb, vb) allows"""
    l = [0] * 9
    l[i] = lb * MASK29 if i < 8 else ((vb * Q) >> 232) - spare
    return l if sign > 0 else neg_limbs(l)


def rand_lazy(rng, lb, vb):
    """random limbs within (lb, vb): limbs 0..7 anywhere up to lb (2^29 - 1), the top limb anywhere the value bound leaves"""
    l = [rng.randrange(lb * MASK29 + 1) for _ in range(8)]
    low = sum(x << (29 * i) for i, x in enumerate(l))
    return l + [rng.randrange(((vb * Q - low) >> 232) + 1)]


def rand_sdiff(rng, vb):
    """the limb-wise difference of two random normalized values below vb q: either sign, mixed limb signs"""
    x, y = norm9(rng.randrange(vb * Q)), norm9(rng.randrange(vb * Q))
    return [(a - b) & 0xffffffff for a, b in zip(x, y)]


def _sg(l):
    return 1 if any(x >> 31 for x in l) else 0


def _b(lb, vb, l):
    return (lb, vb, _sg(l))


# ---------------------------------------------------------------------------------------------------------------- Montgomery and wide products
# the contract points: per operand pair ((lb, vb) of the first factor, (lb, vb) of the second)
MUL_LBS = [(1, 6), (6, 1), (2, 3), (3, 2)]
MUL_VBS = [(13, 13), (1, 169), (169, 1)]
POINTS = {
    # la lu + lc lv = 6 and sum of the value products = 338 (the < 3q regime), and one point of the < 2q regime (169)
    "fe_mul2": [[((1, 13), (3, 13)), ((3, 13), (1, 13))], [((2, 1), (2, 169)), ((1, 169), (2, 1))], [((5, 337), (1, 1)), ((1, 1), (1, 1))],
                [((1, 2), (1, 1)), ((1, 2), (5, 168))], [((2, 13), (3, 13)), ((6, 1), (0, 1))], [((1, 12), (3, 12)), ((3, 5), (1, 5))]],
    # limb sum 2 (all limbs below 2^29 in magnitude) and the value bound 169
    "fe_mul2s": [[((1, 9), (1, 9)), ((1, 8), (1, 11))], [((1, 1), (1, 168)), ((1, 1), (1, 1))]],
    # every operand normalized; 338 = 169 + 156 + 1 + 1 + 1 + 10, and the same split another way round; 169 = the < 2q regime
    "fe_mul6": [[((1, 13), (1, 13)), ((1, 12), (1, 13)), ((1, 1), (1, 1)), ((1, 1), (1, 1)), ((1, 1), (1, 1)), ((1, 1), (1, 10))],
                [((1, 1), (1, 1)), ((1, 10), (1, 1)), ((1, 7), (1, 8)), ((1, 8), (1, 7)), ((1, 2), (1, 28)), ((1, 159), (1, 1))],
                [((1, 4), (1, 7)), ((1, 7), (1, 4)), ((1, 4), (1, 7)), ((1, 7), (1, 4)), ((1, 4), (1, 7)), ((1, 29), (1, 1))]],
    "fe_mul5": [[((1, 13), (1, 13)), ((1, 12), (1, 13)), ((1, 1), (1, 1)), ((1, 1), (1, 1)), ((1, 1), (1, 11))],
                [((1, 1), (1, 1)), ((1, 11), (1, 1)), ((1, 7), (1, 8)), ((1, 8), (1, 7)), ((1, 214), (1, 1))],
                [((1, 4), (1, 7)), ((1, 7), (1, 4)), ((1, 4), (1, 7)), ((1, 7), (1, 4)), ((1, 57), (1, 1))]],
    # column bound 6, value bound 1024
    "fe_wmul2": [[((1, 16), (3, 32)), ((3, 32), (1, 16))], [((6, 1023), (1, 1)), ((0, 1), (1, 1))], [((2, 6), (1, 3)), ((2, 6), (2, 9))], [((1, 1), (1, 1)), ((5, 31), (1, 33))]],
    "fe_wmul2s": [[((1, 32), (1, 16)), ((1, 16), (1, 32))], [((1, 2), (1, 511)), ((1, 1), (1, 2))]],          # (a signed top limb holds up to 675 q)
}
POINTS["fe_mul"] = [[((la, va), (lu, vu))] for la, lu in MUL_LBS for va, vu in MUL_VBS]
POINTS["fe_sqr"] = [[((2, 13), (2, 13))], [((1, 13), (1, 13))], [((2, 1), (2, 1))]]


def _point_ok(name, pt):
    """the leaf's BN_REQUIRE lines, restated"""
    ls, vs = sum(a[0] * u[0] for a, u in pt), sum(a[1] * u[1] for a, u in pt)
    if name in ("fe_mul", "fe_sqr"):
        return ls <= 6 and vs <= 169
    if name == "fe_mul2":
        return ls <= 6 and vs <= 338
    if name == "fe_mul2s":
        return ls <= 2 and vs <= 169
    if name in ("fe_mul6", "fe_mul5"):
        return all(a[0] == 1 and u[0] == 1 for a, u in pt) and vs <= 338
    if name == "fe_wmul2":
        return ls <= 6 and vs <= 1024
    return ls <= 2 and vs <= 1024


def _flat(pt):
    return [b for pair in pt for b in pair]


def product_cases(name):
    d = LEAVES[LEAF_ID[name]][3]
    signed = d.get("signed", False)
    sqr = d["family"] == "sqr"
    pts = POINTS[name]
    assert all(_point_ok(name, pt) for pt in pts), name
    rng = random.Random(1000 + LEAF_ID[name])
    npairs = len(pts[0])
    out = []

    def emit(cname, ops, bs):
        if sqr:
            ops, bs = ops[:1], bs[:1]
        out.append((cname, ops, [_b(lb, vb, l) if signed else (lb, vb, 0) for (lb, vb), l in zip(bs, ops)], 0))

    # ---- hot limb: at the first contract point (for fe_mul at two opposite ones)
    for pi, pt in enumerate(pts[:1] if name != "fe_mul" else [pts[6], pts[4]]):
        bs = _flat(pt)
        for p in range(npairs):
            for i in range(9):
                for j in range(i if sqr else 0, 9):
                    for sa, su in ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if signed else [(1, 1)]):
                        ops = [list(ZERO9) for _ in bs]
                        if sqr:
                            ops[0] = [x | y for x, y in zip(hot(i, *bs[0], spare=bs[0][0]), hot(j, *bs[0], spare=bs[0][0]))]     # (room under vb q for the other limb)
                        else:
                            ops[2 * p], ops[2 * p + 1] = hot(i, *bs[2 * p], sign=sa), hot(j, *bs[2 * p + 1], sign=su)
                        emit("hot pair %d a[%d] u[%d] %+d %+d point %d" % (p, i, j, sa, su, pi), ops, bs)
    # ---- ceilings: every contract point; signed forms in every sign combination of the products (the first factor of each carries the sign)
    for pi, pt in enumerate(pts):
        bs = _flat(pt)
        hi = [_ints(at_bound(lb, vb)) if lb else list(ZERO9) for lb, vb in bs]
        if not signed:
            emit("ceiling point %d" % pi, hi, bs)
            continue
        for signs in [(1, 1), (1, -1), (-1, 1), (-1, -1)]:
            for flip in (0, 1):             # the sign on the first or on the second factor of each product
                ops = [neg_limbs(l) if (signs[k // 2] < 0 and k % 2 == flip) else l for k, l in enumerate(hi)]
                emit("ceiling point %d signs %+d %+d on factor %d" % (pi, signs[0], signs[1], flip), ops, bs)
        emit("ceiling point %d both factors negative" % pi, [neg_limbs(l) for l in hi], bs)
    # ---- degenerate
    bs1 = [(1, 1)] * (2 * npairs)
    emit("all zero", [list(ZERO9) for _ in bs1], bs1)
    emit("q - 1 everywhere", [list(QM1) for _ in bs1], bs1)
    if signed:
        emit("-(q - 1) everywhere", [neg_limbs(QM1) for _ in bs1], bs1)
        emit("q - 1 against -(q - 1)", [list(QM1) if k % 2 else neg_limbs(QM1) for k in range(len(bs1))], bs1)
    for z in range(1 if sqr else 2 * npairs):
        if not sqr:
            emit("operand %d zero, q - 1 elsewhere" % z, [list(ZERO9) if k == z else list(QM1) for k in range(len(bs1))], bs1)
    # ---- random: half with lazy limbs at the contract points in turn, half normalized values (for the signed forms: differences, both signs)
    for r in range(256):
        pt = pts[r % len(pts)]
        bs = _flat(pt)
        if signed:
            ops = [rand_sdiff(rng, vb) for lb, vb in bs]
        elif r % 2:
            ops = [rand_lazy(rng, lb, vb) if lb else list(ZERO9) for lb, vb in bs]
        else:
            ops = [norm9(rng.randrange(vb * Q)) if lb else list(ZERO9) for lb, vb in bs]
        emit("random %d" % r, ops, bs)
    return out


# ---------------------------------------------------------------------------------------------------------------- the wide reduction
WRED_CEIL = {True: ((4, 10150), (3, 2900)), False: ((4, 39150), (1, 0))}        # n.wb + 9 x.wb + px.wb + 170 d.vb = 40 000 with d at (3, 5)
WRED_D = (3, 5)


def wred_cases(name):
    d = LEAVES[LEAF_ID[name]][3]
    xi, sub = d["xi"], d["sub"]
    rng = random.Random(1000 + LEAF_ID[name])
    out = []

    def emit(cname, n, x, px, neg, dd, nb, xb, db):
        if not xi:              # the x operands are not read; their claimed bound is (1, 0)
            x, px, xb = ZERO18, ZERO18, (1, 0)
        out.append((cname, [_ints(n), _ints(x), _ints(px), _ints(dd)], [nb + (0,), xb + (0,), xb + (0,), db + (0,)], int(neg)))

    # ---- everything tests/test_hostsim_wide.py forms for this specialisation: the tower's coefficient sets ...
    for cname, cxi, nb, xb in COMBOS:
        if cxi != xi:
            continue
        d_hi = at_bound(*D_BOUND)
        for neg in (False, True):
            for sn in (1, -1):
                for sx in (1, -1):
                    for sp in (1, -1):
                        emit("%s bounds %+d %+d %+d neg %d" % (cname, sn, sx, sp, neg), wide_raw(*nb, sn), wide_raw(*xb, sx), wide_raw(*xb, sp), neg, d_hi, nb, xb, D_BOUND)
            emit("%s zero neg %d" % (cname, neg), ZERO18, ZERO18, ZERO18, neg, ZERO9, nb, xb, D_BOUND)
            emit("%s zero minus d neg %d" % (cname, neg), ZERO18, ZERO18, ZERO18, neg, d_hi, nb, xb, D_BOUND)
            qq, nq = norm18((Q - 1) * (Q - 1)), norm18(-(Q - 1) * (Q - 1))
            emit("%s (q-1)^2 neg %d" % (cname, neg), qq, qq, qq, neg, QM1, nb, xb, D_BOUND)
            emit("%s -(q-1)^2 neg %d" % (cname, neg), nq, qq, nq, neg, QM1, nb, xb, D_BOUND)
            for i in range(25):
                vals = [rng.randrange(b[1] * Q * Q + 1) * rng.choice((1, -1)) for b in (nb, xb, xb)]
                emit("%s random %d neg %d" % (cname, i, neg), *(norm18(v) for v in vals), neg, norm9(rng.randrange(6 * Q)), nb, xb, D_BOUND)
    # ---- ... and the leaf's own ceiling, raw and carry-propagated
    nb, xb = WRED_CEIL[xi]
    assert nb[1] + (10 * xb[1] if xi else 0) + 170 * WRED_D[1] == 40000
    d_hi = at_bound(*WRED_D)
    for neg in (False, True):
        for sn in (1, -1):
            for sx in (1, -1):
                for sp in (1, -1):
                    emit("ceiling %+d %+d %+d neg %d" % (sn, sx, sp, neg), wide_raw(*nb, sn), wide_raw(*xb, sx), wide_raw(*xb, sp), neg, d_hi, nb, xb, WRED_D)
                    vals = [s_ * b[1] * Q * Q for s_, b in ((sn, nb), (sx, xb), (sp, xb))]
                    emit("ceiling normalized %+d %+d %+d neg %d" % (sn, sx, sp, neg), *(norm18(v) for v in vals), neg, d_hi, nb, xb, WRED_D)
    # ---- hot limb: one limb of one operand at its ceiling (the top limbs with both signs), everything else zero
    for neg in (False, True):
        emit("all zero neg %d" % neg, ZERO18, ZERO18, ZERO18, neg, ZERO9, nb, xb, WRED_D)
        emit("all zero but d = q - 1 neg %d" % neg, ZERO18, ZERO18, ZERO18, neg, QM1, nb, xb, WRED_D)
        for oi, (w, (lb, wb)) in enumerate([(18, nb), (18, xb), (18, xb), (9, WRED_D)]):
            if (oi in (1, 2) and not xi) or (oi == 3 and not sub):
                continue
            for i in range(w):
                for sign in ((1, -1) if (w == 18 and i == 17) else (1,)):
                    ops = [list(ZERO18), list(ZERO18), list(ZERO18), list(ZERO9)]
                    if w == 18:
                        ops[oi][i] = lb * MASK29 if i < 17 else (sign * ((wb * Q * Q) >> 493)) & 0xffffffff
                    else:
                        ops[oi] = hot(i, lb, wb)
                    emit("hot operand %d limb %d %+d neg %d" % (oi, i, sign, neg), *ops[:3], neg, ops[3], nb, xb, WRED_D)
    # ---- random within the ceiling: raw limbs (not carry-propagated) with a random top limb of either sign
    for r in range(256):
        ws = []
        for lb, wb in (nb, xb, xb):
            top = rng.randrange(-((wb * Q * Q) >> 493), ((wb * Q * Q) >> 493) + 1)
            ws.append([rng.randrange(lb * MASK29 + 1) for _ in range(17)] + [top & 0xffffffff])
        emit("random %d" % r, *ws, r & 1, rand_lazy(rng, *WRED_D), nb, xb, WRED_D)
    return out


# ---------------------------------------------------------------------------------------------------------------- the fused reductions
def lc_points(d):
    """the ceiling of a fused reduction: limb bounds - wide terms at 4, the narrow part at sum |C| lb = 4 - and the value bounds with
    sum |C| vb as close to 500 as the coefficients allow (once per operand carrying the weight)"""
    C = d["C"]
    if d["family"] == "lc3w":
        lbs, cap = [8 if c else 1 for c in C], 1000
    else:
        _, _, N = lc_branch(d)
        lbs, cap = [4 if (c and not n) else 1 for c, n in zip(C, N)], 500
        grow = True
        while grow:
            grow = False
            for i, n in enumerate(N):
                if n and sum(abs(C[k]) * lbs[k] for k in range(len(C)) if N[k]) + abs(C[i]) <= 4:
                    lbs[i] += 1; grow = True
    used = [i for i, c in enumerate(C) if c]
    pts = []
    for heavy in used or [None]:
        vbs = [1] * len(C)
        rest = cap - sum(abs(C[i]) for i in used)
        for i in ([heavy] + [u for u in used if u != heavy]) if used else []:
            vbs[i] += rest // abs(C[i]); rest -= (rest // abs(C[i])) * abs(C[i])
        assert sum(abs(C[i]) * vbs[i] for i in used) <= cap
        if (lbs, vbs) not in pts:
            pts.append((lbs, vbs))
    return pts


def lc_cases(name):
    _, kinds, _, d = LEAVES[LEAF_ID[name]]
    C = d["C"][:len(kinds)]
    unsigned_only = d["family"] == "lc3w"
    flags = (0, 1) if d.get("flag") else (0,)
    rng = random.Random(1000 + LEAF_ID[name])
    pts = lc_points(d)
    used = [i for i, c in enumerate(C) if c]
    nops = len(kinds)
    out = []

    def emit(cname, ops, lbs, vbs, flag):
        out.append((cname, ops, [(lbs[i], vbs[i], 0) if unsigned_only else _b(lbs[i], vbs[i], ops[i]) for i in range(nops)], flag))

    signs_of = (lambda k: [(1,) * k]) if unsigned_only else (lambda k: [tuple(1 if (m >> b) & 1 == 0 else -1 for b in range(k)) for m in range(1 << k)])
    for flag in flags:
        lbs, vbs = pts[0]
        # ---- hot limb: every limb of every operand that is read, both signs
        for oi in used:
            for i in range(9):
                for sign in ((1,) if unsigned_only else (1, -1)):
                    ops = [list(ZERO9) for _ in range(nops)]
                    ops[oi] = hot(i, lbs[oi], vbs[oi], sign=sign)
                    emit("hot operand %d limb %d %+d flag %d" % (oi, i, sign, flag), ops, lbs, vbs, flag)
        # ---- ceilings: every point, every sign pattern of the operands
        for pi, (lbs, vbs) in enumerate(pts):
            hi = [_ints(at_bound(lbs[i], vbs[i])) if C[i] else list(ZERO9) for i in range(nops)]
            for signs in signs_of(len(used)):
                ops = list(hi)
                for s_, oi in zip(signs, used):
                    if s_ < 0:
                        ops[oi] = neg_limbs(hi[oi])
                emit("ceiling point %d signs %s flag %d" % (pi, signs, flag), ops, lbs, vbs, flag)
        # ---- degenerate
        one = [1] * nops
        emit("all zero flag %d" % flag, [list(ZERO9) for _ in range(nops)], one, one, flag)
        emit("q - 1 everywhere flag %d" % flag, [list(QM1) for _ in range(nops)], one, one, flag)
        if not unsigned_only:
            emit("-(q - 1) everywhere flag %d" % flag, [neg_limbs(QM1) for _ in range(nops)], one, one, flag)
        for z in used:
            emit("operand %d zero, q - 1 elsewhere flag %d" % (z, flag), [list(ZERO9) if k == z else list(QM1) for k in range(nops)], one, one, flag)
    # ---- random: lazy limbs at the ceiling points in turn, each operand negated limb-wise at random; every other case a difference of two values
    for r in range(256):
        lbs, vbs = pts[r % len(pts)]
        ops = []
        for i in range(nops):
            if unsigned_only or r % 2 == 0:
                l = rand_lazy(rng, lbs[i], vbs[i])
                ops.append(neg_limbs(l) if (not unsigned_only and rng.random() < 0.5) else l)
            else:
                ops.append(rand_sdiff(rng, vbs[i]))
        emit("random %d" % r, ops, lbs, vbs, flags[(r // 2) % len(flags)])
    return out


# ---------------------------------------------------------------------------------------------------------------- all cases, packed
_cache = {}


def cases(name):
    if name not in _cache:
        fam = LEAVES[LEAF_ID[name]][3]["family"]
        _cache[name] = wred_cases(name) if fam == "wred" else lc_cases(name) if fam in ("lc", "lc3w") else product_cases(name)
    return _cache[name]


def pack(name):
    """(ops uint32 [n, stride], bounds uint32 [n, 3 operands], flags int32 [n]) of cases(name)"""
    cs = cases(name)
    ops = np.array([[x for op in c[1] for x in op] for c in cs], np.uint64).astype(np.uint32)
    bounds = np.array([[x for b in c[2] for x in b] for c in cs], np.uint32)
    flags = np.array([c[3] for c in cs], np.int32)
    kinds = LEAVES[LEAF_ID[name]][1]
    assert ops.shape == (len(cs), sum(18 if k == "w" else 9 for k in kinds)) and bounds.shape == (len(cs), 3 * len(kinds))
    return ops, bounds, flags


# ---------------------------------------------------------------------------------------------------------------- the integer model
def check(name, case, got):
    """None when the result limbs `got` are what fe.hpp promises of the leaf for this case, else a short description of what is wrong"""
    _, kinds, outw, d = LEAVES[LEAF_ID[name]]
    cname, ops, bounds, flag = case
    got = _ints(got)
    fam = d["family"]
    if fam in ("mont", "sqr"):
        signed = d.get("signed", False)
        vals = [value(l, signed=signed) for l in ops]
        if fam == "sqr":
            vals = vals * 2
        total = sum(vals[k] * vals[k + 1] for k in range(0, len(vals), 2))
        bound = d.get("bound") or (2 if sum(bounds[k][1] * bounds[k + 1][1] for k in range(0, len(bounds), 2)) <= 169 else 3)
        if any(x > MASK29 for x in got[:8]):
            return "a limb beyond 29 bits"
        r = value(got, top_signed=signed)
        if not (abs(r) if signed else r) < bound * Q or r < 0 and not signed:
            return "value %d q, stated bound %d q" % (r // Q, bound)
        return None if (r * R261 - total) % Q == 0 else "wrong residue"
    if fam == "wide":
        signed = d.get("signed", False)
        v = [value(l, signed=signed) for l in ops]
        if any(x > MASK29 for x in got[:17]):
            return "a limb beyond 29 bits"
        return None if value(got, top_signed=True) == v[0] * v[1] + v[2] * v[3] else "not the integer a u + c v"
    if fam == "wred":
        T = value(ops[0], top_signed=True)
        if d["xi"]:
            T += 9 * value(ops[1], top_signed=True) + (-1 if flag else 1) * value(ops[2], top_signed=True)
        want = T * RINV - (value(ops[3]) if d["sub"] else 0)
        r = value(got)
        if any(x > MASK29 for x in got[:8]):
            return "a limb beyond 29 bits"
        if not 0 <= r < 3 * Q:
            return "value %d q outside [0, 3q)" % (r // Q)
        return None if (r - want) % Q == 0 else "wrong residue"
    C = list(d["C"][:len(kinds)])
    if flag:
        C[1] = -C[1]
    want = sum(c * value(l, signed=(fam == "lc")) for c, l in zip(C, ops))
    r = value(got, top_signed=True)
    if any(x > MASK29 for x in got[:8]):
        return "a limb beyond 29 bits"
    if not 0 <= r < 3 * Q:
        return "value %d q outside [0, 3q)" % (r // Q)
    return None if (r - want) % Q == 0 else "wrong residue"


def failures(name, got, limit=5):
    """(count, the first few 'case name: what is wrong') of a leaf's results against the model"""
    bad = [(c[0], e) for c, g in zip(cases(name), got) for e in [check(name, c, g)] if e]
    return len(bad), ["%s: %s" % b for b in bad[:limit]]
