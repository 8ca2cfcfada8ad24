"""The lazily reduced Karatsuba products of the lane-pair tower (bn_amd/csrc/fe.hpp fe_wmul2 / fe_wmul2s / fe_wred, tower.hpp f6_mul_lazy and
the Fq2B forms of f12_mul_src / f12_sqr) in the host simulation, bounds enforced (tests/hostsim/hostsim_wide.cpp):

  * the wide dual product against Python integers - the 18 limbs ARE a*u + c*v, before any reduction;
  * the wide reduction against (n + xi-combination) R^-1 - d mod q for every coefficient set the tower uses, with operands at the stated limb
    and value bounds, all-zero operands, q - 1, and signed differences of both signs;
  * f6_mul, f12_mul and f12_sqr of the lane-pair mapping bit for bit against the oracle on the 64 edge elements of tests/edge_inputs.py (each as
    the left and as the right operand) and on 200 random elements;
  * the same three with TWO lane pairs side by side - the even and the odd slot of a batch, simulated by lanequad.hpp's four-lane value type -
    every edge element once on the even and once on the odd slot, a different element on the other one.  (The slots of a real batch, with
    ragged waves and dead lanes, are the GPU test's: tests/test_gpu_wide_tower.py.)
"""
import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
import hostsim_wide_lib as W
from leaf_cases import COMBOS, D_BOUND, at_bound, sdiff, wide_raw          # the case makers shared with the leaf tests

Q = M.Q
R261 = 1 << 261
MASK29 = W.MASK29


def norm9(v):
    return W.limbs9(v)


# ---------------------------------------------------------------------------------------------------------------- the wide product
def _unsigned_cases():
    rng = np.random.default_rng(5)
    zero = norm9(0)
    # the operand contract of the lane-pair product: a, c (own and partner's component of the first operand): lb <= 2, vb <= 6;  u: standard
    # form (1, 3);  v: the biased negation fe_neg<1, 9> of a standard element (2, 9)
    A, U, V = at_bound(2, 6), at_bound(1, 3), at_bound(2, 9)
    B = ((2, 6), (1, 3), (2, 6), (2, 9))
    yield "at the bounds", (A, U, A, V), B
    yield "all zero", (zero, zero, zero, zero), B
    yield "q - 1", (norm9(Q - 1),) * 4, ((1, 1),) * 4
    yield "zero partner", (A, U, zero, zero), B
    for i in range(20):
        ops = tuple(norm9(int.from_bytes(rng.bytes(32), "little") % (3 * Q)) for _ in range(4))
        yield "random %d" % i, ops, ((1, 3),) * 4


def test_wide_product_is_the_integer():
    for name, ops, bounds in _unsigned_cases():
        got = W.wmul2(False, *ops, bounds)
        a, u, c, v = (W.limbs_value(x) for x in ops)
        assert all(int(l) <= MASK29 for l in got[:17]), name
        assert W.limbs_value(got, top_signed=True) == a * u + c * v, name


def _signed_cases():
    rng = np.random.default_rng(6)
    hi, lo, zero = at_bound(1, 3), norm9(0), norm9(0)
    mid = norm9(Q - 1)
    # differences of standard elements, of both signs and at both extremes: (1, 3) each, value bound max(3, 3)
    B = ((1, 3),) * 4
    yield "largest positive times largest negative", (sdiff(hi, lo), sdiff(lo, hi), sdiff(hi, lo), sdiff(lo, hi)), B
    yield "negative times negative", (sdiff(lo, hi), sdiff(lo, hi), sdiff(lo, hi), sdiff(lo, hi)), B
    yield "positive times positive", (sdiff(hi, lo), sdiff(hi, lo), sdiff(hi, lo), sdiff(hi, lo)), B
    yield "all zero", (zero,) * 4, B
    yield "q - 1 against 0", (sdiff(mid, lo), sdiff(lo, mid), sdiff(lo, mid), sdiff(mid, lo)), B
    yield "equal operands", (sdiff(mid, mid), sdiff(hi, hi), sdiff(mid, mid), sdiff(hi, hi)), B
    for i in range(20):
        r = [norm9(int.from_bytes(rng.bytes(32), "little") % (3 * Q)) for _ in range(8)]
        yield "random %d" % i, tuple(sdiff(r[2 * j], r[2 * j + 1]) for j in range(4)), B


def test_signed_wide_product_is_the_integer():
    seen = set()
    for name, ops, bounds in _signed_cases():
        got = W.wmul2(True, *ops, bounds)
        a, u, c, v = (W.limbs_value(x, signed_limbs=True) for x in ops)
        want = a * u + c * v
        seen.add((want > 0) - (want < 0))
        assert all(int(l) <= MASK29 for l in got[:17]), name
        assert W.limbs_value(got, top_signed=True) == want, name
    assert seen == {-1, 0, 1}


# ---------------------------------------------------------------------------------------------------------------- the wide reduction
def _check_wred(name, xi, sub, n, x, px, neg, d, bounds):
    got = W.wred(xi, sub, n, x, px, neg, d, bounds)
    T = W.limbs_value(n, top_signed=True)
    if xi:
        T += 9 * W.limbs_value(x, top_signed=True) + (-1 if neg else 1) * W.limbs_value(px, top_signed=True)
    want = T * pow(R261, -1, Q) - (W.limbs_value(d) if sub else 0)
    r = W.limbs_value(got)
    assert all(int(l) <= MASK29 for l in got[:8]), name
    assert 0 <= r < 3 * Q, (name, r // Q)
    assert (r - want) % Q == 0, name


def test_wide_reduction_of_every_coefficient_set():
    rng = np.random.default_rng(7)
    zero18, zero9 = W.limbs18(0), norm9(0)
    for cname, xi, nb, xb in COMBOS:
        for sub in (False, True):
            for neg in (False, True):
                tag = (cname, sub, neg)
                bounds = (nb, xb, xb, D_BOUND)
                d_hi = at_bound(*D_BOUND)
                # at the bounds, every sign pattern of the three wide terms
                for sn in (1, -1):
                    for sx in (1, -1):
                        for sp in (1, -1):
                            _check_wred((tag, "bounds", sn, sx, sp), xi, sub, wide_raw(*nb, sn), wide_raw(*xb, sx), wide_raw(*xb, sp), neg, d_hi, bounds)
                _check_wred((tag, "zero"), xi, sub, zero18, zero18, zero18, neg, zero9, bounds)
                _check_wred((tag, "zero minus d"), xi, sub, zero18, zero18, zero18, neg, d_hi, bounds)
                qq, nq = W.limbs18((Q - 1) * (Q - 1)), W.limbs18(-(Q - 1) * (Q - 1))
                xq, xn = (qq, nq) if xi else (zero18, zero18)          # (without xi the x operands are not read; their claimed bound is zero)
                _check_wred((tag, "(q-1)^2"), xi, sub, qq, xq, xq, neg, norm9(Q - 1), bounds)
                _check_wred((tag, "-(q-1)^2"), xi, sub, nq, xq, xn, neg, norm9(Q - 1), bounds)
                for i in range(25):
                    vals = [int.from_bytes(rng.bytes(70), "little") % (b[1] * Q * Q + 1) * (1 if rng.integers(2) else -1) for b in (nb, xb, xb)]
                    d = norm9(int.from_bytes(rng.bytes(32), "little") % (6 * Q))
                    _check_wred((tag, "random", i), xi, sub, *(W.limbs18(v) for v in vals), neg, d, bounds)


def test_wide_reduction_at_the_stated_ceiling():
    """the leaf's own bounds, beyond anything the tower forms: n.wb + 9 x.wb + px.wb + 170 d.vb = 40 000 (the |te| < 2^31 and column-sum claims of
    fe.hpp fe_wred), n.lb = 4, x.lb = 3, d at (3, 5); every sign pattern, both lane parities, with and without the subtrahend"""
    d_bound = (3, 5)
    for cname, xi, nb, xb in [("xi", True, (4, 10150), (3, 2900)), ("plain", False, (4, 39150), (1, 0))]:
        assert nb[1] + (10 * xb[1] if xi else 0) + 170 * d_bound[1] == 40000
        bounds = (nb, xb, xb, d_bound)
        for sub in (False, True):
            for neg in (False, True):
                for sn in (1, -1):
                    for sx in (1, -1):
                        for sp in (1, -1):
                            _check_wred((cname, sub, neg, sn, sx, sp), xi, sub, wide_raw(*nb, sn), wide_raw(*xb, sx), wide_raw(*xb, sp), neg, at_bound(*d_bound), bounds)
                            # the same values with carry-propagated limbs (the top limb alone carries the bound)
                            vals = [s_ * b[1] * Q * Q for s_, b in ((sn, nb), (sx, xb), (sp, xb))]
                            _check_wred((cname, sub, neg, sn, sx, sp, "normalized"), xi, sub, *(W.limbs18(v) for v in vals), neg, at_bound(*d_bound), bounds)


def test_wide_sum_and_reduction_of_real_products():
    """the path of one coefficient as the tower walks it: three products, their limb-wise sum, one reduction - against the integers"""
    rng = np.random.default_rng(8)
    for i in range(10):
        r = [int.from_bytes(rng.bytes(32), "little") % (3 * Q) for _ in range(12)]
        S = ((1, 3),) * 4
        v0 = W.wmul2(False, *(norm9(x) for x in r[0:4]), S)
        v1 = W.wmul2(False, *(norm9(x) for x in r[4:8]), S)
        m = W.wmul2(True, sdiff(norm9(r[8]), norm9(r[9])), sdiff(norm9(r[10]), norm9(r[11])), sdiff(norm9(r[9]), norm9(r[8])), sdiff(norm9(r[11]), norm9(r[10])), S)
        x01 = W.wadd(W.wadd(m, v0, ((1, 18), (1, 18))), v1, ((2, 36), (1, 18)))
        want = r[0] * r[1] + r[2] * r[3] + r[4] * r[5] + r[6] * r[7] + 2 * (r[8] - r[9]) * (r[10] - r[11])
        assert W.limbs_value(x01, top_signed=True) == want
        got = W.wred(False, False, x01, x01, x01, False, norm9(0), ((3, 54), (3, 54), (3, 54), (1, 1)))
        assert (W.limbs_value(got) * R261 - want) % Q == 0 and W.limbs_value(got) < 3 * Q


# ---------------------------------------------------------------------------------------------------------------- the tower
@pytest.fixture(scope="module")
def elements(oracle):
    """(names, 64 edge elements, their fixed partners, 200 random elements)"""
    edge = E.edge_fq12(oracle)
    names, vals = list(edge), list(edge.values())
    partners = [vals[j] for j in E.edge_partners(len(vals))]
    rng = np.random.default_rng(9)
    rnd = [oracle.fq12_from_ints([int.from_bytes(rng.bytes(40), "little") % Q for _ in range(12)]) for _ in range(200)]
    return names, vals, partners, rnd


def test_fq6_mul_lazy_against_the_oracle(oracle, elements):
    names, vals, partners, rnd = elements
    for name, a, b in zip(names, vals, partners):
        for x, y in ((a[:24], b[:24]), (b[:24], a[:24]), (a[:24], a[24:]), (a[24:], b[24:])):
            assert np.array_equal(W.fq6_mul(x, y), oracle.fq6_mul(x, y)), name
    for i in range(0, 200, 2):
        x, y = rnd[i], rnd[i + 1]
        for p, q in ((x[:24], y[:24]), (x[24:], y[24:])):
            want = oracle.fq6_mul(p, q)
            assert np.array_equal(W.fq6_mul(p, q), want) and np.array_equal(W.fq6_mul(p, q, wide=False), want), i


def test_fq6_mul_lazy_with_the_subtrahend_inside(oracle, elements):
    names, vals, partners, rnd = elements
    pad = np.zeros(24, np.uint64)
    def want(a, b, d):
        return oracle.fq12_sub(np.concatenate([oracle.fq6_mul(a, b), pad]), np.concatenate([d, pad]))[:24]
    for name, a, b in zip(names, vals, partners):
        assert np.array_equal(W.fq6_mul_sub(a[:24], b[:24], a[24:]), want(a[:24], b[:24], a[24:])), name
        assert np.array_equal(W.fq6_mul_sub(b[24:], a[24:], b[:24]), want(b[24:], a[24:], b[:24])), name
    for i in range(0, 200, 2):
        x, y = rnd[i], rnd[i + 1]
        assert np.array_equal(W.fq6_mul_sub(x[:24], y[:24], y[24:]), want(x[:24], y[:24], y[24:])), i


def test_fq12_mul_lazy_against_the_oracle(oracle, elements):
    names, vals, partners, rnd = elements
    for name, a, b in zip(names, vals, partners):
        want = oracle.fq12_mul(a, b)
        assert np.array_equal(W.fq12_mul(a, b), want), (name, "left")
        assert np.array_equal(W.fq12_mul(b, a), want), (name, "right")
        assert np.array_equal(W.fq12_mul(a, b, conj=True), oracle.fq12_mul(a, oracle.fq12_unitary_inverse(b))), (name, "conjugate")
    for i in range(200):
        a, b = rnd[i], rnd[(i + 1) % 200]
        want = oracle.fq12_mul(a, b)
        assert np.array_equal(W.fq12_mul(a, b), want), i
        if i < 20:
            assert np.array_equal(W.fq12_mul(a, b, wide=False), want), i


def test_fq12_sqr_lazy_against_the_oracle(oracle, elements):
    names, vals, partners, rnd = elements
    for name, a in list(zip(names, vals)) + [("random %d" % i, a) for i, a in enumerate(rnd)]:
        want = oracle.fq12_sqr(a)
        for reduced_c1 in (False, True):
            assert np.array_equal(W.fq12_sqr(a, reduced_c1=reduced_c1), want), (name, reduced_c1)
    for a in rnd[:20]:
        assert np.array_equal(W.fq12_sqr(a, wide=False), oracle.fq12_sqr(a))


def test_two_slots_side_by_side(oracle, elements):
    """two lane pairs in one call, each edge element once on the even slot (its partner element on the odd one) and once on the odd slot"""
    names, vals, partners, rnd = elements
    n = len(vals)
    for i, (name, a, b) in enumerate(zip(names, vals, partners)):
        c, d = vals[(i + 7) % n], partners[(i + 7) % n]           # what the other slot computes
        for (ae, be, ao, bo) in ((a, b, c, d), (c, d, a, b)):
            ge, go = W.fq12_mul_slots(ae, be, ao, bo)
            assert np.array_equal(ge, oracle.fq12_mul(ae, be)) and np.array_equal(go, oracle.fq12_mul(ao, bo)), (name, "f12_mul")
            ge, go = W.fq6_mul_slots(ae[:24], be[24:], ao[:24], bo[24:])
            assert np.array_equal(ge, oracle.fq6_mul(ae[:24], be[24:])) and np.array_equal(go, oracle.fq6_mul(ao[:24], bo[24:])), (name, "f6_mul")
        for (ae, ao) in ((a, c), (c, a)):
            for reduced_c1 in (False, True):
                ge, go = W.fq12_sqr_slots(ae, ao, reduced_c1)
                assert np.array_equal(ge, oracle.fq12_sqr(ae)) and np.array_equal(go, oracle.fq12_sqr(ao)), (name, "f12_sqr", reduced_c1)
    for i in range(0, 200, 4):
        ge, go = W.fq12_mul_slots(rnd[i], rnd[i + 1], rnd[i + 2], rnd[i + 3])
        assert np.array_equal(ge, oracle.fq12_mul(rnd[i], rnd[i + 1])) and np.array_equal(go, oracle.fq12_mul(rnd[i + 2], rnd[i + 3])), i


def test_chains_keep_the_bounds(oracle, elements):
    """outputs fed back as they are: six squarings in the reduced form (Gt::pow's shape), and (a^2) * a three times (a Miller step's square feeding a product)"""
    names, vals, partners, rnd = elements
    for a in [vals[names.index("all q-1")], vals[names.index("0,q-1 x6")], rnd[0], rnd[1]]:
        want = a
        for _ in range(6):
            want = oracle.fq12_sqr(want)
        assert np.array_equal(W.fq12_sqr_chain(a, 6, True), want)
        want = a
        for _ in range(3):
            want = oracle.fq12_mul(oracle.fq12_sqr(want), want)
        assert np.array_equal(W.fq12_sqr_chain(a, 3, False), want)


def test_multiply_instruction_counts(elements):
    """the design arithmetic: six wide products and three wide reductions per Fq6 product"""
    names, vals, partners, rnd = elements
    a, b = rnd[0], rnd[1]
    f6 = 6 * 162 + 2 * (100 + 18 + 36) + (100 + 18)
    assert W.macs(0, a, b) == f6 == 1398
    assert W.macs(2, a, b) == 2 * f6 + (f6 + 27) + 37 + 19 + 19
    assert W.macs(4, a, b) == 2 * f6 + 27 + 37 + 37
    assert W.macs(0, a, b) <= 0.88 * W.macs(1, a, b) and W.macs(2, a, b) <= 0.88 * W.macs(3, a, b) and W.macs(4, a, b) <= 0.89 * W.macs(5, a, b)
