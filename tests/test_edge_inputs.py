"""CPU checks of tests/edge_inputs.py: every edge representation is the point it came from, the edge points are group elements,
and the crafted scalars drive the device's GLV / GLS splits (bn_amd/csrc/curve.hpp, compiled for the CPU by tests/hostsim/) further
than random scalars do.  The GPU side of these inputs is tests/test_gpu_edges.py."""
import random
from fractions import Fraction

import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
import hostsim_lib
from bn_oracle import FR
from conftest import canon_infinity


@pytest.fixture(scope="module")
def hs():
    return hostsim_lib.HostSim(bounds=True)


def test_edge_z_values():
    """the Fq edge values are what their names say; FE_LIMBS_MAX / _MIN have the claimed 9 x 29-bit internal images (x 2^261 mod q)"""
    assert all(0 < z < M.Q for z in E.FQ_Z) and len(set(E.FQ_Z)) == len(E.FQ_Z)
    assert all(M.f2_mul(z, M.f2_inv(z)) == M.F2_ONE for z in E.FQ2_Z) and len(set(E.FQ2_Z)) == len(E.FQ2_Z)
    assert E.R_INV * M.MONT_R % M.Q == 1
    limbs = lambda v: [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [v >> 232]
    hi, lo = limbs(E.FE_LIMBS_MAX * (1 << 261) % M.Q), limbs(E.FE_LIMBS_MIN * (1 << 261) % M.Q)
    assert hi[:8] == [(1 << 29) - 1] * 8 and hi[8] == (M.Q >> 232) - 1
    assert lo[:8] == [0] * 8 and lo[8] == M.Q >> 232


def test_edge_points_are_group_elements(oracle):
    """the smallest- and largest-x G1 points are on the curve and of order r (cofactor 1: r P = (r - 1) P + P = 0); k G2 for the edge k"""
    aff = E.edge_g1_affine()
    assert aff[0][0] < 64 and aff[2][0] > M.Q - 64 and aff[0][1] == M.Q - aff[1][1] and aff[2][1] == M.Q - aff[3][1]
    for (x, y), p in zip(aff, E.edge_g1_points(oracle)):
        assert (y * y - x ** 3 - 3) % M.Q == 0
        rp = oracle.g1_add(oracle.g1_mul(p, oracle.fp_from_int(FR, M.R_ORD - 1)), p)
        assert not rp[8:].any(), (x, y)
    g2 = E.edge_g2_points(oracle)
    assert oracle.g2_eq(g2[0], oracle.g2_one()) and oracle.g2_eq(oracle.g2_add(g2[0], g2[1]), oracle.g2_zero())


def test_rescaled_points_equal_their_source(oracle):
    """rescale(P, z) is P in another Jacobian representation, for every edge z, on edge, random and infinite points"""
    rng = np.random.default_rng(501)
    k = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(2)])
    g1 = E.edge_g1_points(oracle) + [oracle.g1_mul_batch_jacobian(oracle.g1_one().reshape(1, 12), k[:1])[0], oracle.g1_zero()]
    g2 = E.edge_g2_points(oracle) + [oracle.g2_mul_batch_jacobian(oracle.g2_one().reshape(1, 24), k[1:])[0], oracle.g2_zero()]
    for p in g1:
        for z in E.FQ_Z:
            r = E.rescale_g1(oracle, p, z)
            assert oracle.g1_eq(r, p), z
            assert z == 1 or not p[8:].any() or not np.array_equal(r, p), z     # a different representation (unless z = 1 or infinity)
    for p in g2:
        for z in E.FQ2_Z:
            r = E.rescale_g2(oracle, p, z)
            assert oracle.g2_eq(r, p), z
            assert z == (1, 0) or not p[16:].any() or not np.array_equal(r, p), z


def _glv_device(oracle, hs, k):
    d = hs.call("hs_glv_decompose", oracle.fp_from_int(FR, k), out_words=12).view(np.uint32)
    m1 = sum(int(d[i]) << (32 * i) for i in range(5)); m2 = sum(int(d[6 + i]) << (32 * i) for i in range(5))
    return m1, int(d[5]), m2, int(d[11])


def _gls_device(oracle, hs, k):
    d = hs.call("hs_gls_decompose", oracle.fp_from_int(FR, k), out_words=16).view(np.uint32)
    return [(int(d[4 * i]) | int(d[4 * i + 1]) << 32 | int(d[4 * i + 2]) << 64, int(d[4 * i + 3])) for i in range(4)]


def _random_scalars(seed, n=20000):
    rnd = random.Random(seed)
    return [rnd.randrange(M.R_ORD) for _ in range(n)]


def test_glv_split_of_crafted_scalars(oracle, hs):
    """glv_decompose on the crafted set: a valid split equal to the integer model, larger parts than 20 000 random scalars reach, every
    sign pattern the split can produce.  What the split CAN produce: the device takes c_i = floor(k G_i / 2^256) with G_i rounded down,
    so c_i is the true floor or one less and (k1, k2) = s v1 + t v2 with 0 <= s < 1 + r d1, 0 <= t < 1 + r d2 (d_i: the rounding of
    G_i / 2^256).  k1 = s a1 + t a2 >= 0 (a1, a2 > 0): neg1 is never set; |k1|, |k2| stay below the bound B computed here, which is
    below 2^127 - so the top Booth window (32, bits 127..131) is never reached by any canonical scalar and the highest reachable is 31"""
    lam = E.GLV_LAMBDA
    def stats(ks):
        mx, signs, top = 0, set(), -1
        for k in ks:
            m1, s1, m2, s2 = _glv_device(oracle, hs, k)
            assert (m1, s1, m2, s2) == E.glv_split(k), k
            assert ((-m1 if s1 else m1) + (-m2 if s2 else m2) * lam - k) % M.R_ORD == 0, k
            mx = max(mx, m1, m2); signs.add((s1, s2)); top = max(top, E.top_window(m1, E.GLV_WINDOWS), E.top_window(m2, E.GLV_WINDOWS))
        return mx, signs, top
    crafted = E.glv_crafted()
    cmax, csigns, ctop = stats(crafted)
    rmax, rsigns, rtop = stats(_random_scalars(3))
    assert cmax > rmax, (hex(cmax), hex(rmax))
    d1 = Fraction((E.GLV_B2 << 256) - E.GLV_G1 * M.R_ORD, M.R_ORD << 256)
    d2 = Fraction((-E.GLV_B1 << 256) - E.GLV_G2 * M.R_ORD, M.R_ORD << 256)
    s_max, t_max = 1 + M.R_ORD * d1, 1 + M.R_ORD * d2
    bound = max(s_max * E.GLV_A1 + t_max * E.GLV_A2, s_max * -E.GLV_B1, t_max * E.GLV_B2)      # k2 = s b1 + t b2: opposite signs
    assert cmax <= bound < 2 ** 127
    assert cmax > bound * Fraction(999, 1000)                # the crafted set sits at the bound
    assert csigns == {(0, 0), (0, 1)} and rsigns <= csigns    # every producible pattern (neg1 = 0 always; k2 >= 0 needs s < t b2 / |b1|)
    assert ctop == E.GLV_WINDOWS - 2 and rtop <= ctop
    print("GLV: crafted max |k_i| %#x (random %#x), bound %#x; highest Booth window %d of %d" % (cmax, rmax, int(bound), ctop, E.GLV_WINDOWS - 1))


def _gls_reachable_sign_patterns():
    """sign patterns of (k_0..k_3) = sum_j sign(g_j) f_j B_j over f in [0, 1]^4, f_j = k |g_j| - c_j (the split's remainder, see
    gls_decompose; g = row 0 of the inverse basis): a 17^4 grid plus 200 000 random points of the cube"""
    w = np.array([[(-1 if E.GLS_GNEG[j] else 1) * float(E.GLS_B[j][i]) for i in range(4)] for j in range(4)])
    g = np.linspace(0, 1, 17)
    f = np.stack(np.meshgrid(g, g, g, g, indexing="ij"), -1).reshape(-1, 4)
    f = np.concatenate([f, np.random.default_rng(7).random((200000, 4))])
    v = f @ w                                                # k e_0 = sum_j k g_j B_j and the device subtracts sign(g_j) c_j B_j
    v[np.abs(v) < 1] = 0
    return {tuple(int(x) for x in row) for row in np.unique(v < 0, axis=0)}


def test_gls_split_of_crafted_scalars(oracle, hs):
    """gls_decompose on the crafted set (G2 mul and Gt::pow's default chain): a valid split equal to the integer model, larger parts than
    20 000 random scalars, every producible sign pattern.  Bound: c_j is the true floor of k |g_j| or one less (G_j rounded down, the
    rounding times k below 2^-34), so |k_i| <= (1 + 2^-34) sum_j |B_ji| < 2^66: the top Booth window (17, bits 67..71) is never reached
    and the highest reachable is 16 (bits 63..67)"""
    lam = E.GLS_LAMBDA
    def stats(ks):
        mx, signs, top = 0, set(), -1
        for k in ks:
            parts = _gls_device(oracle, hs, k)
            assert parts == E.gls_split(k), k
            assert sum((-m if s else m) * pow(lam, i, M.R_ORD) for i, (m, s) in enumerate(parts)) % M.R_ORD == k
            mx = max(mx, max(m for m, _ in parts)); signs.add(tuple(s for _, s in parts))
            top = max(top, max(E.top_window(m, E.GLS_WINDOWS) for m, _ in parts))
        return mx, signs, top
    cmax, csigns, ctop = stats(E.gls_crafted())
    rmax, rsigns, rtop = stats(_random_scalars(4))
    assert cmax > rmax, (hex(cmax), hex(rmax))
    bound = max(sum(abs(E.GLS_B[j][i]) for j in range(4)) for i in range(4)) * (1 + Fraction(M.R_ORD, 1 << 288))
    assert M.R_ORD * max(E.GLS_G) < (1 << 288) * (1 << 256) and cmax <= bound < 2 ** 66
    reachable = _gls_reachable_sign_patterns()
    assert len(reachable) < 16 and rsigns <= reachable
    assert csigns == reachable, sorted(reachable - csigns)
    assert {tuple(s for _, s in E.gls_split(k)) for k in E.crafted_gls_by_sign()} == reachable
    assert ctop == E.GLS_WINDOWS - 2 and rtop <= ctop
    print("GLS: crafted max |k_i| %#x (random %#x), bound %#x; %d of 16 sign patterns producible; highest Booth window %d of %d"
          % (cmax, rmax, int(bound), len(reachable), ctop, E.GLS_WINDOWS - 1))


def test_crafted_scalars_through_the_device_chains(oracle, hs):
    """the G1 GLV chain and the G2 GLS chain of the kernels (host build, bounds enforced) on edge points in edge representations times
    crafted scalars, normalized, against the reference's G * Fr"""
    g1 = E.edge_g1_points(oracle)
    for i, kv in enumerate(E.glv_crafted()[::6]):
        p = E.rescale_g1(oracle, g1[i % 4], E.FQ_Z[i % len(E.FQ_Z)])
        k = oracle.fp_from_int(FR, kv)
        assert np.array_equal(hs.call("hs_g1_mul_glv", p, k, out_words=24), canon_infinity(oracle.g1_normalize(oracle.g1_mul(p, k)))), kv
    g2 = E.edge_g2_points(oracle)
    for i, kv in enumerate(E.crafted_gls_by_sign() + E.gls_crafted()[::40]):
        q = E.rescale_g2(oracle, g2[i % 3], E.FQ2_Z[i % len(E.FQ2_Z)])
        k = oracle.fp_from_int(FR, kv)
        want = canon_infinity(oracle.g2_normalize(oracle.g2_mul(q, k)))
        assert np.array_equal(hs.call("hs_g2_mul_gls", q, k, out_words=48), want), kv
        assert np.array_equal(hs.call("hsb_g2_mul_gls", q, k, out_words=48), want), kv


def test_edge_fq12_set(oracle):
    """the 64 edge Fq12 elements are what their names say (checked with the independent big-integer model), non-zero and distinct but for -1, which the list holds twice; their
    easy-part images are cyclotomic, their final exponentiations have an order dividing r, and the Fq6-subfield elements map to one"""
    ints = E.edge_fq12_ints()
    edge = E.edge_fq12(oracle)
    assert len(ints) == 64 and list(edge) == list(ints)
    # (the list names -1 twice: on its own and as the first of the twelve single slots; everything else is distinct)
    assert ints["-1"] == ints["q-1 in slot 0"] and len({tuple(v) for v in ints.values()}) == 63
    assert all(len(v) == 12 and any(v) and all(0 <= c < M.Q for c in v) for v in ints.values())
    assert all(c in E.FQ12_POOL for nm, v in ints.items() if nm.startswith("pool draw") for c in v)
    assert sum(nm.startswith("pool draw") for nm in ints) == 40 and sum(nm.startswith("q-1 in slot") for nm in ints) == 12
    m1 = ints["-1"]
    assert m1 == [M.Q - 1] + [0] * 11 and ints["w"][6] == 1 and sum(ints["w"]) == 1 and ints["c0 only"] == [M.Q - 1] * 6 + [0] * 6
    f12 = lambda v: (((v[0], v[1]), (v[2], v[3]), (v[4], v[5])), ((v[6], v[7]), (v[8], v[9]), (v[10], v[11])))
    flat = lambda x: [c for h in x for f2 in h for c in f2]
    assert flat(M.f12_mul(f12(m1), f12(m1))) == ints["one"] and flat(M.f12_mul(f12(ints["w"]), f12(ints["w"]))) == [0, 0, 1, 0] + [0] * 8   # w^2 = v
    for nm, a in edge.items():
        assert oracle.fq12_to_ints(a) == ints[nm], nm
    one = oracle.fq12_one()
    rm1 = oracle.fp_from_int(FR, M.R_ORD - 1)
    for nm, c, g in zip(edge, E.edge_cyclotomic(oracle), E.edge_gt(oracle)):
        assert E.oracle_is_cyclotomic(oracle, c), nm
        assert np.array_equal(oracle.fq12_mul(oracle.gt_pow(g, rm1), g), one), nm                       # g^r == 1
    gt = dict(zip(edge, E.edge_gt(oracle)))
    assert np.array_equal(gt["c0 only"], one) and np.array_equal(gt["-1"], one) and not np.array_equal(gt["all q-1"], one)
    p = E.edge_partners()
    assert len(p) == 64 and all(0 <= j < 64 and j != i for i, j in enumerate(p))
