"""GPU parity at the edges (run with -m gpu on an MI355X): G1/G2 mul, group addition, Gt::pow, the pairing routes and the wire codecs on
edge representations, edge points and crafted scalars (tests/edge_inputs.py), the launch seams of the scalar multiplications, and the
decoders at the exact modulus limits.  Every comparison is bit for bit against the oracle or, for the seams, device against device."""
import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
from bn_oracle import FR
from conftest import canon_infinity

pytestmark = pytest.mark.gpu

EDGE_SCALARS = [0, 1, 2, M.R_ORD - 1, M.R_ORD - 2, 1 << 200]          # test_gpu_parity.py's


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def te(eng):
    import torch
    from bn_amd import distributed as D
    return D.TorchEngine(eng, torch.device("cuda", 0))


def _random_jacobian(oracle, rng, n, g):
    k = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(n)])
    if g == 1:
        return list(oracle.g1_mul_batch_jacobian(np.tile(oracle.g1_one(), (n, 1)), k))
    return list(oracle.g2_mul_batch_jacobian(np.tile(oracle.g2_one(), (n, 1)), k))


def _g1_edge_reps(oracle, rng):
    """edge points, a random Jacobian point and infinity, each under every edge z"""
    base = E.edge_g1_points(oracle) + _random_jacobian(oracle, rng, 1, 1) + [oracle.g1_zero()]
    return [E.rescale_g1(oracle, p, z) for p in base for z in E.FQ_Z]


def _g2_edge_reps(oracle, rng):
    base = E.edge_g2_points(oracle) + _random_jacobian(oracle, rng, 1, 2) + [oracle.g2_zero()]
    return [E.rescale_g2(oracle, p, z) for p in base for z in E.FQ2_Z]


def _dev(te, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(te.device)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _mul_case(oracle, te, eng, g, points, scalars):
    """points x scalars paired cyclically (every point and every scalar at least once): the normalizing kernel against the reference's
    G * Fr, and the reference chain (bn254_g*_mul_jacobian_dev) against the oracle's raw Jacobian limbs"""
    import torch
    n = max(len(points), len(scalars))
    P = np.stack([points[i % len(points)] for i in range(n)])
    k = E.fr(oracle, [scalars[i % len(scalars)] for i in range(n)])
    if g == 1:
        got, want = eng.g1_mul_batch(P, k), canon_infinity(oracle.g1_mul_batch(P, k))
        jac = te.g1_mul(_dev(te, P), _dev(te, k), normalize=False); want_jac = oracle.g1_mul_batch_jacobian(P, k)
    else:
        got, want = eng.g2_mul_batch(P, k), canon_infinity(oracle.g2_mul_batch(P, k))
        jac = te.g2_mul(_dev(te, P), _dev(te, k), normalize=False); want_jac = oracle.g2_mul_batch_jacobian(P, k)
    torch.cuda.synchronize()
    bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not bad, ("normalized", bad[:8])
    bad = [i for i in range(n) if not np.array_equal(_host(jac)[i], want_jac[i])]
    assert not bad, ("jacobian", bad[:8])


def test_g1_mul_edge_representations_and_crafted_scalars(oracle, te, eng):
    """bn254_g1_mul_M (GLV split, signed windows, jac_madd_signed / jac_double over Fq) on edge-z points x crafted GLV scalars"""
    rng = np.random.default_rng(601)
    _mul_case(oracle, te, eng, 1, _g1_edge_reps(oracle, rng), E.glv_crafted() + EDGE_SCALARS)


def test_g2_mul_edge_representations_and_crafted_scalars(oracle, te, eng):
    """bn254_g2_mul_M (four-way GLS split) on edge-z points x crafted GLS scalars, one per producible sign pattern first"""
    rng = np.random.default_rng(602)
    ks = E.crafted_gls_by_sign() + E.gls_crafted()[::3] + EDGE_SCALARS
    _mul_case(oracle, te, eng, 2, _g2_edge_reps(oracle, rng), ks)


def _add_pairs(oracle, rng, g):
    """(a, b) rows: the same point in two representations (the doubling branch), P and -P in two representations (infinity), an edge-z
    point plus infinity (also infinity with x, y != 0), a generic sum"""
    zs = E.FQ_Z if g == 1 else E.FQ2_Z
    rs = E.rescale_g1 if g == 1 else E.rescale_g2
    neg, zero = (oracle.g1_neg, oracle.g1_zero()) if g == 1 else (oracle.g2_neg, oracle.g2_zero())
    pts = (E.edge_g1_points(oracle) if g == 1 else E.edge_g2_points(oracle)) + _random_jacobian(oracle, rng, 2, g)
    A, B = [], []
    for i, p in enumerate(pts):
        for j, z in enumerate(zs):
            z2 = zs[(j + 1 + i) % len(zs)]
            A += [rs(oracle, p, z), rs(oracle, p, z), rs(oracle, p, z), rs(oracle, zero, z2), rs(oracle, p, z)]
            B += [rs(oracle, p, z2), rs(oracle, neg(p), z2), rs(oracle, zero, z2), rs(oracle, p, z),
                  rs(oracle, pts[(i + 1) % len(pts)], z2)]
    return np.stack(A), np.stack(B)


@pytest.mark.parametrize("g", [1, 2])
def test_group_addition_across_representations(oracle, eng, g):
    """bn254_g*_add_M with and without negate_b: equal points found across different z (h == 0 && sd == 0: jac_double_cold_vec on the
    GPU), opposite points across different z, infinity operands, generic sums - raw Jacobian limbs equal the reference's"""
    rng = np.random.default_rng(603 + g)
    A, B = _add_pairs(oracle, rng, g)
    add, neg = (oracle.g1_add, oracle.g1_neg) if g == 1 else (oracle.g2_add, oracle.g2_neg)
    run = eng.g1_add_batch if g == 1 else eng.g2_add_batch
    s, d = run(A, B), run(A, B, negate_b=True)
    for i in range(A.shape[0]):
        assert np.array_equal(s[i], add(A[i], B[i])), ("sum", i % 5, i)
        assert np.array_equal(d[i], add(A[i], neg(B[i]))), ("difference", i % 5, i)
    # the rows really reach the branches they are there for
    z = slice(8, None) if g == 1 else slice(16, None)
    assert not s[1::5][:, z].any() and not d[0::5][:, z].any()                                 # P + (-P), P - P: infinity
    assert np.array_equal(s[0], add(A[0], A[0]))                                                 # doubling: same limbs as A + A


def _pairing_values(oracle, eng, n):
    rng = np.random.default_rng(605)
    P = np.stack(_random_jacobian(oracle, rng, n, 1)); Q = np.stack(_random_jacobian(oracle, rng, n, 2))
    return eng.pairing_batch(P, Q)


def test_gt_pow_modes_on_crafted_scalars(oracle, eng):
    """bn254_gt_pow_B in modes 0 (Frobenius decomposition: the GLS split), 2 (one-dimensional cyclotomic) and 1 (general) on pairing
    values with the crafted scalars of both splits"""
    ks = E.crafted_gls_by_sign() + E.gls_crafted()[::8] + E.glv_crafted()[::16] + EDGE_SCALARS
    g = _pairing_values(oracle, eng, 8)
    a = np.stack([g[i % 8] for i in range(len(ks))]); a[3] = oracle.fq12_one()
    k = E.fr(oracle, ks)
    want = np.stack([oracle.gt_pow(a[i], k[i]) for i in range(len(ks))])
    try:
        for mode in (0, 2, 1):
            eng.set_option("gt_pow_mode", mode)
            got = eng.gt_pow_batch(a, k)
            bad = [i for i in range(len(ks)) if not np.array_equal(got[i], want[i])]
            assert not bad, (mode, bad[:8])
    finally:
        eng.set_option("gt_pow_mode", None)


ROUTES = (("wave", {"wave_pairing_max": 1 << 20, "wave_fe_max": 1 << 20}, "pairing_wave"),
          ("four-lane", {"wave_pairing_max": 0, "wave_fe_max": 0, "quad_max": 1 << 20}, "miller_quad"),
          ("lane-pair", {"wave_pairing_max": 0, "wave_fe_max": 0, "quad_max": 0}, "miller"))


def test_pairing_routes_on_edge_representations(oracle, eng):
    """pairing_batch through the wave, four-lane and lane-pair routes on edge-z G1 and G2 points (infinity with x, y != 0 included), the
    multi-pairing, and the native prepared table of an edge-z Q (bn254_g2_prepare) shared and per pair"""
    rng = np.random.default_rng(606)
    g1, g2 = _g1_edge_reps(oracle, rng), _g2_edge_reps(oracle, rng)
    n = max(len(g1), len(g2))
    P = np.stack([g1[i % len(g1)] for i in range(n)]); Q = np.stack([g2[(5 * i) % len(g2)] for i in range(n)])
    want = oracle.pairing_batch(P, Q)
    eng.profile(True)
    try:
        for name, opts, kernel in ROUTES:
            with eng.options(**opts):
                eng.profile_reset()
                got = eng.pairing_batch(P, Q)
                assert eng.kernel_stats(kernel)[1] >= 1, name
            bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
            assert not bad, (name, bad[:8])
    finally:
        eng.profile(False)
    assert np.array_equal(eng.pairing_product(P, Q), oracle.pairing_product(P, Q))
    for q in (g2[2], g2[len(E.FQ2_Z) + 5]):                        # G2 under z = (q-1, q-1), (r-1) G2 under (FE_LIMBS_MAX, 0)
        prep = eng.g2_prepare(q)
        with eng.options(wave_pairing_max=0):
            assert np.array_equal(eng.pairing_prepared_native_batch(P[:40], prep), oracle.pairing_batch(P[:40], np.tile(q, (40, 1))))
        prep.close()
    m = 48
    prep = eng.g2_prepare(Q[:m])
    with eng.options(wave_pairing_max=0):
        assert np.array_equal(eng.pairing_prepared_native_batch(P[:m], prep), want[:m])
        assert np.array_equal(eng.pairing_product_prepared_native(P[:m], prep), oracle.pairing_product(P[:m], Q[:m]))
    prep.close()


def test_encode_edge_representations(oracle, eng):
    """g1_encode_batch / g2_encode_batch (safegcd inversion of z) at the edge z values, infinity with x, y != 0 included"""
    rng = np.random.default_rng(607)
    P = np.stack(_g1_edge_reps(oracle, rng)); Q = np.stack(_g2_edge_reps(oracle, rng))
    e1, e2 = eng.g1_encode_batch(P), eng.g2_encode_batch(Q)
    for i in range(P.shape[0]):
        assert np.array_equal(e1[i], oracle.g1_encode(P[i])), i
    for i in range(Q.shape[0]):
        assert np.array_equal(e2[i], oracle.g2_encode(Q[i])), i


# ------------------------------------------------------------------------------------------------ launch seams
def _seam_inputs(te, g, n):
    """n distinct Jacobian points (the reference chain on the device, as bench.py builds them) and n distinct scalars"""
    import torch
    from bn_amd import distributed as D
    g1, g2 = D.generator_limbs()
    kb = D.synthetic_scalars_device(te, 0, n, g - 1)
    base = te.empty(n, 12 if g == 1 else 24)
    te.e.tile_dev(_dev(te, g1 if g == 1 else g2).data_ptr(), 96 if g == 1 else 192, n, base.data_ptr(), te._stream())
    P = (te.g1_mul if g == 1 else te.g2_mul)(base, kb, normalize=False)
    k = D.synthetic_scalars_device(te, 1 << 24, (1 << 24) + n, 1)
    torch.cuda.synchronize()
    return P, k


@pytest.mark.parametrize("g", [1, 2])
def test_mul_launch_seams(oracle, te, g):
    """bn_mul_dev cuts a normalizing call into launches of 2^20 G1 (2^19 G2) points that reuse ONE context-owned window table in stream
    order: batches just above (and, for G2, just below) that size against the same inputs in separate calls below it, element for
    element, and against the oracle at the seam and on a random sample"""
    import torch
    step = (1 << 20) if g == 1 else (1 << 19)
    sizes = [step + 1, step + 4097] if g == 1 else [step - 1, step + 1, step + 4097]
    nmax = max(sizes)
    P, k = _seam_inputs(te, g, nmax)
    mul = te.g1_mul if g == 1 else te.g2_mul
    ref = torch.cat([mul(P[lo:lo + step // 2], k[lo:lo + step // 2]) for lo in range(0, nmax, step // 2)])   # calls of half a launch
    torch.cuda.synchronize()
    Pn, kn = _host(P), _host(k)
    rng = np.random.default_rng(608 + g)
    for n in sizes:
        out = mul(P[:n], k[:n])
        torch.cuda.synchronize()
        assert torch.equal(out, ref[:n]), n
        idx = sorted({i for i in (0, 1, step - 1, step, step + 1, n - 1) if i < n} | set(rng.choice(n, 1024, replace=False).tolist()))
        want = canon_infinity((oracle.g1_mul_batch if g == 1 else oracle.g2_mul_batch)(Pn[idx], kn[idx]))
        assert np.array_equal(_host(out)[idx], want), n


def test_sub_launches_with_small_rounds(oracle, eng):
    """BN254_OPT_ROUND_PAIRS = 96: Gt::pow at ragged sizes runs as several sub-launches of (nearly) one round plus a short tail, reusing
    one window table - element for element equal to the default single launch.  The scalar multiplications are cut by their own launch
    size, not by the round: the same option leaves them as they are (checked at ragged n as well)"""
    rng = np.random.default_rng(609)
    g = _pairing_values(oracle, eng, 16)
    n = 1000
    a = np.stack([g[i % 16] for i in range(n)])
    ks = E.gls_crafted() + E.glv_crafted()
    k = E.fr(oracle, [ks[i % len(ks)] for i in range(n)])
    P1 = np.stack(_random_jacobian(oracle, rng, 8, 1) * 125)[:n - 3]; P2 = np.stack(_random_jacobian(oracle, rng, 8, 2) * 125)[:n - 5]
    base = {}
    try:
        for mode in (0, 2, 1):
            eng.set_option("gt_pow_mode", mode)
            base[mode] = eng.gt_pow_batch(a, k)
        m1, m2 = eng.g1_mul_batch(P1, k[:n - 3]), eng.g2_mul_batch(P2, k[:n - 5])
        with eng.options(round_pairs=96):
            for mode in (0, 2, 1):
                eng.set_option("gt_pow_mode", mode)
                for m in (n, 97, 95, 193):
                    assert np.array_equal(eng.gt_pow_batch(a[:m], k[:m]), base[mode][:m]), (mode, m)
            assert np.array_equal(eng.g1_mul_batch(P1, k[:n - 3]), m1) and np.array_equal(eng.g2_mul_batch(P2, k[:n - 5]), m2)
    finally:
        eng.set_option("gt_pow_mode", None)
    for i in rng.choice(n, 24, replace=False):
        assert np.array_equal(base[0][i], oracle.gt_pow(a[i], k[i])), i


# ------------------------------------------------------------------------------------------------ wire limits
def test_decoders_at_the_modulus_limits(oracle, eng):
    """the batch decoders on coordinates at the exact limits - x or y = q - 1 (on the curve: the largest-x point, y = q - 1 on the point
    with y^2 = 1) against = q and the generator shifted by q; G2 coordinates q^2 - 1 (c1 = c0 = q - 1) against q^2 and a valid point
    with a coordinate + q^2; Fr 0, 1, r - 2 and r - 1 against r, r + 1 and 2^256 - 1 - record by record, status and output equal to the oracle's"""
    Q, R = M.Q, M.R_ORD
    (xe, ye), (xe2, ye2) = E.edge_g1_affine()[2:]
    (x1, _), _ = E.g1_points_with_y_one()
    g1 = [E.g1_record(xe, ye), E.g1_record(xe2, ye2), E.g1_record(x1, 1), E.g1_record(x1, Q - 1), E.g1_record(Q - 1, Q - 1),
          E.g1_record(Q, ye), E.g1_record(xe, Q), E.g1_record(Q + 1, 2), E.g1_record(1, Q + 2), E.g1_record(1, Q - 2),
          E.g1_record(Q - 1, Q), E.g1_record(Q, Q), E.g1_record(0, 0, tag=0), E.g1_record(Q, Q, tag=0)]
    d1, s1 = eng.g1_decode_batch(np.stack(g1))
    for i, rec in enumerate(g1):
        rc, want = oracle.g1_decode(rec)
        assert s1[i] == rc and np.array_equal(d1[i], want if rc == 0 else oracle.g1_zero()), (i, s1[i], rc)
    assert list(s1[:4]) == [0, 0, 0, 0] and list(s1[5:9]) == [1, 1, 1, 1] and s1[9] == 0
    q2 = Q * Q
    gq = E.g2_ints(oracle, oracle.g2_normalize(E.edge_g2_points(oracle)[2]))
    gx, gy = E.fq2_packed(gq[0]), E.fq2_packed(gq[1])
    g2 = [E.g2_record(gx, gy), E.g2_record(q2 - 1, gy), E.g2_record(gx, q2 - 1), E.g2_record(q2, gy), E.g2_record(gx, q2),
          E.g2_record(gx + q2, gy), E.g2_record(gx, gy + q2), E.g2_record((Q - 1) * Q + (Q - 1), q2 - 1), E.g2_record(q2 + Q - 1, gy),
          E.g2_record(Q * Q - Q, gy), E.g2_record(q2, q2, tag=0)]
    d2, s2 = eng.g2_decode_batch(np.stack(g2))
    for i, rec in enumerate(g2):
        rc, want = oracle.g2_decode(rec)
        assert s2[i] == rc and np.array_equal(d2[i], want if rc == 0 else oracle.g2_zero()), (i, s2[i], rc)
    assert s2[0] == 0 and list(s2[3:7]) == [2, 2, 2, 2] and s2[1] != 2 and s2[2] != 2
    fr = [R - 1, R, R + 1, (1 << 256) - 1, 0, R - 2, 1]
    b = np.stack([np.frombuffer(v.to_bytes(32, "big"), np.uint8) for v in fr])
    dk, sk = eng.fr_decode_batch(b)
    for i in range(len(fr)):
        rc, want = oracle.fr_decode(b[i])
        assert sk[i] == rc and np.array_equal(dk[i], want), (i, sk[i], rc)
    assert list(sk) == [0, 1, 1, 1, 0, 0, 0] and np.array_equal(dk[0], oracle.fp_from_int(FR, R - 1))
