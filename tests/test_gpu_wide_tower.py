"""GPU parity of the lane-pair kernels whose Fq12 products and squarings run on lazily reduced Fq6 products (tower.hpp f6_mul_lazy: wide dual
products, one Montgomery reduction per coefficient - the asm leaves of fe_asm.hpp that the CPU twins of tests/test_hostsim_wide.py stand in
for).  Run with -m gpu on an MI355X.  The lane-pair kernels are forced at small n (wave_pairing_max = wave_fe_max = quad_max = 0) and the
kernel statistics say that they ran: n = 1, 2, 3 (one wave with dead lanes), 65 (two waves, ragged) and 130.  Every list is followed by its
rotation by one, so each element sits once on an even and once on an odd slot.  Every comparison is bit for bit against the oracle."""
import numpy as np
import pytest

import edge_inputs as E
from bn_oracle import FR

pytestmark = pytest.mark.gpu

LANE_PAIR = {"wave_pairing_max": 0, "wave_fe_max": 0, "quad_max": 0}
SIZES = (1, 2, 3, 65, 130)


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def te(eng):
    import torch
    from bn_amd import distributed as D
    return D.TorchEngine(eng, torch.device("cuda", 0))


def _dev(te, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).to(te.device)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _slots(vals, n=130):
    """the list, its rotation by one, then the list again, cut to n: element i at slot i and at slot len + (i - 1) % len.  The length is even
    (64 here), so the two slots of every element differ in parity, and both lie below 2 len <= n"""
    vals = list(vals)
    L = len(vals)
    assert L % 2 == 0 and 2 * L <= n
    out = (vals + vals[1:] + vals[:1] + vals)[:n]
    for i in range(L):
        second = L + (i - 1) % L
        assert out[i] is vals[i] and out[second] is vals[i] and (i + second) % 2 == 1, i
    return np.stack(out)


def _bad(got, want):
    return [i for i in range(got.shape[0]) if not np.array_equal(got[i], want[i])][:8]


@pytest.fixture(scope="module")
def sets(oracle):
    """inputs and oracle references, computed once, shared and read-only"""
    rng = np.random.default_rng(2301)
    m = 64                                               # an even length: see _slots
    ks = [oracle.fp_from_int(FR, int.from_bytes(rng.bytes(40), "little") % E.R) for _ in range(2 * m)]
    P = oracle.g1_mul_batch_jacobian(np.tile(oracle.g1_one(), (m, 1)), np.stack(ks[:m]))
    Q = oracle.g2_mul_batch_jacobian(np.tile(oracle.g2_one(), (m, 1)), np.stack(ks[m:]))
    P[3] = oracle.g1_zero(); Q[5] = oracle.g2_zero(); P[8] = oracle.g1_zero(); Q[8] = oracle.g2_zero()      # infinity on either side, and on both
    e = oracle.pairing_batch(P, Q)
    s = {"P": _slots(P), "Q": _slots(Q), "pairing": _slots(e)}
    # infinity on one side sits on an odd and on an even slot (P[3]: 3 and 66, Q[5]: 5 and 68), on both sides likewise (8 and 71)
    assert all(np.array_equal(s["P"][i], oracle.g1_zero()) for i in (3, 66, 8, 71)) and all(np.array_equal(s["Q"][i], oracle.g2_zero()) for i in (5, 68, 8, 71))
    edge, cyc, gt = list(E.edge_fq12(oracle).values()), E.edge_cyclotomic(oracle), E.edge_gt(oracle)
    s["edge"], s["cyc"], s["gt"] = _slots(edge), _slots(cyc), _slots(gt)
    s["fe_edge"] = s["gt"]
    s["fe_cyc"] = _slots([oracle.fq12_final_exponentiation(a) for a in cyc])
    s["fe_gt"] = _slots([oracle.fq12_final_exponentiation(a) for a in gt])
    partners = [edge[j] for j in E.edge_partners(len(edge))]
    s["partner"] = _slots(partners)
    s["mul"] = _slots([oracle.fq12_mul(a, b) for a, b in zip(edge, partners)])
    kk = E.GT_EDGE_SCALARS + E.crafted_gls_by_sign()
    k = E.fr(oracle, [kk[i % len(kk)] for i in range(len(gt))])
    s["k"] = _slots(k)
    s["pow"] = _slots([oracle.gt_pow(a, ki) for a, ki in zip(gt, k)])
    for v in s.values():
        v.setflags(write=False)
    return s


def test_pairing_batch_on_the_lane_pair_kernels(oracle, eng, sets):
    one = oracle.fq12_one()
    assert all(np.array_equal(sets["pairing"][i], one) for i in (3, 5, 8, 66, 68, 71))
    eng.profile(True)
    try:
        with eng.options(**LANE_PAIR):
            for n in SIZES:
                eng.profile_reset()
                got = eng.pairing_batch(sets["P"][:n], sets["Q"][:n])
                assert eng.kernel_stats("miller")[1] >= 1 and eng.kernel_stats("final_exp")[1] >= 1, n
                assert eng.kernel_stats("miller_quad")[1] == 0 and eng.kernel_stats("pairing_wave")[1] == 0, n
                assert not _bad(got, sets["pairing"][:n]), (n, _bad(got, sets["pairing"][:n]))
    finally:
        eng.profile(False)


@pytest.mark.parametrize("kind", ["edge", "cyc", "gt"])
def test_final_exponentiation_on_the_lane_pair_kernel(eng, te, sets, kind):
    src_all, want = sets[kind], sets["fe_" + kind]
    eng.profile(True)
    try:
        with eng.options(**LANE_PAIR):
            for n in SIZES:
                eng.profile_reset()
                src = _dev(te, src_all[:n]); out = te.empty(n, 48)
                eng.final_exp_batch_dev(src.data_ptr(), out.data_ptr(), n, te._stream())
                got = _host(out)
                assert eng.kernel_stats("final_exp")[1] >= 1 and eng.kernel_stats("final_exp_wave")[1] == 0 and eng.kernel_stats("final_exp_quad")[1] == 0, (kind, n)
                assert not _bad(got, want[:n]), (kind, n, "out of place", _bad(got, want[:n]))
                assert np.array_equal(_host(src), src_all[:n]), (kind, n, "the input was written")
                eng.final_exp_batch_dev(src.data_ptr(), src.data_ptr(), n, te._stream())
                assert not _bad(_host(src), want[:n]), (kind, n, "in place")
    finally:
        eng.profile(False)


def test_gt_mul_on_edge_elements(eng, te, sets):
    with eng.options(**LANE_PAIR):
        for n in SIZES:
            a, b, out = _dev(te, sets["edge"][:n]), _dev(te, sets["partner"][:n]), te.empty(n, 48)
            eng.gt_mul_dev(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, te._stream())
            assert not _bad(_host(out), sets["mul"][:n]), (n, "out of place")
            assert np.array_equal(_host(a), sets["edge"][:n]) and np.array_equal(_host(b), sets["partner"][:n]), (n, "an input was written")
            eng.gt_mul_dev(a.data_ptr(), b.data_ptr(), a.data_ptr(), n, te._stream())
            assert not _bad(_host(a), sets["mul"][:n]), (n, "in place, left")
            a = _dev(te, sets["edge"][:n])
            eng.gt_mul_dev(a.data_ptr(), b.data_ptr(), b.data_ptr(), n, te._stream())
            assert not _bad(_host(b), sets["mul"][:n]), (n, "in place, right")
            assert np.array_equal(eng.gt_mul_batch(sets["edge"][:n], sets["partner"][:n]), sets["mul"][:n]), (n, "host arrays")


def test_gt_pow_on_order_r_elements(eng, te, sets):
    with eng.options(**LANE_PAIR):
        for n in SIZES:
            a, k, out = _dev(te, sets["gt"][:n]), _dev(te, sets["k"][:n]), te.empty(n, 48)
            eng.gt_pow_dev(a.data_ptr(), k.data_ptr(), out.data_ptr(), n, te._stream())
            assert not _bad(_host(out), sets["pow"][:n]), (n, "out of place")
            assert np.array_equal(_host(a), sets["gt"][:n]), (n, "the input was written")
            eng.gt_pow_dev(a.data_ptr(), k.data_ptr(), a.data_ptr(), n, te._stream())
            assert not _bad(_host(a), sets["pow"][:n]), (n, "in place")
