"""The batched multi-pairing over prepared G2 points on an MI355X (run with -m gpu): bn254_pairing_product_batch_prepared_native and its _dev /
Python / C++ faces, bit for bit against the oracle (segment j = the oracle's pairings of its pairs folded with fq12_mul: the final
exponentiation is a homomorphism), against bn254_pairing_product_batch on the gathered points and against the one-product prepared entry
point; on every route - the segmented native Miller kernel writing straight to the outputs (no segment above four pairs), the same kernel in
front of the segmented fold, sub-launch and chunk seams, the small route through the general kernels - and inside groth16.verify_batch."""
import ctypes as C

import numpy as np
import pytest

import edge_inputs as E

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 300]
KEY_EXTRA = 20            # further P per key point (the first three G2 points): what pairs 1-3 of a Groth16-shaped check draw from
ONE = np.zeros(48, np.uint64); ONE[:4] = [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]
SCOPES = ("miller_native_seg", "g2_gather", "gt_segment", "gt_tail_seg", "miller_wave", "miller_quad", "miller", "pairing_wave", "miller_native_shared",
          "final_exp_wave", "final_exp_quad", "final_exp")


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def pool(oracle):
    """(P, G2S, hq, B): unique pairs (P[u], G2S[hq[u]]) and their pairings B[u].  G2S: ~170 distinct G2 points - random Jacobian points (z != 1),
    edge representations of edge points, points at infinity; P likewise, with points at infinity.  The first three G2 points (the "key") meet
    KEY_EXTRA more P each.  Batches index into the pairs, so the expected values cost one oracle pairing per unique pair."""
    rng = np.random.default_rng(2025)
    n = 150
    k = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(2 * n + 3 * KEY_EXTRA)])
    P = list(oracle.g1_mul_batch_jacobian(np.tile(oracle.g1_one(), (n, 1)), k[:n]))
    G2S = list(oracle.g2_mul_batch_jacobian(np.tile(oracle.g2_one(), (n, 1)), k[n:2 * n]))
    hq = list(range(n))
    g1e = [E.rescale_g1(oracle, p, z) for p in E.edge_g1_points(oracle) for z in E.FQ_Z[:4]]
    g2e = [E.rescale_g2(oracle, q, z) for q in E.edge_g2_points(oracle) for z in E.FQ2_Z[:4]]
    for i, p in enumerate(g1e):
        P.append(p); hq.append(i)
    for i, q in enumerate(g2e):
        P.append(P[i]); hq.append(len(G2S)); G2S.append(q)
    for i in range(4):
        P.append(oracle.g1_zero()); hq.append(i)
        P.append(P[i]); hq.append(len(G2S)); G2S.append(oracle.g2_zero())
    extra = oracle.g1_mul_batch_jacobian(np.tile(oracle.g1_one(), (3 * KEY_EXTRA, 1)), k[2 * n:])
    key_pairs = {}
    for kk in range(3):
        key_pairs[kk] = list(range(len(P), len(P) + KEY_EXTRA))
        for x in extra[kk * KEY_EXTRA:(kk + 1) * KEY_EXTRA]:
            P.append(x); hq.append(kk)
    P, G2S, hq = np.stack(P), np.stack(G2S), np.array(hq)
    return {"P": P, "G2S": G2S, "hq": hq, "B": oracle.pairing_batch(P, G2S[hq]), "key_pairs": key_pairs}


@pytest.fixture(scope="module")
def handle(eng, pool):
    """the distinct G2 points in a shuffled order behind ONE handle; pos[g] = where point g of G2S sits"""
    rng = np.random.default_rng(77)
    perm = rng.permutation(pool["G2S"].shape[0])
    pos = np.empty_like(perm); pos[perm] = np.arange(perm.size)
    h = eng.g2_prepare(pool["G2S"][perm])
    assert h.count == perm.size
    yield h, pos
    h.close()


def _segments(rng, pool, lengths):
    offs = np.zeros(len(lengths) + 1, np.uint64)
    offs[1:] = np.cumsum(lengths)
    idx = rng.integers(0, pool["P"].shape[0], int(offs[-1]))
    return offs, idx


def _want(oracle, pool, offs, idx, segs=None):
    B = pool["B"]
    out = []
    for j in (range(len(offs) - 1) if segs is None else segs):
        acc = oracle.fq12_one()
        for i in idx[int(offs[j]):int(offs[j + 1])]:
            acc = oracle.fq12_mul(acc, B[i])
        out.append(acc)
    return np.stack(out)


def _stats(eng):
    return {k: eng.kernel_stats(k)[1] for k in SCOPES}


def _run(eng, P, h, offs, qi, **opts):
    eng.profile(True); eng.profile_reset()
    try:
        with eng.options(**opts):
            got = eng.pairing_product_batch_prepared_native(P, h, offs, qi)
        return got, _stats(eng)
    finally:
        eng.profile(False)


def test_ragged_segments_against_the_oracle(oracle, eng, pool, handle):
    """segments with lengths from {0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 300}, random indices into a handle of ~170 points (edge representations,
    points at infinity; P at infinity among the pairs): every output byte-equal to the oracle's fold, to Engine.pairing_product_batch on the
    gathered points and, per segment, to pairing_product_prepared_native; on the native route and with the default thresholds"""
    h, pos = handle
    rng = np.random.default_rng(11)
    lengths = [int(x) for x in rng.choice(LENGTHS, 70)] + LENGTHS + [0, 300, 0, 1]
    offs, idx = _segments(rng, pool, lengths)
    P, qi = pool["P"][idx], pos[pool["hq"][idx]]
    want = _want(oracle, pool, offs, idx)
    got, st = _run(eng, P, h, offs, qi, wave_pairing_max=0)
    assert got.shape == (len(lengths), 48)
    bad = [j for j in range(len(lengths)) if not np.array_equal(got[j], want[j])]
    assert not bad, (bad[:10], [lengths[j] for j in bad[:10]])
    assert st["miller_native_seg"] >= 1 and st["gt_segment"] >= 1 and st["miller"] == 0 and st["miller_wave"] == 0, st
    got2, _ = _run(eng, P, h, offs, qi)
    assert np.array_equal(got2, want)
    assert np.array_equal(eng.pairing_product_batch(P, pool["G2S"][pool["hq"][idx]], offs), want)
    one_point = eng.g2_prepare(pool["G2S"][0])
    for j, L in enumerate(lengths):
        a, b = int(offs[j]), int(offs[j + 1])
        if L == 0:
            assert np.array_equal(eng.pairing_product_prepared_native(P[:0], one_point), got[j]), j
            continue
        hj = eng.g2_prepare(pool["G2S"][pool["hq"][idx[a:b]]])
        try:
            assert np.array_equal(eng.pairing_product_prepared_native(P[a:b], hj), got[j]), (j, L)
        finally:
            hj.close()
    one_point.close()


def _groth_block(rng, pool, m):
    """m checks of four pairs in the Groth16 layout: a handle [K0, K1, K2, B_0 .. B_{m-1}], check j = indices [3 + j, 0, 1, 2].
    Returns the handle's points, P, q_index, offsets and the pool pair behind every pair (for the expected values)."""
    hq = pool["hq"]
    b = rng.integers(0, hq.size, m)
    idx = np.empty((m, 4), np.int64)
    idx[:, 0] = b
    for kk in range(3):
        idx[:, 1 + kk] = rng.choice(pool["key_pairs"][kk], m)
    Q = np.concatenate([pool["G2S"][:3], pool["G2S"][hq[b]]])
    qi = np.empty((m, 4), np.uint64)
    qi[:, 0] = 3 + np.arange(m); qi[:, 1:] = np.arange(3)
    idx = idx.reshape(-1)
    return Q, pool["P"][idx], qi.reshape(-1), np.arange(m + 1, dtype=np.uint64) * 4, idx


def test_groth16_shape_writes_straight_to_the_outputs(oracle, eng, pool):
    """all segments four pairs, indices [3 + j, 0, 1, 2]: the Miller kernel's values are the segments' - no fold launch at all"""
    rng = np.random.default_rng(12)
    m = 5000
    Q, P, qi, offs, idx = _groth_block(rng, pool, m)
    h = eng.g2_prepare(Q)
    try:
        got, st = _run(eng, P, h, offs, qi)
        assert st["miller_native_seg"] >= 1 and st["gt_segment"] == 0 and st["gt_tail_seg"] == 0 and st["miller"] == 0, st
        sample = sorted(set(rng.integers(0, m, 300).tolist()) | {0, m - 1})
        assert np.array_equal(got[sample], _want(oracle, pool, offs, idx, sample))
        assert np.array_equal(got, eng.pairing_product_batch(P, Q[qi.astype(np.int64)], offs))
    finally:
        h.close()


def test_many_four_pair_checks(oracle, eng, pool):
    """m = 2^16 checks of 4 pairs over a handle of 2^16 + 3 points: 2048 segments spread over the batch, the last included, against the oracle"""
    rng = np.random.default_rng(13)
    m = 1 << 16
    Q, P, qi, offs, idx = _groth_block(rng, pool, m)
    h = eng.g2_prepare(Q)
    try:
        got, st = _run(eng, P, h, offs, qi)
        assert st["miller_native_seg"] >= 1 and st["gt_segment"] == 0, st
        sample = sorted(set(np.linspace(0, m - 1, 2048).astype(int).tolist()))
        assert sample[-1] == m - 1
        assert np.array_equal(got[sample], _want(oracle, pool, offs, idx, sample))
    finally:
        h.close()


def test_routes_give_the_same_bytes(oracle, eng, pool, handle):
    """a handful of checks: the small route (general kernels on the gathered points, no native Miller launch), the same call with
    BN254_OPT_WAVE_PAIRING_MAX = 0 (native route) - each proven by its profile scope"""
    h, pos = handle
    rng = np.random.default_rng(14)
    lengths = [int(x) for x in rng.choice([0, 1, 2, 3, 4, 5, 16], 40)]
    offs, idx = _segments(rng, pool, lengths)
    P, qi = pool["P"][idx], pos[pool["hq"][idx]]
    want = _want(oracle, pool, offs, idx)
    got, st = _run(eng, P, h, offs, qi)
    assert np.array_equal(got, want)
    assert st["miller_native_seg"] == 0 and st["g2_gather"] == 1 and st["miller_wave"] == 1 and st["gt_tail_seg"] == 1, st
    got, st = _run(eng, P, h, offs, qi, wave_pairing_max=0)
    assert np.array_equal(got, want)
    assert st["miller_native_seg"] >= 1 and st["g2_gather"] == 0 and st["miller_wave"] == 0 and st["gt_segment"] >= 1, st
    # eight checks of four pairs: small route, and the native kernel writing the outputs itself
    offs, idx = _segments(rng, pool, [4] * 8)
    P, qi = pool["P"][idx], pos[pool["hq"][idx]]
    want = _want(oracle, pool, offs, idx)
    got, st = _run(eng, P, h, offs, qi)
    assert np.array_equal(got, want) and st["miller_native_seg"] == 0, st
    got, st = _run(eng, P, h, offs, qi, wave_pairing_max=0)
    assert np.array_equal(got, want) and st["miller_native_seg"] == 1 and st["gt_segment"] == 0, st


def test_segments_across_sub_launch_seams(oracle, eng, pool, handle):
    """one machine round cut down to 64 (BN254_OPT_ROUND_PAIRS): 200 short segments go out in four sub-launches of pieces; segments of 300, 129,
    70 ... pairs give 164 pieces in three chunks of values, their partial products carried across the cuts"""
    h, pos = handle
    rng = np.random.default_rng(15)
    lengths = [int(x) for x in rng.choice([0, 1, 2, 3, 4], 200)]
    offs, idx = _segments(rng, pool, lengths)
    P, qi = pool["P"][idx], pos[pool["hq"][idx]]
    got, st = _run(eng, P, h, offs, qi, round_pairs=64, wave_pairing_max=0)
    assert np.array_equal(got, _want(oracle, pool, offs, idx))
    assert st["miller_native_seg"] == 4 and st["gt_segment"] == 0, st
    lengths = [300, 5, 0, 70, 1, 64, 65, 3, 0, 129, 2, 0]
    offs, idx = _segments(rng, pool, lengths)
    P, qi = pool["P"][idx], pos[pool["hq"][idx]]
    got, st = _run(eng, P, h, offs, qi, round_pairs=64, wave_pairing_max=0)
    assert np.array_equal(got, _want(oracle, pool, offs, idx))
    assert sum(-(-L // 4) for L in lengths) == 164 and st["miller_native_seg"] >= 3 and st["gt_segment"] >= 3, st


def test_one_long_segment_between_empty_ones(oracle, eng, pool, handle):
    """5000 pairs = 1250 pieces in ONE Miller launch, folded in ceil(log16 1250) = 3 levels; the empty segments give one"""
    h, pos = handle
    rng = np.random.default_rng(16)
    lengths = [0] * 1000 + [5000] + [0] * 1000
    offs, idx = _segments(rng, pool, lengths)
    P, qi = pool["P"][idx], pos[pool["hq"][idx]]
    got, st = _run(eng, P, h, offs, qi)
    assert st["miller_native_seg"] == 1 and st["gt_segment"] == 3 and st["miller"] == 0, st
    assert (got[:1000] == ONE).all() and (got[1001:] == ONE).all()
    assert np.array_equal(got[1000], _want(oracle, pool, offs, idx, [1000])[0])
    assert np.array_equal(got[1000], eng.pairing_product(P, pool["G2S"][pool["hq"][idx]]))


def test_index_conventions_and_errors(oracle, eng, pool, handle):
    """q_index = None on a one-point and on a many-point handle; an index repeated inside a segment; an index == count: -2 and `out` untouched
    from host buffers, the factor one from device buffers (the documented memory-safe mapping to the identity record)"""
    import torch
    h, pos = handle
    n = h.count
    G2S, hq, Pp = pool["G2S"], pool["hq"], pool["P"]
    for opts in ({}, {"wave_pairing_max": 0}):
        # one point: every pair against it
        kp = pool["key_pairs"][0]
        sel = np.array(kp[:11])
        one_point = eng.g2_prepare(G2S[0])
        offs = np.array([0, 4, 4, 5, 11], np.uint64)
        got, _ = _run(eng, Pp[sel], one_point, offs, None, **opts)
        assert np.array_equal(got, _want(oracle, pool, offs, sel))
        got, _ = _run(eng, Pp[sel], one_point, offs, np.zeros(11, np.uint64), **opts)
        assert np.array_equal(got, _want(oracle, pool, offs, sel))
        one_point.close()
        # many points, no indices: pair i against point i
        first = np.array([int(np.flatnonzero(hq == g)[0]) for g in np.argsort(pos)])           # a pool pair for every position of the handle
        offs = np.array([0, 3, 3, 20, 21, n], np.uint64)
        got, _ = _run(eng, Pp[first], h, offs, None, **opts)
        assert np.array_equal(got, _want(oracle, pool, offs, first))
        # one index three times in a segment (and the same pool pair twice)
        u = int(pool["key_pairs"][1][0])
        sel = np.array([u, 5, u, pool["key_pairs"][1][1], 7])
        offs = np.array([0, 5], np.uint64)
        got, _ = _run(eng, Pp[sel], h, offs, pos[hq[sel]], **opts)
        assert np.array_equal(got, _want(oracle, pool, offs, sel))
    # host buffers: an index == count is an error, before anything is written
    sel = np.arange(6)
    qi = pos[hq[sel]].astype(np.uint64); qi[4] = n
    P = np.ascontiguousarray(Pp[sel]); offs = np.array([0, 2, 6], np.uint64)
    out = np.full((2, 48), 7, np.uint64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    assert eng._lib.bn254_pairing_product_batch_prepared_native(eng._h, vp(P), h._h, vp(qi), vp(offs), 2, vp(out)) == -2
    assert (out == 7).all()
    toomany = np.ascontiguousarray(np.tile(Pp[:1], (n + 1, 1))); offs2 = np.array([0, n + 1], np.uint64)
    assert eng._lib.bn254_pairing_product_batch_prepared_native(eng._h, vp(toomany), h._h, None, vp(offs2), 1, vp(out)) == -2
    assert (out == 7).all()
    # device buffers: the same index gives the factor one (native route and small route)
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(P.view(np.int64)).to(dev)
    dqi = torch.from_numpy(qi.view(np.int64)).to(dev)
    keep = np.array([0, 1, 2, 3, 5])
    offs_keep = np.array([0, 2, 5], np.uint64)
    want = _want(oracle, pool, offs_keep, sel[keep])
    for opts in ({}, {"wave_pairing_max": 0}):
        dout = torch.zeros((2, 48), dtype=torch.int64, device=dev)
        with eng.options(**opts):
            eng.pairing_product_batch_prepared_native_dev(dp.data_ptr(), h, offs, dout.data_ptr(), dqi.data_ptr())
        torch.cuda.synchronize(dev)
        assert np.array_equal(dout.cpu().numpy().view(np.uint64), want), opts


def test_device_entry_on_a_side_stream(eng, pool, handle):
    import torch
    h, pos = handle
    rng = np.random.default_rng(17)
    for lengths in ([int(x) for x in rng.choice(LENGTHS, 30)], [int(x) for x in rng.choice(LENGTHS, 60)] + [300] * 8):
        offs, idx = _segments(rng, pool, lengths)
        P, qi = np.ascontiguousarray(pool["P"][idx]), np.ascontiguousarray(pos[pool["hq"][idx]].astype(np.uint64))
        dev = torch.device("cuda", 0)
        dp = torch.from_numpy(P.view(np.int64)).to(dev)
        dqi = torch.from_numpy(qi.view(np.int64)).to(dev)
        out = torch.zeros((len(lengths), 48), dtype=torch.int64, device=dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            eng.pairing_product_batch_prepared_native_dev(dp.data_ptr(), h, [int(x) for x in offs], out.data_ptr(), dqi.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), eng.pairing_product_batch(P, pool["G2S"][pool["hq"][idx]], offs))


def test_python_api(oracle, eng, pool):
    """bn_amd.PreparedG2.pairing_product_batch / pairing_check_batch: (G1, index) segments and the array form"""
    import bn_amd
    from bn_amd.api import R_MOD
    from bn_oracle import FR
    P, Q = oracle.g1_one(), oracle.g2_one()
    a, b = 12345678901234567890, 98765432109876543210
    fr = lambda v: oracle.fp_from_int(FR, v % R_MOD)
    aP, bQ, abP, abP1 = oracle.g1_mul(P, fr(a)), oracle.g2_mul(Q, fr(b)), oracle.g1_mul(P, fr(a * b)), oracle.g1_mul(P, fr(a * b + 1))
    prep = bn_amd.PreparedG2(np.stack([Q, bQ]), engine=eng)
    G1 = bn_amd.G1
    segs = [[(G1(aP), 1), (G1(oracle.g1_neg(abP)), 0)], [], [(G1(P), 0)], [(G1(aP), 1), (G1(oracle.g1_neg(abP1)), 0)]]
    res = prep.pairing_product_batch(segs)
    assert res[0] == bn_amd.Gt.one() and res[1] == bn_amd.Gt.one() and np.array_equal(res[2].limbs, oracle.pairing_batch(P, Q)[0])
    assert prep.pairing_check_batch(segs).tolist() == [True, True, False, False]
    ps = np.stack([aP, oracle.g1_neg(abP), P, oracle.g1_neg(P)])
    assert prep.pairing_check_batch(ps, q_index=[1, 0, 0, 0], offsets=[0, 2, 4, 4]).tolist() == [True, True, True]
    with pytest.raises(ValueError):
        prep.pairing_product_batch([[(G1(P), 2)]])
    prep.close()


def test_cpp_host_product_batch_prepared(oracle, tmp_path):
    """a compiled host program (g++ on include/bn254.hpp): bn::PreparedG2::pairing_product_batch and pairing_check_batch"""
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parents[1]
    src = tmp_path / "host.cpp"
    src.write_text(r'''
#include "bn254.hpp"
#include <cstdio>
template <class T> void dump(const T &t) { const uint64_t *w = reinterpret_cast<const uint64_t *>(&t); for (size_t i = 0; i < sizeof(T) / 8; ++i) std::printf("%llu ", (unsigned long long)w[i]); std::printf("\n"); }
int main() {
    using namespace bn;
    std::vector<G1> p; std::vector<G2> q;
    G1 a = G1::one(); G2 b = G2::one();
    for (int i = 0; i < 5; ++i) { p.push_back(a); q.push_back(b); a = a + G1::one(); b = b + b; }      // (i+1) G1, 2^i G2: Jacobian z != 1
    p[3] = G1::zero();
    PreparedG2 prep(q);
    for (auto &g : prep.pairing_product_batch(p, {4, 0, 2, 3, 1}, {0, 2, 2, 5})) dump(g);
    for (auto &g : prep.pairing_product_batch(p, {}, {0, 5})) dump(g);
    std::vector<G1> cp = {G1::one(), -G1::one(), G1::one(), G1::one()};
    for (bool ok : prep.pairing_check_batch(cp, {1, 1, 0, 0}, {0, 2, 4, 4})) std::printf("%d\n", ok ? 1 : 0);
    return 0;
}
''')
    exe = tmp_path / "host"
    subprocess.check_call(["g++", "-std=c++17", "-I", str(root / "include"), str(src), "-o", str(exe),
                           "-L", str(root / "bn_amd"), "-lbn254_hip", "-Wl,-rpath," + str(root / "bn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lines = subprocess.check_output([str(exe)], timeout=600).decode().strip().split("\n")
    got = [np.array([int(x) for x in l.split()], np.uint64) for l in lines[:4]]
    P = np.stack([oracle.g1_one()] * 5); Q = np.stack([oracle.g2_one()] * 5)
    for i in range(1, 5):
        P[i] = oracle.g1_add(P[i - 1], oracle.g1_one()); Q[i] = oracle.g2_add(Q[i - 1], Q[i - 1])
    P[3] = oracle.g1_zero()
    qi = [4, 0, 2, 3, 1]
    B = oracle.pairing_batch(P, Q[qi])
    assert np.array_equal(got[0], oracle.fq12_mul(B[0], B[1]))
    assert np.array_equal(got[1], oracle.fq12_one())
    assert np.array_equal(got[2], oracle.fq12_mul(oracle.fq12_mul(B[2], B[3]), B[4]))
    D = oracle.pairing_batch(P, Q)
    acc = oracle.fq12_one()
    for i in range(5):
        acc = oracle.fq12_mul(acc, D[i])
    assert np.array_equal(got[3], acc)
    assert [l.strip() for l in lines[4:7]] == ["1", "0", "1"]


def test_groth16_prepared_equals_the_general_path():
    """groth16.verify_batch(..., prepared=True) == verify_batch(...) on a block with valid proofs, a wrong public input, a wrong C and B at
    infinity (which makes e(A, B) one, so the check fails) - 5 checks (small route) and 1200 checks (native route)"""
    import bn_amd
    from bn_amd import Fr, G2, groth16
    from test_gpu_msm import _groth16_setup
    rng = np.random.default_rng(880)
    l = 2
    vk, prove = _groth16_setup(rng, l)
    for m in (5, 1200):
        inputs = [[Fr.random(rng) for _ in range(l)] for _ in range(m)]
        proofs = prove(inputs)
        want = np.ones(m, bool)
        inputs[1][1] = inputs[1][1] + Fr.one(); want[1] = False
        proofs[2] = (proofs[2][0], proofs[2][1], proofs[3][2]); want[2] = False
        proofs[m - 1] = (proofs[m - 1][0], G2.zero(), proofs[m - 1][2]); want[m - 1] = False
        plain = groth16.verify_batch(vk, proofs, inputs)
        eng = bn_amd.api.default_engine()
        eng.profile(True); eng.profile_reset()
        try:
            prepared = groth16.verify_batch(vk, proofs, inputs, prepared=True)
            launches = eng.kernel_stats("miller_native_seg")[1]
        finally:
            eng.profile(False)
        assert prepared.dtype == bool and np.array_equal(prepared, plain) and np.array_equal(plain, want), (m, np.flatnonzero(prepared != want))
        assert (launches >= 1) == (m == 1200), (m, launches)
    assert groth16.verify_batch(vk, [], [], prepared=True).shape == (0,)
