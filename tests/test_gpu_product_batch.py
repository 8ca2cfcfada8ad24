"""The batched multi-pairing on an MI355X (run with -m gpu): bn254_pairing_product_batch and its _dev / _multi / Python / C++ faces, bit for
bit against the oracle (segment j = the oracle's pairings of its pairs folded with fq12_mul: the final exponentiation is a homomorphism), on
every route - the two-launch wave route (Miller loops per wave + the ragged wave tail), the segmented lane-pair fold after each Miller
mapping, segments across chunk seams - and as the predicate of pairing checks."""
import numpy as np
import pytest

import edge_inputs as E
from bn_oracle import FR

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 5, 16, 17, 64, 300]


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def pool(oracle):
    """unique pairs (P, Q) and their pairings: random Jacobian points (z != 1), edge representations of edge points, points at infinity on
    either side.  Batches index into it, so pairs repeat and the expected values cost one oracle pairing per unique pair."""
    rng = np.random.default_rng(2024)
    n = 160
    k = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(2 * n)])
    P = list(oracle.g1_mul_batch_jacobian(np.tile(oracle.g1_one(), (n, 1)), k[:n]))
    Q = list(oracle.g2_mul_batch_jacobian(np.tile(oracle.g2_one(), (n, 1)), k[n:]))
    g1e = [E.rescale_g1(oracle, p, z) for p in E.edge_g1_points(oracle) for z in E.FQ_Z[:4]]
    g2e = [E.rescale_g2(oracle, q, z) for q in E.edge_g2_points(oracle) for z in E.FQ2_Z[:4]]
    for i, p in enumerate(g1e):
        P.append(p); Q.append(Q[i])
    for i, q in enumerate(g2e):
        P.append(P[i]); Q.append(q)
    for i in range(4):
        P.append(oracle.g1_zero()); Q.append(Q[i])
        P.append(P[i]); Q.append(oracle.g2_zero())
    P, Q = np.stack(P), np.stack(Q)
    return P, Q, oracle.pairing_batch(P, Q)


def _segments(rng, pool, lengths):
    """CSR offsets and the pool index of every pair for segments of the given lengths"""
    offs = np.zeros(len(lengths) + 1, np.uint64)
    offs[1:] = np.cumsum(lengths)
    idx = rng.integers(0, pool[0].shape[0], int(offs[-1]))
    return offs, idx


def _want(oracle, pool, offs, idx, segs=None):
    """oracle value of segments `segs` (all by default): fold of the pool's pairings with fq12_mul"""
    B = pool[2]
    out = []
    for j in (range(len(offs) - 1) if segs is None else segs):
        acc = oracle.fq12_one()
        for i in idx[int(offs[j]):int(offs[j + 1])]:
            acc = oracle.fq12_mul(acc, B[i])
        out.append(acc)
    return np.stack(out)


def _stats(eng, names=("gt_segment", "gt_tail_seg", "miller_wave", "miller_quad", "miller", "pairing_wave", "final_exp_wave", "final_exp_quad", "final_exp")):
    return {k: eng.kernel_stats(k)[1] for k in names}


def _run(eng, pool, offs, idx, **opts):
    eng.profile(True); eng.profile_reset()
    try:
        with eng.options(**opts):
            got = eng.pairing_product_batch(pool[0][idx], pool[1][idx], offs)
        return got, _stats(eng)
    finally:
        eng.profile(False)


def test_ragged_segments_against_the_oracle(oracle, eng, pool):
    """~300 segments with lengths from {0, 1, 2, 3, 4, 5, 16, 17, 64, 300}; every output byte-equal to the oracle's fold, to
    Engine.pairing_product on the segment alone, and (length 1) to pairing_batch"""
    rng = np.random.default_rng(1)
    lengths = list(rng.choice(LENGTHS, 300)) + [0, 300, 0, 1]
    offs, idx = _segments(rng, pool, lengths)
    got, st = _run(eng, pool, offs, idx)
    want = _want(oracle, pool, offs, idx)
    assert got.shape == (len(lengths), 48)
    bad = [j for j in range(len(lengths)) if not np.array_equal(got[j], want[j])]
    assert not bad, (bad[:10], [lengths[j] for j in bad[:10]])
    assert st["gt_segment"] >= 1
    for j in range(len(lengths)):
        a, b = int(offs[j]), int(offs[j + 1])
        assert np.array_equal(got[j], eng.pairing_product(pool[0][idx[a:b]], pool[1][idx[a:b]])), j
    ones = [j for j, L in enumerate(lengths) if L == 1]
    single = eng.pairing_batch(pool[0][idx[offs[ones].astype(np.int64)]], pool[1][idx[offs[ones].astype(np.int64)]])
    assert np.array_equal(got[ones], single)


def test_goldens_through_segments(oracle, eng, goldens):
    """the committed pairing goldens: as 96 segments of one pair, and grouped (the products of the goldens)"""
    g1, g2, gt = goldens["g1"], goldens["g2"], goldens["gt"]
    n = g1.shape[0]
    assert np.array_equal(eng.pairing_product_batch(g1, g2, np.arange(n + 1)), gt)
    offs = np.array([0, 3, 3, 10, 11, 40, n], np.uint64)
    want = []
    for a, b in zip(offs[:-1], offs[1:]):
        acc = oracle.fq12_one()
        for i in range(int(a), int(b)):
            acc = oracle.fq12_mul(acc, gt[i])
        want.append(acc)
    assert np.array_equal(eng.pairing_product_batch(g1, g2, offs), np.stack(want))


def test_routes_give_the_same_bytes(oracle, eng, pool):
    """the two-launch wave route, the wave route behind fold levels (segments above the tail cap), the segmented fold after every Miller
    mapping (wave / four-lane / lane pairs: 3584, 16384 and 2^16 pairs in a call) - each proven to have run by its profile scope"""
    rng = np.random.default_rng(2)
    short = list(rng.choice([0, 1, 2, 3, 4, 5, 16], 40))
    offs, idx = _segments(rng, pool, short)
    want = _want(oracle, pool, offs, idx)
    got, st = _run(eng, pool, offs, idx)
    assert np.array_equal(got, want)
    assert st["gt_tail_seg"] == 1 and st["gt_segment"] == 0 and st["miller_wave"] == 1 and st["final_exp_wave"] == 0     # two launches
    got, st = _run(eng, pool, offs, idx, wave_pairing_max=0)
    assert np.array_equal(got, want) and st["gt_tail_seg"] == 0 and st["gt_segment"] >= 1

    mixed = list(rng.choice(LENGTHS, 12)) + [300, 17]
    offs, idx = _segments(rng, pool, mixed)
    want = _want(oracle, pool, offs, idx)
    got, st = _run(eng, pool, offs, idx)
    assert np.array_equal(got, want) and st["gt_tail_seg"] == 1 and st["gt_segment"] >= 1       # long segments folded down to the tail
    got, st = _run(eng, pool, offs, idx, wave_fe_max=0)
    assert np.array_equal(got, want) and st["gt_tail_seg"] == 0 and st["gt_segment"] >= 1

    # the hand-over sizes of the Miller mappings (3584, 16384 and one machine round, 2^16, on 256 CUs)
    for total, miller in ((eng.get_option("wave_pairing_max"), "miller_wave"), (eng.get_option("quad_max"), "miller_quad"), (eng.get_option("round_pairs"), "miller")):
        lengths = []
        while sum(lengths) < total:
            lengths.append(int(rng.choice(LENGTHS)))
        lengths[-1] -= sum(lengths) - total
        offs, idx = _segments(rng, pool, lengths)
        got, st = _run(eng, pool, offs, idx)
        assert st[miller] == 1 and st["gt_segment"] >= 1, (total, st)
        sample = sorted(set(rng.integers(0, len(lengths), 200).tolist()) | {len(lengths) - 1})
        assert np.array_equal(got[sample], _want(oracle, pool, offs, idx, sample)), total


def test_segments_across_chunks(oracle, eng, pool):
    """chunks of one machine round cut down to 64 pairs (BN254_OPT_ROUND_PAIRS): segments of 300, 65 and 64 pairs cross chunk seams and carry
    their partial product; on the wave Miller kernel and on the lane-pair one"""
    rng = np.random.default_rng(3)
    lengths = [300, 5, 0, 70, 1, 64, 65, 3, 0, 129, 2, 0]
    offs, idx = _segments(rng, pool, lengths)
    want = _want(oracle, pool, offs, idx)
    got, _ = _run(eng, pool, offs, idx, round_pairs=64)
    assert np.array_equal(got, want)
    got, st = _run(eng, pool, offs, idx, round_pairs=64, wave_pairing_max=0, quad_max=0)
    assert np.array_equal(got, want) and st["miller"] >= 10


def test_one_long_segment_beside_many_empty_ones(eng, pool):
    """one segment of 5000 pairs between 2 x 10 000 empty segments: ceil(log16 5000) = 4 fold levels, not 5000 products in a row"""
    rng = np.random.default_rng(4)
    lengths = [0] * 10000 + [5000] + [0] * 10000
    offs, idx = _segments(rng, pool, lengths)
    got, st = _run(eng, pool, offs, idx)
    assert st["gt_segment"] == 4, st
    one = np.zeros(48, np.uint64); one[:4] = [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]
    assert (got[:10000] == one).all() and (got[10001:] == one).all()
    assert np.array_equal(got[10000], eng.pairing_product(pool[0][idx], pool[1][idx]))


def test_many_four_pair_segments(oracle, eng, pool):
    """m = 2^16 segments of 4 pairs (2^18 pairs, four chunks): 2048 segments spread over the batch, the last included, against the oracle"""
    rng = np.random.default_rng(5)
    m = 1 << 16
    offs, idx = _segments(rng, pool, [4] * m)
    got = eng.pairing_product_batch(pool[0][idx], pool[1][idx], offs)
    sample = sorted(set(np.linspace(0, m - 1, 2048).astype(int).tolist()))
    assert sample[-1] == m - 1
    assert np.array_equal(got[sample], _want(oracle, pool, offs, idx, sample))


def test_checks(oracle, eng):
    """pairing_check_batch: e(aP, bQ) e(-abP, Q) == 1 and e(P, Q) e(-P, Q) == 1; the same with one scalar changed is not"""
    import bn_amd
    from bn_amd.api import R_MOD
    P, Q = oracle.g1_one(), oracle.g2_one()
    a, b = 12345678901234567890, 98765432109876543210
    fr = lambda v: oracle.fp_from_int(FR, v % R_MOD)
    aP, bQ, abP = oracle.g1_mul(P, fr(a)), oracle.g2_mul(Q, fr(b)), oracle.g1_mul(P, fr(a * b))
    abP1 = oracle.g1_mul(P, fr(a * b + 1))
    ps = np.stack([aP, oracle.g1_neg(abP), P, oracle.g1_neg(P), aP, oracle.g1_neg(abP1), P, oracle.g1_neg(aP)])
    qs = np.stack([bQ, Q, Q, Q, bQ, Q, Q, Q])
    offs = [0, 2, 4, 6, 8, 8]
    ok = bn_amd.pairing_check_batch(ps, qs, offs, engine=eng)
    assert ok.dtype == bool and ok.tolist() == [True, True, False, False, True]
    G1, G2 = bn_amd.G1, bn_amd.G2
    segs = [[(G1(aP), G2(bQ)), (G1(oracle.g1_neg(abP)), G2(Q))], [], [(G1(P), G2(Q))]]
    res = bn_amd.pairing_product_batch(segs, engine=eng)
    assert res[0] == bn_amd.Gt.one() and res[1] == bn_amd.Gt.one() and np.array_equal(res[2].limbs, oracle.pairing_batch(P, Q)[0])
    assert bn_amd.pairing_check_batch(segs, engine=eng).tolist() == [True, True, False]


def test_device_entry_on_a_side_stream(eng, pool):
    import torch
    rng = np.random.default_rng(6)
    lengths = list(rng.choice(LENGTHS, 30))
    offs, idx = _segments(rng, pool, lengths)
    P, Q = pool[0][idx], pool[1][idx]
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.ascontiguousarray(P).view(np.int64)).to(dev)
    dq = torch.from_numpy(np.ascontiguousarray(Q).view(np.int64)).to(dev)
    out = torch.zeros((len(lengths), 48), dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        eng.pairing_product_batch_dev(dp.data_ptr(), dq.data_ptr(), [int(x) for x in offs], out.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), eng.pairing_product_batch(P, Q, offs))


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_engine_matches_one_engine(eng, pool, devices):
    """segments straddle the natural pair shards (a 300-pair segment across n/2, n/3 and 2n/3 - asserted); empty segments at both ends;
    the offset checks answer on a real handle"""
    import ctypes as C
    import bn_amd
    rng = np.random.default_rng(7)
    lengths = [0, 0, 5, 300, 17, 300, 3, 300, 64, 300, 0]
    offs, idx = _segments(rng, pool, lengths)
    n, G = int(offs[-1]), len(devices)
    for g in range(1, G):
        b = n * g // G
        assert any(offs[j] < b < offs[j + 1] for j in range(len(lengths))), (G, g, b)
    P, Q = pool[0][idx], pool[1][idx]
    me = bn_amd.MultiEngine(devices)
    try:
        assert np.array_equal(me.pairing_product_batch(P, Q, offs), eng.pairing_product_batch(P, Q, offs))
        out = np.zeros((3, 48), np.uint64)
        for bad in ([0, 3, 2, 4], [1, 2, 3, 4]):                           # decreasing; offsets[0] != 0
            o = np.array(bad, np.uint64)
            rc = me._lib.bn254_pairing_product_batch_multi(me._h, C.c_void_p(P.ctypes.data), C.c_void_p(Q.ctypes.data), C.c_void_p(o.ctypes.data), 3,
                                                            C.c_void_p(out.ctypes.data))
            assert rc == -2, bad
        assert not out.any()
    finally:
        me.close()


def test_small_route_with_a_deep_fold(oracle, eng, pool):
    """the wave route raised above 4096 pairs (BN254_OPT_WAVE_PAIRING_MAX): a segment of 5000 pairs needs three fold levels before the
    ragged tail, which must still find the 17-pair segment's partial products where its own level left them"""
    rng = np.random.default_rng(8)
    for lengths in ([17, 5000], [5000, 17], [17, 300, 0, 5000, 33, 4]):
        offs, idx = _segments(rng, pool, lengths)
        got, st = _run(eng, pool, offs, idx, wave_pairing_max=8192)
        assert st["gt_tail_seg"] == 1 and st["miller_wave"] == 1 and st["gt_segment"] == 3, (lengths, st)
        assert np.array_equal(got, _want(oracle, pool, offs, idx)), lengths


def test_cpp_host_product_batch(oracle, tmp_path):
    """a compiled host program (g++ on include/bn254.hpp): bn::pairing_product_batch and bn::pairing_check_batch"""
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
    for (auto &g : pairing_product_batch(p, q, {0, 2, 2, 5})) dump(g);
    std::vector<G1> cp = {G1::one(), -G1::one(), G1::one(), G1::one()};
    std::vector<G2> cq = {G2::one(), G2::one(), G2::one(), G2::one()};
    for (bool ok : pairing_check_batch(cp, cq, {0, 2, 4, 4})) std::printf("%d\n", ok ? 1 : 0);
    return 0;
}
''')
    exe = tmp_path / "host"
    subprocess.check_call(["g++", "-std=c++17", "-I", str(root / "include"), str(src), "-o", str(exe),
                           "-L", str(root / "bn_amd"), "-lbn254_hip", "-Wl,-rpath," + str(root / "bn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lines = subprocess.check_output([str(exe)], timeout=600).decode().strip().split("\n")
    got = [np.array([int(x) for x in l.split()], np.uint64) for l in lines[:3]]
    P = np.stack([oracle.g1_one()] * 5); Q = np.stack([oracle.g2_one()] * 5)
    for i in range(1, 5):
        P[i] = oracle.g1_add(P[i - 1], oracle.g1_one()); Q[i] = oracle.g2_add(Q[i - 1], Q[i - 1])
    P[3] = oracle.g1_zero()
    B = oracle.pairing_batch(P, Q)
    assert np.array_equal(got[0], oracle.fq12_mul(B[0], B[1]))
    assert np.array_equal(got[1], oracle.fq12_one())
    assert np.array_equal(got[2], oracle.fq12_mul(oracle.fq12_mul(B[2], B[3]), B[4]))
    assert [l.strip() for l in lines[3:6]] == ["1", "0", "1"]
