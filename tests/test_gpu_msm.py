"""The segmented multi-scalar multiplication on an MI355X (run with -m gpu): bn254_g{1,2}_msm_batch and its _dev / _multi / Python faces, bit
for bit against the oracle - segment j = oracle g*_mul_batch of its terms, folded in index order with g*_add, then g*_normalize; where the
oracle's sum has z == 0 the expected image is G::zero() = (0, 1, 0) (conftest.canon_infinity) - and Groth16 block verification on top."""
import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
from conftest import canon_infinity

pytestmark = pytest.mark.gpu

R = M.R_ORD
FOLD = 4                                   # BN_MSM_FOLD of bn_amd/csrc/bn254_seg.hip: values per lane (lane pair) and fold level
LONG = 3001                                # "one of a few thousand": six fold levels
LENGTHS = [0, 1, 2, 3, FOLD - 1, FOLD, FOLD + 1, FOLD * FOLD + 1, LONG]
STEP = {1: 1 << 20, 2: 1 << 19}            # terms per launch of the term kernel (BN_MUL_LANES_PER_LAUNCH lanes; G2: two lanes per point)
SEAM_SAMPLE = 48                           # segments of the seam call checked against the oracle besides the straddling ones (named cut: the
                                           # full CPU fold of 2^20 terms would take minutes; every segment is still checked device against device)


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
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(te.device)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _ops(oracle, g):
    if g == 1:
        return oracle.g1_mul_batch, oracle.g1_add, oracle.g1_normalize, oracle.g1_zero()
    return oracle.g2_mul_batch, oracle.g2_add, oracle.g2_normalize, oracle.g2_zero()


def _want(oracle, g, P, K, offs, segs=None):
    """the oracle's value of segments `segs` (all by default)"""
    mul, add, norm, zero = _ops(oracle, g)
    out = []
    for j in (range(len(offs) - 1) if segs is None else segs):
        a, b = int(offs[j]), int(offs[j + 1])
        acc = zero
        if b > a:
            for t in mul(P[a:b], K[a:b]):
                acc = add(acc, t)
        out.append(norm(acc))
    return canon_infinity(np.stack(out))


def _msm(eng, g):
    return eng.g1_msm_batch if g == 1 else eng.g2_msm_batch


@pytest.fixture(scope="module")
def points(oracle, te):
    """{g: 512 random points with z != 1}: the reference's own chain on the device (bn254_g*_mul_jacobian_dev), as the other tests make them"""
    import torch
    rng = np.random.default_rng(801)
    out = {}
    for g in (1, 2):
        k = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(512)])
        base = np.tile(oracle.g1_one() if g == 1 else oracle.g2_one(), (512, 1))
        P = _host((te.g1_mul if g == 1 else te.g2_mul)(_dev(te, base), _dev(te, k), normalize=False))
        torch.cuda.synchronize()
        w = P.shape[1] // 3
        assert not np.array_equal(P[0, 2 * w:2 * w + 4], oracle.fp_from_int(E.FQ, 1))            # really z != 1
        out[g] = P
    return out


def _random_scalars(oracle, rng, n):
    return E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(n)])


def _offsets(lengths):
    offs = np.zeros(len(lengths) + 1, np.uint64)
    offs[1:] = np.cumsum(lengths)
    return offs


@pytest.mark.parametrize("g", [1, 2])
def test_ragged_segments_against_the_oracle(oracle, eng, points, g):
    """every length of LENGTHS (0, 1, 2, 3, B-1, B, B+1, B^2+1, a few thousand) at least once, in a shuffled order, random points with z != 1
    and random scalars: every output byte-equal to the oracle's fold"""
    rng = np.random.default_rng(810 + g)
    lengths = LENGTHS + list(rng.choice(LENGTHS[:-1], 40))
    rng.shuffle(lengths)
    offs = _offsets(lengths)
    n = int(offs[-1])
    P = points[g][rng.integers(0, 512, n)]
    K = _random_scalars(oracle, rng, n)
    eng.profile(True); eng.profile_reset()
    try:
        got = _msm(eng, g)(P, K, offs)
        launches = {s: eng.kernel_stats(f"g{g}_msm_{s}")[1] for s in ("mul", "fold")}
    finally:
        eng.profile(False)
    want = _want(oracle, g, P, K, offs)
    for j, L in enumerate(lengths):
        assert np.array_equal(got[j], want[j]), (j, L)
    # one launch of the term kernel; ceil(log_B LONG) fold levels
    levels = 1
    while FOLD ** levels < LONG:
        levels += 1
    assert launches == {"mul": 1, "fold": levels}, launches


def _special_segments(oracle, g, pts, rng):
    """[(name, points, scalars as integers, the sum is the point at infinity)]"""
    zero = oracle.g1_zero() if g == 1 else oracle.g2_zero()
    rs, zs = (E.rescale_g1, E.FQ_Z) if g == 1 else (E.rescale_g2, E.FQ2_Z)
    P, Q, S = pts[0], pts[1], pts[2]
    k, s, t = (int.from_bytes(rng.bytes(40), "little") % R for _ in range(3))
    crafted = (E.glv_crafted() if g == 1 else E.crafted_gls_by_sign() + E.gls_crafted()[::5])
    INF = True
    segs = [
        ("a term with the point at infinity", [P, zero, Q], [k, s, t], False),
        ("infinity first", [zero, P], [k, s], False),
        ("a zero scalar", [P, Q, S], [k, 0, t], False),
        ("all scalars zero", [P, Q, S], [0, 0, 0], INF),
        ("all points at infinity", [zero, zero], [k, s], INF),
        ("the same term twice (doubling branch)", [P, P], [k, k], False),
        ("the same term four times", [P, P, P, P], [k, k, k, k], False),
        ("P k + P (r - k): cancels", [P, P], [k, R - k], INF),
        ("cancels, then a term (infinity as left operand)", [P, P, Q], [k, R - k, s], False),
        ("a term, then a cancelling pair", [Q, P, P], [s, k, R - k], False),
        ("two representations of one point, equal scalars", [rs(oracle, P, zs[4]), rs(oracle, P, zs[3])], [k, k], False),
        ("two representations, opposite scalars", [rs(oracle, P, zs[4]), rs(oracle, P, zs[1])], [k, R - k], INF),
        ("scalars 1 and r - 1 of one point", [P, P], [1, R - 1], INF),
        ("scalars 1, r - 1 of different points", [P, Q], [1, R - 1], False),
        ("scalar 1 twice", [P, P], [1, 1], False),
        ("cancelling runs across a piece boundary", [P] * (2 * FOLD), [k] * FOLD + [R - k] * FOLD, INF),
        ("crafted scalars in one segment", [pts[i % 8] for i in range(len(crafted))], crafted, False),
    ]
    segs += [(f"crafted scalar {c:#x} with a random term", [P, Q], [c, s], False) for c in crafted[:: max(1, len(crafted) // 24)]]
    return segs


@pytest.mark.parametrize("g", [1, 2])
def test_special_branches_each_in_its_own_segment(oracle, eng, points, g):
    rng = np.random.default_rng(820 + g)
    segs = _special_segments(oracle, g, points[g], rng)
    offs = _offsets([len(p) for _, p, _, _ in segs])
    P = np.stack([x for _, p, _, _ in segs for x in p])
    K = E.fr(oracle, [x for _, _, ks, _ in segs for x in ks])
    got = _msm(eng, g)(P, K, offs)
    want = _want(oracle, g, P, K, offs)
    zero = oracle.g1_zero() if g == 1 else oracle.g2_zero()
    for j, (name, _, _, inf) in enumerate(segs):
        assert np.array_equal(got[j], want[j]), name
        assert np.array_equal(got[j], zero) == inf, name                       # infinity exactly where it is meant, and as G::zero()
    # two properties of the oracle on which the expectation above rests: a cancelling sum has z == 0 and normalize leaves it alone
    # (hence canon_infinity in _want), and adding a point to itself equals doubling it after normalisation
    mul, add, norm, _ = _ops(oracle, g)
    k = E.fr(oracle, [5, R - 5])
    T = mul(np.stack([points[g][0]] * 2), k)
    s = add(T[0], T[1])
    w = s.shape[0] // 3
    assert not s[2 * w:].any() and np.array_equal(norm(s), s)                       # z == 0 and normalize leaves it as it is
    dbl = oracle.g1_double if g == 1 else oracle.g2_double
    assert np.array_equal(norm(add(T[0], T[0])), norm(dbl(T[0])))


@pytest.mark.parametrize("g", [1, 2])
def test_segments_of_one_term_are_mul_batch_and_one_segment_is_the_host_fold(oracle, eng, points, g):
    rng = np.random.default_rng(830 + g)
    n = 300
    P = points[g][rng.integers(0, 512, n)]
    K = _random_scalars(oracle, rng, n)
    K[7] = 0; P[11] = oracle.g1_zero() if g == 1 else oracle.g2_zero()
    mulb = eng.g1_mul_batch if g == 1 else eng.g2_mul_batch
    addb = eng.g1_add_batch if g == 1 else eng.g2_add_batch
    terms = mulb(P, K)
    assert np.array_equal(_msm(eng, g)(P, K, np.arange(n + 1, dtype=np.uint64)), terms)
    # mixed: length-1 segments between longer ones
    lengths = [1, 5, 1, 1, FOLD + 1, 1]
    offs = _offsets(lengths)
    got = _msm(eng, g)(P[:int(offs[-1])], K[:int(offs[-1])], offs)
    for j, L in enumerate(lengths):
        if L == 1:
            assert np.array_equal(got[j], terms[int(offs[j])]), j
    # one segment = the host fold through the existing Python API: mul_batch, add_batch level by level, normalise by one
    acc = terms
    while acc.shape[0] > 1:
        if acc.shape[0] % 2:
            acc = np.concatenate([acc, (oracle.g1_zero() if g == 1 else oracle.g2_zero())[None]])
        acc = addb(acc[0::2], acc[1::2])
    folded = mulb(acc, E.fr(oracle, [1]))
    assert np.array_equal(_msm(eng, g)(P, K, [0, n]), folded)
    # ... and through the object API
    import bn_amd
    G = bn_amd.G1 if g == 1 else bn_amd.G2
    pts = [G(p) for p in P[:5]]; ks = [bn_amd.Fr.from_limbs(k) for k in K[:5]]
    one_seg = G.msm(pts, ks)
    assert np.array_equal(one_seg.limbs, _want(oracle, g, P[:5], K[:5], [0, 5])[0])
    batch = (bn_amd.g1_msm_batch if g == 1 else bn_amd.g2_msm_batch)([list(zip(pts, ks)), [], list(zip(pts[:2], ks[:2]))])
    assert np.array_equal(np.stack([b.limbs for b in batch]), _want(oracle, g, np.concatenate([P[:5], P[:2]]), np.concatenate([K[:5], K[:2]]), [0, 5, 5, 7]))
    arr = (bn_amd.g1_msm_batch if g == 1 else bn_amd.g2_msm_batch)(P[:5], K[:5], offsets=[0, 2, 5])
    assert np.array_equal(np.stack([b.limbs for b in arr]), _want(oracle, g, P[:5], K[:5], [0, 2, 5]))


def _seam_inputs(te, g, n):
    """n distinct Jacobian points (the reference chain on the device, as bench.py builds them) and n distinct scalars, device-resident"""
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


def _msm_dev(te, g, P, k, offs, lo=0, hi=None):
    """msm_batch_dev on terms [offs[lo], offs[hi]) / segments [lo, hi) of device tensors"""
    hi = len(offs) - 1 if hi is None else hi
    a, b = int(offs[lo]), int(offs[hi])
    out = te.empty(hi - lo, P.shape[1])
    f = te.e.g1_msm_batch_dev if g == 1 else te.e.g2_msm_batch_dev
    f(P[a:b].data_ptr(), k[a:b].data_ptr(), [int(x) - a for x in offs[lo:hi + 1]], out.data_ptr(), te._stream())
    return out


@pytest.mark.parametrize("g", [1, 2])
def test_launch_cut_and_carry_across_chunks(oracle, te, g):
    """Two calls with BN254_OPT_* untouched.  (a) n just above one launch of the term kernel (2^20 G1 terms / 2^19 G2 points): short ragged
    segments, one of them straddling the cut (asserted) - every segment equal to the same segments computed in calls that stay below the
    cut, and the straddling segment, its neighbours, the first, the last and SEAM_SAMPLE random ones equal to the oracle.  (b) one segment
    longer than two launches (its partial sum is carried in AND out of the middle chunk) between short ones: the long one against the sum
    of its eight parts, each computed below the cut; its neighbours, the last and SEAM_SAMPLE random short ones against the oracle."""
    import torch
    step = STEP[g]
    rng = np.random.default_rng(840 + g)
    nmax = 2 * step + 6000
    P, k = _seam_inputs(te, g, nmax)
    Pn = kn = None

    def host():
        nonlocal Pn, kn
        if Pn is None:
            Pn, kn = _host(P), _host(k)
        return Pn, kn

    # (a)
    lengths = []
    total = 0
    while total < step + 4097:
        L = int(rng.choice([0, 1, 2, 3, 5, FOLD, FOLD + 1, 16, 33]))
        lengths.append(L); total += L
    offs = _offsets(lengths)
    m = len(lengths)
    straddle = [j for j in range(m) if offs[j] < step < offs[j + 1]]
    if not straddle:                                   # a boundary fell on the cut: lengthen the segment in front of it by one term
        j = int(np.searchsorted(offs, step)) - 1
        lengths[j] += 1
        offs = _offsets(lengths)
        straddle = [j for j in range(m) if offs[j] < step < offs[j + 1]]
    assert len(straddle) == 1 and int(offs[-1]) > step
    out = _msm_dev(te, g, P, k, offs)
    torch.cuda.synchronize()
    js = straddle[0]
    # the same segments in calls below the cut: [0, js), {js} alone, (js, m)
    parts = torch.cat([_msm_dev(te, g, P, k, offs, 0, js), _msm_dev(te, g, P, k, offs, js, js + 1), _msm_dev(te, g, P, k, offs, js + 1, m)])
    torch.cuda.synchronize()
    assert torch.equal(out, parts)
    sample = sorted({0, 1, js - 1, js, js + 1, m - 2, m - 1} | set(rng.choice(m, SEAM_SAMPLE, replace=False).tolist()))
    Ph, kh = host()
    assert np.array_equal(_host(out)[sample], _want(oracle, g, Ph, kh, offs, sample)), "seam"

    # (b) segments: 3 short, one of 2 * step + 100 terms, then short ones to the end
    lengths = [2, 0, 5, 2 * step + 100]
    total = sum(lengths)
    while total < nmax - 40:
        L = int(rng.choice([1, 2, 3, FOLD + 1, 16]))
        lengths.append(L); total += L
    offs = _offsets(lengths)
    m = len(lengths)
    assert offs[3] < step and offs[4] > 2 * step and int(offs[-1]) <= nmax
    out = _msm_dev(te, g, P, k, offs)
    torch.cuda.synchronize()
    # the long segment as the sum of eight parts, each a call below the cut, summed by a ninth call with scalars one
    a, b = int(offs[3]), int(offs[4])
    cuts = [a + (b - a) * i // 8 for i in range(9)]
    assert max(y - x for x, y in zip(cuts, cuts[1:])) < step
    partial = torch.cat([_msm_dev(te, g, P, k, cuts, i, i + 1) for i in range(8)])
    ones = _dev(te, E.fr(oracle, [1] * 8))
    total_pt = _msm_dev(te, g, partial, ones, [0, 8])
    torch.cuda.synchronize()
    assert torch.equal(out[3], total_pt[0])
    w = P.shape[1] // 3
    assert _host(out[3:4])[0, 2 * w:].any()                                    # a finite point, not an accident of two infinities
    sample = sorted({0, 1, 2, 4, 5, m - 1} | set(rng.choice(np.arange(4, m), SEAM_SAMPLE, replace=False).tolist()))
    Ph, kh = host()
    assert np.array_equal(_host(out)[sample], _want(oracle, g, Ph, kh, offs, sample)), "carry"


@pytest.mark.parametrize("g", [1, 2])
def test_device_entry_on_a_side_stream(oracle, eng, te, points, g):
    import torch
    rng = np.random.default_rng(850 + g)
    lengths = list(rng.choice(LENGTHS[:-1], 30)) + [300]
    offs = _offsets(lengths)
    n = int(offs[-1])
    P = points[g][rng.integers(0, 512, n)]
    K = _random_scalars(oracle, rng, n)
    dp, dk = _dev(te, P), _dev(te, K)
    out = torch.zeros((len(lengths), P.shape[1]), dtype=torch.int64, device=te.device)
    s = torch.cuda.Stream(te.device)
    s.wait_stream(torch.cuda.current_stream(te.device))
    with torch.cuda.stream(s):
        (eng.g1_msm_batch_dev if g == 1 else eng.g2_msm_batch_dev)(dp.data_ptr(), dk.data_ptr(), [int(x) for x in offs], out.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(_host(out), _msm(eng, g)(P, K, offs))


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
@pytest.mark.parametrize("g", [1, 2])
def test_multi_engine_matches_one_engine(oracle, eng, points, g, devices):
    """segments straddle the natural term shards (a 300-term segment across n/2, n/3 and 2n/3 - asserted); empty segments at both ends
    (offsets[j] == n: the last rank); the offset checks answer on a real handle"""
    import ctypes as C
    import bn_amd
    rng = np.random.default_rng(860 + g)
    lengths = [0, 0, 5, 300, 17, 300, 3, 300, 64, 300, 0, 0]
    offs = _offsets(lengths)
    n, G = int(offs[-1]), len(devices)
    for r in range(1, G):
        b = n * r // G
        assert any(offs[j] < b < offs[j + 1] for j in range(len(lengths))), (G, r, b)
    P = points[g][rng.integers(0, 512, n)]
    K = _random_scalars(oracle, rng, n)
    me = bn_amd.MultiEngine(devices)
    try:
        one = _msm(eng, g)(P, K, offs)
        assert np.array_equal((me.g1_msm_batch if g == 1 else me.g2_msm_batch)(P, K, offs), one)
        assert np.array_equal(one[[0, 1, -1]], np.stack([oracle.g1_zero() if g == 1 else oracle.g2_zero()] * 3))
        # segments that END exactly on a shard boundary and start there
        lengths2 = [n // G] * G + [n - n // G * G]
        offs2 = _offsets(lengths2)
        assert np.array_equal((me.g1_msm_batch if g == 1 else me.g2_msm_batch)(P, K, offs2), _msm(eng, g)(P, K, offs2))
        out = np.zeros((3, P.shape[1]), np.uint64)
        f = me._lib.bn254_g1_msm_batch_multi if g == 1 else me._lib.bn254_g2_msm_batch_multi
        for bad in ([0, 3, 2, 4], [1, 2, 3, 4]):                           # decreasing; offsets[0] != 0
            o = np.array(bad, np.uint64)
            assert f(me._h, C.c_void_p(P.ctypes.data), C.c_void_p(K.ctypes.data), C.c_void_p(o.ctypes.data), 3, C.c_void_p(out.ctypes.data)) == -2, bad
        assert not out.any()
    finally:
        me.close()


# ------------------------------------------------------------------------------------------------ Groth16 block verification
def _groth16_setup(rng, l):
    """a verifying key from a known trapdoor (host Fr arithmetic), and a prover that knows it"""
    import bn_amd
    from bn_amd import Fr, G1, G2, groth16
    eng = bn_amd.api.default_engine()
    alpha, beta, gamma, delta = (Fr.random(rng) for _ in range(4))
    ic = [Fr.random(rng) for _ in range(l + 1)]
    g1, g2 = G1.one().limbs, G2.one().limbs
    pts = eng.g1_mul_batch(np.tile(g1, (l + 2, 1)), np.stack([alpha.limbs] + [c.limbs for c in ic]))
    q = eng.g2_mul_batch(np.tile(g2, (3, 1)), np.stack([beta.limbs, gamma.limbs, delta.limbs]))
    vk = groth16.VerifyingKey(G1(pts[0]), G2(q[0]), G2(q[1]), G2(q[2]), [G1(p) for p in pts[1:]])

    def prove(inputs_list):
        """valid proofs for every set of public inputs, in three GPU calls"""
        a = [Fr.random(rng) for _ in inputs_list]; b = [Fr.random(rng) for _ in inputs_list]
        c = []
        for ai, bi, inp in zip(a, b, inputs_list):
            s = ic[0]
            for x, w in zip(inp, ic[1:]):
                s = s + x * w
            c.append((ai * bi - alpha * beta - gamma * s) * delta.inverse())
        m = len(inputs_list)
        AC = eng.g1_mul_batch(np.tile(g1, (2 * m, 1)), np.stack([x.limbs for x in a + c]))
        Bp = eng.g2_mul_batch(np.tile(g2, (m, 1)), np.stack([x.limbs for x in b]))
        return [(G1(AC[i]), G2(Bp[i]), G1(AC[m + i])) for i in range(m)]
    return vk, prove


@pytest.mark.parametrize("l", [1, 2, 9])
def test_groth16_verify_batch(l):
    from bn_amd import Fr, G1, groth16
    rng = np.random.default_rng(870 + l)
    vk, prove = _groth16_setup(rng, l)
    m = 64 if l == 9 else 5
    inputs = [[Fr.random(rng) for _ in range(l)] for _ in range(m)]
    proofs = prove(inputs)
    assert groth16.verify_batch(vk, proofs, inputs).all()
    want = np.ones(m, bool)
    bad_input = [1] if m == 5 else [3, 17, 40]
    bad_c = [2] if m == 5 else [5, 18, 63]
    bad_a = [4] if m == 5 else [0, 31]
    for j in bad_input:
        inputs[j] = list(inputs[j]); inputs[j][j % l] = inputs[j][j % l] + Fr.one(); want[j] = False
    for j in bad_c:
        proofs[j] = (proofs[j][0], proofs[j][1], proofs[(j + 1) % m][2]); want[j] = False
    for j in bad_a:
        proofs[j] = (G1.zero(), proofs[j][1], proofs[j][2]); want[j] = False
    got = groth16.verify_batch(vk, proofs, inputs)
    assert got.dtype == bool and np.array_equal(got, want), np.flatnonzero(got != want)
    single = np.array([groth16.verify_batch(vk, [proofs[j]], [inputs[j]])[0] for j in range(m)])
    assert np.array_equal(single, want)
    assert groth16.verify_batch(vk, [], []).shape == (0,)
