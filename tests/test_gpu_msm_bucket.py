"""One large multi-scalar multiplication by the bucket (Pippenger) method on an MI355X (run with -m gpu): bn254_g{1,2}_msm and its _dev /
_multi / Python faces.  Unless stated otherwise the bucket route is forced (msm_bucket_min = 0).  Up to n = 600 every result is compared with
the oracle - g*_mul_batch of the terms, g*_add in index order, g*_normalize, the point at infinity as G::zero() (conftest.canon_infinity);
larger cases device against device, with the one-segment g*_msm_batch (the parent's route, still in the library) as the comparison.

Two readings of the issue that the cases below fix: (1) with default options n == 1 is, like the one-segment msm_batch it is defined to be,
the plain multiplication kernel (scope g*_mul), so "the fold ran" is asserted for every n but 1 and "the multiplication ran" for n == 1;
(2) "every digit equal to 2^c - 1" is not below r for any c, so the crafted scalar fills every window but the top one."""
import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
from conftest import canon_infinity

pytestmark = pytest.mark.gpu

R = M.R_ORD
SIZES = [0, 1, 2, 3, 63, 64, 65, 257]
WIDTHS = [1, 2, 5, 8, 9, 11, 12, 13, 14, 16]                # 9, 11, 12, 14: what bn_msm_window_bits picks from 2^15 terms on
BUCKET_SCOPES = ("digits", "bucket", "reduce")


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


def _zero(oracle, g):
    return oracle.g1_zero() if g == 1 else oracle.g2_zero()


def _fold(oracle, g, terms):
    add, norm = (oracle.g1_add, oracle.g1_normalize) if g == 1 else (oracle.g2_add, oracle.g2_normalize)
    acc = _zero(oracle, g)
    for t in terms:
        acc = add(acc, t)
    return canon_infinity(norm(acc)[None])[0]


def _want(oracle, g, P, K):
    """the oracle fold: mul_batch, add in index order, normalize"""
    assert len(P) <= 600
    mul = oracle.g1_mul_batch if g == 1 else oracle.g2_mul_batch
    return _fold(oracle, g, mul(np.asarray(P), np.asarray(K)) if len(P) else [])


def _msm(eng, g):
    return eng.g1_msm if g == 1 else eng.g2_msm


def _batch(eng, g, P, K):
    """the parent's route: one segment of the segmented call"""
    return (eng.g1_msm_batch if g == 1 else eng.g2_msm_batch)(P, K, [0, len(P)])[0]


def _scopes(eng, g):
    return {s: eng.kernel_stats(f"g{g}_msm_{s}")[1] for s in BUCKET_SCOPES + ("fold", "mul")} | {"plain_mul": eng.kernel_stats(f"g{g}_mul")[1]}


@pytest.fixture(scope="module")
def points(oracle, te):
    """{g: 512 random points with z != 1}: the reference's own chain on the device, as tests/test_gpu_msm.py makes them"""
    import torch
    rng = np.random.default_rng(1001)
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


@pytest.fixture(scope="module")
def prefix(oracle, points):
    """{g: (P, K, want)}: 257 terms with random full-width scalars and want[n] = the oracle fold of the first n terms, computed once"""
    out = {}
    for g in (1, 2):
        rng = np.random.default_rng(1010 + g)
        P = points[g][rng.integers(0, 512, max(SIZES))]
        K = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(max(SIZES))])
        terms = (oracle.g1_mul_batch if g == 1 else oracle.g2_mul_batch)(P, K)
        out[g] = (P, K, {n: _fold(oracle, g, terms[:n]) for n in SIZES})
    return out


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("g", [1, 2])
def test_sizes_and_window_widths(eng, prefix, g, c):
    """digits inside a word (1, 2, 8, 16), across word seams (5, 9, 11, 12, 13, 14), a short top window (5, 8, 13, 16; one bit at 11, two bits
    at 9, 12 and 14), the largest bucket table (16)"""
    P, K, want = prefix[g]
    with eng.options(msm_bucket_min=0, msm_window_bits=c):
        for n in SIZES:
            eng.profile(True); eng.profile_reset()
            try:
                got = _msm(eng, g)(P[:n], K[:n])
                ran = _scopes(eng, g)
            finally:
                eng.profile(False)
            assert np.array_equal(got, want[n]), (n, c)
            # the bucket scopes ran (no terms: nothing to sort or accumulate, the reduction and the tail still run), then the tail's fold
            assert ran["reduce"] == 1 and ran["fold"] >= 1 and ran["mul"] == 1, (n, c, ran)
            assert (ran["digits"], ran["bucket"]) == ((1, 1) if n else (0, 0)), (n, c, ran)


@pytest.mark.parametrize("g", [1, 2])
def test_default_options_take_the_segmented_route_at_these_sizes(eng, prefix, g):
    P, K, want = prefix[g]
    assert eng.get_option_raw("msm_bucket_min") is None and eng.get_option("msm_bucket_min") > max(SIZES)
    for n in SIZES:
        eng.profile(True); eng.profile_reset()
        try:
            got = _msm(eng, g)(P[:n], K[:n])
            ran = _scopes(eng, g)
        finally:
            eng.profile(False)
        assert np.array_equal(got, want[n]), n
        assert [ran[s] for s in BUCKET_SCOPES] == [0, 0, 0], (n, ran)
        if n == 1:
            assert ran["plain_mul"] == 1 and ran["fold"] == 0, ran               # one segment of one term IS bn254_g*_mul_batch
        else:
            assert ran["fold"] >= 1, (n, ran)


def _crafted(c):
    W = (254 + c - 1) // c
    return [0, 1, R - 1, (1 << (c * (W - 1))) - 1, 1, 1 << (c * (W // 2)), 1 << (c * (W - 1)), 1 << 253]


@pytest.mark.parametrize("c", [5, 11, 13, 14])
@pytest.mark.parametrize("g", [1, 2])
def test_crafted_scalars(oracle, eng, points, g, c):
    """0, 1, r - 1, every window but the top one full, one set bit in the first / a middle / the top window, 2^253: each alone, each beside
    a random term, and all in one call; an all-zero scalar vector gives (0, 1, 0).  c = 11 has a top window of one bit and c = 14 one of
    two bits: the default widths of 2^16, 2^17 and 2^19 terms and of 2^20 terms and more"""
    rng = np.random.default_rng(1020 + g + c)
    ks = _crafted(c)
    P = points[g][rng.integers(0, 512, len(ks) + 1)]
    rnd = int.from_bytes(rng.bytes(40), "little") % R
    with eng.options(msm_bucket_min=0, msm_window_bits=c):
        for i, k in enumerate(ks):
            K = E.fr(oracle, [k])
            assert np.array_equal(_msm(eng, g)(P[i:i + 1], K), _want(oracle, g, P[i:i + 1], K)), hex(k)
            K = E.fr(oracle, [k, rnd])
            assert np.array_equal(_msm(eng, g)(P[i:i + 2], K), _want(oracle, g, P[i:i + 2], K)), hex(k)
        K = E.fr(oracle, ks)
        assert np.array_equal(_msm(eng, g)(P[:len(ks)], K), _want(oracle, g, P[:len(ks)], K))
        assert np.array_equal(_msm(eng, g)(P[:5], E.fr(oracle, [0] * 5)), _zero(oracle, g))


@pytest.mark.parametrize("g", [1, 2])
def test_collisions_inside_a_bucket(oracle, eng, points, g):
    rng = np.random.default_rng(1030 + g)
    zero = _zero(oracle, g)
    k, s = (int.from_bytes(rng.bytes(40), "little") % R for _ in range(2))
    pts = points[g]
    neg = (eng.g1_add_batch if g == 1 else eng.g2_add_batch)(zero[None], pts[:1], negate_b=True)[0]          # -P, the reference's own limbs
    with eng.options(msm_bucket_min=0, msm_window_bits=8):
        # the skew case: one scalar, every term in one bucket per window - device against device (n > 600 for G1)
        n = 1000 if g == 1 else 300
        P = pts[rng.integers(0, 512, n)]
        K = E.fr(oracle, [k] * n)
        got = _msm(eng, g)(P, K)
        assert np.array_equal(got, _batch(eng, g, P, K))
        if n <= 600:
            assert np.array_equal(got, _want(oracle, g, P, K))
        cases = [(f"the same term {t} times", [pts[0]] * t, [k] * t, False) for t in (2, 3, 5)]
        cases += [
            ("P and -P, one scalar", [pts[0], neg], [k, k], True),
            ("P and -P, then a term in another bucket", [pts[0], neg, pts[1]], [k, k, s], False),
            ("P k + P (r - k)", [pts[0], pts[0]], [k, R - k], True),
            ("points at infinity sprinkled in", [zero, pts[0], zero, pts[1], pts[2], zero], [k, s, s, k, s, k], False),
            ("only points at infinity", [zero, zero, zero], [k, s, k], True),
            ("a list whose total is zero", [pts[0], pts[1], pts[0], pts[1]], [k, s, R - k, R - s], True),
        ]
        for name, P, ks, inf in cases:
            P = np.stack(P); K = E.fr(oracle, ks)
            got = _msm(eng, g)(P, K)
            assert np.array_equal(got, _want(oracle, g, P, K)), name
            assert np.array_equal(got, zero) == inf, name


@pytest.mark.parametrize("n", [64, 65, 200])
@pytest.mark.parametrize("g", [1, 2])
def test_chunk_seams(eng, prefix, oracle, g, n):
    """msm_chunk = 64: one full pass, a pass of one term behind it, four passes - all into the same buckets and the one tail"""
    P, K, want = prefix[g]
    for c in (5, 11, 13, 14):
        with eng.options(msm_bucket_min=0, msm_window_bits=c, msm_chunk=64):
            eng.profile(True); eng.profile_reset()
            try:
                got = _msm(eng, g)(P[:n], K[:n])
                ran = _scopes(eng, g)
            finally:
                eng.profile(False)
        assert ran["digits"] == (n + 63) // 64 and ran["bucket"] == (n + 63) // 64 and ran["reduce"] == 1, ran
        assert np.array_equal(got, want[n] if n in want else _want(oracle, g, P[:n], K[:n])), (n, c)


@pytest.mark.parametrize("g", [1, 2])
def test_device_entry_on_a_side_stream(eng, te, prefix, g):
    import torch
    P, K, want = prefix[g]
    n = 257
    dP, dK = _dev(te, P[:n]), _dev(te, K[:n])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=te.device)
    f = eng.g1_msm_dev if g == 1 else eng.g2_msm_dev
    with eng.options(msm_bucket_min=0, msm_window_bits=5):
        with torch.cuda.stream(side):
            out = te.empty(1, P.shape[1])
            f(dP.data_ptr(), dK.data_ptr(), n, out.data_ptr(), side.cuda_stream)
            out0 = te.empty(1, P.shape[1])
            f(0, 0, 0, out0.data_ptr(), side.cuda_stream)                             # no terms: NULL p and k are fine
        side.synchronize()
    assert np.array_equal(_host(out)[0], want[n])
    assert np.array_equal(_host(out0)[0], want[0])


@pytest.mark.parametrize("g", [1, 2])
def test_two_ranks_on_one_gpu(oracle, prefix, g):
    import bn_amd
    P, K, want = prefix[g]
    m = bn_amd.MultiEngine([0, 0])
    try:
        for opts in ({}, {"msm_bucket_min": 0, "msm_window_bits": 5}):
            for name, v in opts.items():
                m.set_option(name, v)
            f = m.g1_msm if g == 1 else m.g2_msm
            assert np.array_equal(f(P[:1], K[:1]), want[1])                           # rank 0's shard is empty
            assert np.array_equal(f(P[:129], K[:129]), _want(oracle, g, P[:129], K[:129]))
            assert np.array_equal(f(P[:0], K[:0]), want[0])
    finally:
        m.close()


@pytest.mark.parametrize("g", [1, 2])
def test_python_faces(prefix, g):
    import bn_amd
    P, K, want = prefix[g]
    G = bn_amd.G1 if g == 1 else bn_amd.G2
    f = bn_amd.g1_msm if g == 1 else bn_amd.g2_msm
    e = bn_amd.api.default_engine()
    with e.options(msm_bucket_min=0, msm_window_bits=5):
        pts = [G(p) for p in P[:65]]; ks = [bn_amd.Fr.from_limbs(k) for k in K[:65]]
        assert np.array_equal(f(pts, ks).limbs, want[65])
        assert np.array_equal(f(P[:65], K[:65]).limbs, want[65])                      # (n, WORDS) / (n, 4) arrays
        assert np.array_equal(G.msm(pts, ks).limbs, want[65])
        assert np.array_equal(f([], []).limbs, G.zero().limbs)
    assert np.array_equal(G.msm(pts[:3], ks[:3]).limbs, want[3])                      # default options: the old route, the same bytes
    own = bn_amd.Engine(0)
    with own.options(msm_bucket_min=0):
        assert np.array_equal(f(P[:64], K[:64], engine=own).limbs, want[64])
    own.close()


@pytest.mark.parametrize("g, n", [(1, 1 << 14), (2, 1 << 12)])
def test_mid_size_at_the_default_window_table(eng, te, g, n):
    """device-made distinct points (z != 1) and scalars; the bucket route at its default width against the one-segment msm_batch"""
    import torch
    from bn_amd import distributed as D
    g1, g2 = D.generator_limbs()
    kb = D.synthetic_scalars_device(te, 0, n, g - 1)
    base = te.empty(n, 12 if g == 1 else 24)
    te.e.tile_dev(_dev(te, g1 if g == 1 else g2).data_ptr(), 96 if g == 1 else 192, n, base.data_ptr(), te._stream())
    P = (te.g1_mul if g == 1 else te.g2_mul)(base, kb, normalize=False)
    k = D.synthetic_scalars_device(te, 1 << 24, (1 << 24) + n, 1)
    out, ref = te.empty(1, P.shape[1]), te.empty(1, P.shape[1])
    with eng.options(msm_bucket_min=0):
        assert eng.get_option_raw("msm_window_bits") is None
        eng.profile(True); eng.profile_reset()
        try:
            (eng.g1_msm_dev if g == 1 else eng.g2_msm_dev)(P.data_ptr(), k.data_ptr(), n, out.data_ptr(), te._stream())
            torch.cuda.synchronize()
            ran = _scopes(eng, g)
        finally:
            eng.profile(False)
    (eng.g1_msm_batch_dev if g == 1 else eng.g2_msm_batch_dev)(P.data_ptr(), k.data_ptr(), [0, n], ref.data_ptr(), te._stream())
    torch.cuda.synchronize()
    assert [ran[s] for s in BUCKET_SCOPES] == [1, 1, 1], ran
    assert torch.equal(out, ref)
    w = P.shape[1] // 3
    assert _host(out)[0, 2 * w:].any()                                                # a finite point


def test_option_ranges(eng):
    from bn_amd import _native
    for name, bad in (("msm_window_bits", 0), ("msm_window_bits", 17), ("msm_chunk", 0), ("msm_chunk", (1 << 22) + 1)):
        with pytest.raises(_native.Bn254Error):
            eng.set_option(name, bad)
        assert eng.get_option_raw(name) is None
    for name, ok in (("msm_window_bits", 1), ("msm_window_bits", 16), ("msm_chunk", 1), ("msm_chunk", 1 << 22), ("msm_bucket_min", 0), ("msm_bucket_min", 1 << 40)):
        with eng.options(**{name: ok}):
            assert eng.get_option(name) == ok
    assert eng.get_option("msm_window_bits") == -1 and eng.get_option("msm_chunk") == 1 << 20          # by size; the default pass
