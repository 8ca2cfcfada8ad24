"""Multi-scalar multiplication against prepared bases on an MI355X (run with -m gpu): bn254_g{1,2}_msm_prepare / bn254_g{1,2}_msm_prepared
and their _dev and Python faces.  The points are those of tests/test_gpu_msm_bucket.py - device-made, z != 1, 257 terms with the oracle fold
computed once.  Unless stated otherwise the prepared bucket route is forced (msm_bucket_min = 0).  Small cases are compared with the oracle
(g*_mul_batch of the terms, g*_add in index order, g*_normalize, infinity as G::zero()), larger ones device against device with
bn254_g{1,2}_msm / _msm_batch on the same raw points and scalars - the bytes the prepared call is defined to return."""
import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
import hostsim_msm_prepared_lib as L
from conftest import canon_infinity
from test_gpu_msm_bucket import SIZES, _batch, _dev, _host, _want, _zero, eng, points, prefix, te  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

R = M.R_ORD
WIDTHS = [3, 5, 8, 11, 13, 14, 16]
NEW = ("digits", "bucket", "reduce")


def _prepare(eng, g, P, c=None):
    return (eng.g1_msm_prepare if g == 1 else eng.g2_msm_prepare)(P, c)


def _call(eng, g):
    return eng.g1_msm_prepared if g == 1 else eng.g2_msm_prepared


def _scopes(eng, g):
    s = {"p_" + n: eng.kernel_stats(f"g{g}_msmp_{n}")[1] for n in NEW + ("table",)}
    s.update({n: eng.kernel_stats(f"g{g}_msm_{n}")[1] for n in NEW + ("fold", "mul")})
    s["plain_mul"] = eng.kernel_stats(f"g{g}_mul")[1]
    return s


def _profiled(eng, g, fn):
    eng.profile(True); eng.profile_reset()
    try:
        got = fn()
        return got, _scopes(eng, g)
    finally:
        eng.profile(False)


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("g", [1, 2])
def test_sizes_and_window_widths(eng, prefix, g, c):
    """digits inside a word (8, 16) and across word seams (3, 5, 11, 13, 14), a short top window, 4 to 32768 buckets; the prepared scopes ran (no
    terms: nothing to sort or accumulate, the reduction and the tail still run) and the scopes of bn254_g{1,2}_msm's bucket route did not"""
    P, K, want = prefix[g]
    W = (254 + c - 1) // c
    h, built = _profiled(eng, g, lambda: _prepare(eng, g, P, c))
    try:
        assert (h.count, h.group, h.window_bits) == (len(P), g, c)
        assert h.device_bytes == W * len(P) * 80 * g + len(P) * 96 * g
        assert built["p_table"] == W
        with eng.options(msm_bucket_min=0):
            for n in SIZES:
                got, ran = _profiled(eng, g, lambda: _call(eng, g)(h, K[:n]))
                assert np.array_equal(got, want[n]), (n, c)
                assert ran["p_reduce"] == 1 and ran["fold"] >= 1 and ran["mul"] == 1, (n, c, ran)
                assert (ran["p_digits"], ran["p_bucket"]) == ((1, 1) if n else (0, 0)), (n, c, ran)
                assert (ran["digits"], ran["bucket"], ran["reduce"], ran["p_table"]) == (0, 0, 0, 0), (n, c, ran)
    finally:
        h.close()


@pytest.mark.parametrize("g", [1, 2])
def test_default_options_take_the_small_route_at_these_sizes(eng, prefix, g):
    """the one-segment bn254_g{1,2}_msm_batch on the handle's kept points: the same bytes, none of the prepared scopes but the build's"""
    from bn_amd import _native
    P, K, want = prefix[g]
    lib = _native.lib()
    assert eng.get_option_raw("msm_bucket_min") is None and lib.bn254_msm_prepared_default_min(g) > max(SIZES)
    h, built = _profiled(eng, g, lambda: _prepare(eng, g, P))
    try:
        c = h.window_bits
        assert c == lib.bn254_msm_prepared_default_window_bits(len(P)) and built["p_table"] == (254 + c - 1) // c
        for n in SIZES:
            got, ran = _profiled(eng, g, lambda: _call(eng, g)(h, K[:n]))
            assert np.array_equal(got, want[n]), n
            assert [ran["p_" + s] for s in NEW] == [0, 0, 0] and [ran[s] for s in NEW] == [0, 0, 0], (n, ran)
            if n == 1:
                assert ran["plain_mul"] == 1 and ran["fold"] == 0, ran          # one segment of one term IS bn254_g*_mul_batch
            else:
                assert ran["fold"] >= 1, (n, ran)
    finally:
        h.close()


@pytest.mark.parametrize("g", [1, 2])
def test_first_names_a_range_of_the_handle(oracle, eng, prefix, g):
    """first in {0, 1, 100}: up to the very end of the handle (first + n == count) against bn254_g{1,2}_msm on the same raw points, three
    terms against the oracle; one term more is BN254_E_BAD_ARG, and so is a first past the end"""
    from bn_amd import _native
    P, K, _ = prefix[g]
    msm = eng.g1_msm if g == 1 else eng.g2_msm
    h = _prepare(eng, g, P, 8)
    try:
        for first in (0, 1, 100):
            n = len(P) - first
            ref = msm(P[first:], K[:n])                                        # default options: the parent's route
            with eng.options(msm_bucket_min=0):
                assert np.array_equal(_call(eng, g)(h, K[:n], first), ref), first
                assert np.array_equal(_call(eng, g)(h, K[:3], first), _want(oracle, g, P[first:first + 3], K[:3])), first
                assert np.array_equal(_call(eng, g)(h, K[:0], len(P)), _zero(oracle, g))
            assert np.array_equal(_call(eng, g)(h, K[:n], first), ref), first       # the small route reads the same range
            for opts in ({}, {"msm_bucket_min": 0}):
                with eng.options(**opts):
                    with pytest.raises(_native.Bn254Error, match="-2"):
                        _call(eng, g)(h, K[:n + 1] if first else np.concatenate([K, K[:1]]), first)
        with pytest.raises(_native.Bn254Error, match="-2"):
            _call(eng, g)(h, K[:0], len(P) + 1)
        other = _prepare(eng, 3 - g, np.zeros((0, 12 * (3 - g)), np.uint64))    # a handle of the other group (of zero points: legal)
        assert (other.count, other.group, other.device_bytes) == (0, 3 - g, 0)
        with pytest.raises(_native.Bn254Error, match="-2"):
            _call(eng, g)(other, K[:0])
        assert np.array_equal((eng.g2_msm_prepared if g == 1 else eng.g1_msm_prepared)(other, K[:0]), _zero(oracle, 3 - g))
        other.close()
    finally:
        h.close()


@pytest.mark.parametrize("g", [1, 2])
def test_export_is_the_oracles_table(oracle, eng, points, g):
    """five points, the middle one at infinity (z = 0 under stale x, y), c = 13: entry (w, i) is the record of normalize(2^(13 w) P_i) -
    packed by the host simulation's aff_record_pack from the ORACLE's coordinates -, flagged exactly for the point at infinity"""
    c, W = 13, 20
    P = points[g][:5].copy()
    P[2, 8 * g:] = 0
    mul, norm = (oracle.g1_mul_batch, oracle.g1_normalize) if g == 1 else (oracle.g2_mul_batch, oracle.g2_normalize)
    h = _prepare(eng, g, P, c)
    try:
        got = h.export()
        assert got.shape == (W, 5, g, 20) and got.dtype == np.uint32
        hs = L.lib()
        for w in range(W):
            multiples = mul(P, E.fr(oracle, [1 << (c * w)] * 5))
            for i in range(5):
                q = canon_infinity(norm(multiples[i])[None])[0]
                inf = not q[8 * g:].any()
                assert inf == (i == 2)
                rec = np.zeros((g, 20), np.uint32)
                for comp in range(g):
                    x, y = np.ascontiguousarray(q[4 * comp:4 * comp + 4]), np.ascontiguousarray(q[4 * g + 4 * comp:4 * g + 4 * comp + 4])
                    hs.hsp_record(L.p32(x), L.p32(y), 1 if inf else 0, L.p32(rec), comp)
                assert np.array_equal(got[w, i], rec), (w, i)
        assert (got[:, 2, :, 18] != 0).all() and (got[:, [0, 1, 3, 4], :, 18] == 0).all() and (got[..., 19] == 0).all()
    finally:
        h.close()


def _crafted(c):
    W, half = (254 + c - 1) // c, 1 << (c - 1)
    below_r = lambda d: sum(d << (c * w) for w in range(W)) & ((1 << 253) - 1)
    return [0, 1, R - 1, 1 << 253, below_r(half), below_r(half + 1), (1 << (c * (W - 1))) - 1]


@pytest.mark.parametrize("c", [5, 13, 16])
@pytest.mark.parametrize("g", [1, 2])
def test_crafted_scalars(oracle, eng, points, g, c):
    """0, 1, r - 1, 2^253, every digit exactly 2^(c-1) (kept, no carry), every digit 2^(c-1) + 1 (every window carries), every window but
    the top one full: each alone, each beside a random term, and all in one call; an all-zero scalar vector gives (0, 1, 0).  c = 16 is
    the width every handle of the default width has"""
    rng = np.random.default_rng(2920 + g + c)
    ks = _crafted(c)
    P = points[g][rng.integers(0, 512, len(ks) + 1)]
    rnd = int.from_bytes(rng.bytes(40), "little") % R
    h = _prepare(eng, g, P, c)
    try:
        with eng.options(msm_bucket_min=0):
            for i, k in enumerate(ks):
                K = E.fr(oracle, [k])
                assert np.array_equal(_call(eng, g)(h, K, i), _want(oracle, g, P[i:i + 1], K)), hex(k)
                K = E.fr(oracle, [k, rnd])
                assert np.array_equal(_call(eng, g)(h, K, i), _want(oracle, g, P[i:i + 2], K)), hex(k)
            K = E.fr(oracle, ks)
            assert np.array_equal(_call(eng, g)(h, K), _want(oracle, g, P[:len(ks)], K))
            assert np.array_equal(_call(eng, g)(h, E.fr(oracle, [0] * 5)), _zero(oracle, g))
    finally:
        h.close()


@pytest.mark.parametrize("g", [1, 2])
def test_collisions_inside_a_bucket(oracle, eng, points, g):
    """ONE handle holds the same point several times, P beside -P and points at infinity; `first` picks the case.  Equal records meet in
    a bucket (the doubling branch of the mixed addition), P and -P cancel there, flagged records are skipped."""
    rng = np.random.default_rng(2930 + g)
    zero = _zero(oracle, g)
    k, s = (int.from_bytes(rng.bytes(40), "little") % R for _ in range(2))
    pts = points[g]
    neg = (eng.g1_add_batch if g == 1 else eng.g2_add_batch)(zero[None], pts[:1], negate_b=True)[0]          # -P, the reference's own limbs
    cases = [(f"the same point {t} times, one scalar", [pts[0]] * t, [k] * t, False) for t in (2, 3, 5)]
    cases += [
        ("P and -P, one scalar", [pts[0], neg], [k, k], True),
        ("P and -P, then a term in other buckets", [pts[0], neg, pts[1]], [k, k, s], False),
        ("P k + P (r - k)", [pts[0], pts[0]], [k, R - k], True),
        ("points at infinity sprinkled in", [zero, pts[0], zero, pts[1], pts[2], zero], [k, s, s, k, s, k], False),
        ("only points at infinity", [zero, zero, zero], [k, s, k], True),
        ("a list whose total is zero", [pts[0], pts[1], pts[0], pts[1]], [k, s, R - k, R - s], True),
    ]
    H = np.stack([p for _, P, _, _ in cases for p in P])
    h = _prepare(eng, g, H, 8)
    try:
        with eng.options(msm_bucket_min=0):
            first = 0
            for name, P, ks, inf in cases:
                P = np.stack(P); K = E.fr(oracle, ks)
                got = _call(eng, g)(h, K, first)
                assert np.array_equal(got, _want(oracle, g, P, K)), name
                assert np.array_equal(got, zero) == inf, name
                first += len(P)
            assert first == h.count
    finally:
        h.close()
    # the skew case: one scalar, every term in one bucket per window - device against device (n > 600 for G1)
    n = 1000 if g == 1 else 300
    P = pts[rng.integers(0, 512, n)]
    K = E.fr(oracle, [k] * n)
    h = _prepare(eng, g, P, 8)
    try:
        with eng.options(msm_bucket_min=0):
            got = _call(eng, g)(h, K)
        assert np.array_equal(got, _batch(eng, g, P, K))
        if n <= 600:
            assert np.array_equal(got, _want(oracle, g, P, K))
    finally:
        h.close()


@pytest.mark.parametrize("n", [64, 65, 200])
@pytest.mark.parametrize("g", [1, 2])
def test_chunk_seams(eng, prefix, oracle, g, n):
    """msm_chunk = 64: one full pass, a pass of one term behind it, four passes - all into the same buckets and the one tail"""
    P, K, want = prefix[g]
    for c in (5, 13):
        h = _prepare(eng, g, P, c)
        try:
            with eng.options(msm_bucket_min=0, msm_chunk=64):
                got, ran = _profiled(eng, g, lambda: _call(eng, g)(h, K[:n]))
        finally:
            h.close()
        assert ran["p_digits"] == (n + 63) // 64 and ran["p_bucket"] == (n + 63) // 64 and ran["p_reduce"] == 1, ran
        assert np.array_equal(got, want[n] if n in want else _want(oracle, g, P[:n], K[:n])), (n, c)


@pytest.mark.parametrize("g", [1, 2])
def test_device_entries_on_a_side_stream(eng, te, prefix, g):
    """prepare_dev and msm_prepared_dev on a side stream, n == 0 (NULL scalars) included"""
    import torch
    P, K, want = prefix[g]
    n = 257
    dP, dK = _dev(te, P[:n]), _dev(te, K[:n])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=te.device)
    prep = eng.g1_msm_prepare_dev if g == 1 else eng.g2_msm_prepare_dev
    f = eng.g1_msm_prepared_dev if g == 1 else eng.g2_msm_prepared_dev
    with eng.options(msm_bucket_min=0):
        with torch.cuda.stream(side):
            h = prep(dP.data_ptr(), n, 5, side.cuda_stream)
            out = te.empty(1, P.shape[1])
            f(h, 0, dK.data_ptr(), n, out.data_ptr(), side.cuda_stream)
            out0 = te.empty(1, P.shape[1])
            f(h, 0, 0, 0, out0.data_ptr(), side.cuda_stream)                      # no terms: NULL k is fine
            out1 = te.empty(1, P.shape[1])
            f(h, 256, dK.data_ptr(), 1, out1.data_ptr(), side.cuda_stream)
        side.synchronize()
    assert (h.count, h.group, h.window_bits) == (n, g, 5)
    assert np.array_equal(_host(out)[0], want[n])
    assert np.array_equal(_host(out0)[0], want[0])
    assert np.array_equal(_host(out1)[0], (eng.g1_mul_batch if g == 1 else eng.g2_mul_batch)(P[256:257], K[:1])[0])
    h.close()


@pytest.mark.parametrize("g", [1, 2])
def test_two_streams_with_two_handles(eng, te, prefix, g):
    """two streams of one context issue calls against different handles, interleaved; the workspace is shared and ordered by the context,
    every result is its own"""
    import torch
    P, K, want = prefix[g]
    A, B = P[:130], P[127:257][::-1].copy()
    msm = eng.g1_msm if g == 1 else eng.g2_msm
    wa, wb = msm(A, K[:130]), msm(B, K[:130])
    assert not np.array_equal(wa, wb)
    ha, hb = _prepare(eng, g, A, 8), _prepare(eng, g, B, 5)
    f = eng.g1_msm_prepared_dev if g == 1 else eng.g2_msm_prepared_dev
    dK = _dev(te, K[:130])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=te.device), torch.cuda.Stream(device=te.device)
    outs = []
    try:
        with eng.options(msm_bucket_min=0):
            for _ in range(3):
                for s, h in ((s1, ha), (s2, hb)):
                    with torch.cuda.stream(s):
                        o = te.empty(1, P.shape[1])
                        f(h, 0, dK.data_ptr(), 130, o.data_ptr(), s.cuda_stream)
                        outs.append((h is ha, o))
            s1.synchronize(); s2.synchronize()
        for is_a, o in outs:
            assert np.array_equal(_host(o)[0], wa if is_a else wb)
    finally:
        ha.close(); hb.close()


@pytest.mark.parametrize("g, n", [(1, 1 << 14), (2, 1 << 12)])
def test_mid_size_at_the_default_width(eng, te, g, n):
    """device-made distinct points (z != 1) and scalars; the prepared bucket route at the default width of the size against
    bn254_g{1,2}_msm_dev on the same raw points (default options: the parent's route at this size)"""
    import torch
    from bn_amd import _native
    from bn_amd import distributed as D
    g1, g2 = D.generator_limbs()
    kb = D.synthetic_scalars_device(te, 0, n, g - 1)
    base = te.empty(n, 12 if g == 1 else 24)
    te.e.tile_dev(_dev(te, g1 if g == 1 else g2).data_ptr(), 96 if g == 1 else 192, n, base.data_ptr(), te._stream())
    P = (te.g1_mul if g == 1 else te.g2_mul)(base, kb, normalize=False)
    k = D.synthetic_scalars_device(te, 1 << 24, (1 << 24) + n, 1)
    out, ref = te.empty(1, P.shape[1]), te.empty(1, P.shape[1])
    h = (eng.g1_msm_prepare_dev if g == 1 else eng.g2_msm_prepare_dev)(P.data_ptr(), n, None, te._stream())
    try:
        assert h.window_bits == _native.lib().bn254_msm_prepared_default_window_bits(n) and h.count == n
        with eng.options(msm_bucket_min=0):
            eng.profile(True); eng.profile_reset()
            try:
                (eng.g1_msm_prepared_dev if g == 1 else eng.g2_msm_prepared_dev)(h, 0, k.data_ptr(), n, out.data_ptr(), te._stream())
                torch.cuda.synchronize()
                ran = _scopes(eng, g)
            finally:
                eng.profile(False)
        (eng.g1_msm_dev if g == 1 else eng.g2_msm_dev)(P.data_ptr(), k.data_ptr(), n, ref.data_ptr(), te._stream())
        torch.cuda.synchronize()
    finally:
        h.close()
    assert [ran["p_" + s] for s in NEW] == [1, 1, 1] and [ran[s] for s in NEW] == [0, 0, 0], ran
    assert torch.equal(out, ref)
    w = P.shape[1] // 3
    assert _host(out)[0, 2 * w:].any()                                                # a finite point


@pytest.mark.parametrize("g", [1, 2])
def test_lifecycle_and_python_faces(eng, prefix, g):
    import bn_amd
    from bn_amd import _native
    P, K, want = prefix[g]
    G = bn_amd.G1 if g == 1 else bn_amd.G2
    prepare = bn_amd.g1_msm_prepare if g == 1 else bn_amd.g2_msm_prepare
    h = prepare(P[:65], 5, engine=eng)
    assert isinstance(h, bn_amd.PreparedMSM) and h.count == 65
    with eng.options(msm_bucket_min=0):
        assert np.array_equal(h.msm(K[:65]).limbs, want[65])                          # an (n,4) array
        ks = [bn_amd.Fr.from_limbs(k) for k in K[:64]]
        assert isinstance(h.msm(ks), G) and np.array_equal(h.msm(ks).limbs, want[64])
        assert h.msm([]) == G.zero()
    assert np.array_equal(h.msm(ks[:3]).limbs, want[3])                               # default options: the small route, the same bytes
    h.close(); h.close()                                                              # twice is harmless
    for use in (lambda: h.count, lambda: h.msm(ks), h.export, lambda: _call(eng, g)(h, K[:2])):
        with pytest.raises(_native.Bn254Error, match="closed"):
            use()
    h2 = prepare([G(p) for p in P[:3]], engine=eng)                                   # a sequence of points, the default width
    assert np.array_equal(h2.msm(ks[:3]).limbs, want[3])
    del h2
