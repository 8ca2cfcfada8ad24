"""bn254_g{1,2}_msm and bn254_g{1,2}_msm_prepared the way a caller runs them, on an MI355X (run with -m gpu): options untouched (unless a case
says otherwise), at the sizes where the library itself changes route, window width and pass count.  Every result is compared byte for byte
with an expectation that shares no code with the MSM routes (tests/msm_known_logs.py): the points are [a_i] G for known a_i - made on the
device by the reference's own chain, z != 1 - so the sum is [sum a_i k_i mod r] G, one multiplication by the oracle.

The window width of the plain bucket route has no accessor; by bn_msm_window_bits (host_plan.hpp, pinned on the CPU by
tests/test_host_plan.py::test_window_width_by_size) a call of n terms with msm_window_bits unset runs at
    2^15: 9      2^16, 2^17: 11      2^18: 12      2^19: 11      2^20 and more: 14
and every prepared handle at 16 (asserted on the handle)."""
import numpy as np
import pytest

import fr_cases as FC
import msm_known_logs as KL
from bn_oracle import FQ
from test_gpu_msm_bucket import _dev, _host, eng, te  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

R = KL.R
NEW = ("digits", "bucket", "reduce")
FIRST = 4096                                           # the second start the G1 set carries a cluster of special terms for
SET = {1: (1 << 20) + 1000, 2: 1 << 18}                 # points per group: the largest call of the group
PLAIN_MIN_G2 = 1 << 18                                 # BN_MSM_BUCKET_MIN_DEFAULT_G2 (host_ctx.hpp): the plain G2 crossover has no accessor


def _plain_min(eng, g):
    return eng.get_option("msm_bucket_min") if g == 1 else PLAIN_MIN_G2


def _prepared_min(g):
    from bn_amd import _native
    return _native.lib().bn254_msm_prepared_default_min(g)


def _scopes(eng, g):
    s = {"p_" + n: eng.kernel_stats(f"g{g}_msmp_{n}")[1] for n in NEW + ("table",)}
    s.update({n: eng.kernel_stats(f"g{g}_msm_{n}")[1] for n in NEW + ("fold",)})
    return s


@pytest.fixture(scope="module")
def sets(oracle, eng, te):
    """{g: (logs, P)}: SET[g] points [a_i] G on the device, Jacobian with z != 1 (a_i = 0: z = 0), and their logarithms; G is the oracle's
    generator, the one the expectation multiplies"""
    import torch
    gen = {1: oracle.g1_one(), 2: oracle.g2_one()}
    out = {}
    for g in (1, 2):
        n = SET[g]
        logs = KL.Logs(np.random.default_rng(3200 + g), n, starts=(0, FIRST) if g == 1 else (0,), seams=(KL.CHUNK,) if g == 1 else ())
        a = _dev(te, KL.montgomery(eng, logs.words))
        base = te.empty(n, 12 * g)
        te.e.tile_dev(_dev(te, gen[g]).data_ptr(), 96 * g, n, base.data_ptr(), te._stream())
        P = (te.g1_mul if g == 1 else te.g2_mul)(base, a, normalize=False)
        torch.cuda.synchronize()
        head = _host(P[:2])
        w = P.shape[1] // 3
        assert head[0, 2 * w:].any() and not np.array_equal(head[0, 2 * w:2 * w + 4], oracle.fp_from_int(FQ, 1))          # really z != 1
        assert not head[1, 2 * w:].any()                                # a = 0: infinity as the chain leaves it
        out[g] = (logs, P)
    return out


def _check(oracle, eng, te, sets, g, lo, n, seed, call):
    """one profiled call over terms [lo, lo + n) of the set: the bytes of the known-logs expectation, a finite point; -> the scope counts"""
    import torch
    logs, P = sets[g]
    k, special = KL.draw_scalars(np.random.default_rng(seed), logs, lo, n)
    assert {0, n - 1} <= set(special)
    want = KL.expected(oracle, g, KL.host_sum(logs, lo, k))
    dk = _dev(te, KL.montgomery(eng, k))
    out = te.empty(1, P.shape[1])
    torch.cuda.synchronize()
    eng.profile(True); eng.profile_reset()
    try:
        call(P[lo:].data_ptr(), dk.data_ptr(), n, out.data_ptr(), te._stream())
        torch.cuda.synchronize()
        ran = _scopes(eng, g)
    finally:
        eng.profile(False)
    got = _host(out)[0]
    print(f"g{g} lo={lo} n={n}: {ran}")
    assert np.array_equal(got, want), (g, lo, n, ran)
    assert got[2 * (P.shape[1] // 3):].any(), "the point at infinity"
    return ran


def _prepare(eng, te, sets, g, count):
    """-> (handle over the first `count` points of the set at the default width, scope counts of the build)"""
    import torch
    from bn_amd import _native
    _, P = sets[g]
    eng.profile(True); eng.profile_reset()
    try:
        h = (eng.g1_msm_prepare_dev if g == 1 else eng.g2_msm_prepare_dev)(P.data_ptr(), count, None, te._stream())
        torch.cuda.synchronize()
        built = _scopes(eng, g)
    finally:
        eng.profile(False)
    try:
        c = h.window_bits
        assert c == _native.lib().bn254_msm_prepared_default_window_bits(count) and h.count == count
        assert built["p_table"] == (254 + c - 1) // c
        assert h.device_bytes == (254 + c - 1) // c * count * 80 * g + count * 96 * g
    except BaseException:
        h.close()
        raise
    print(f"g{g} handle of {count} points: width {c}, {h.device_bytes} bytes")
    return h


def _prepared_call(eng, g, h, first=0):
    f = eng.g1_msm_prepared_dev if g == 1 else eng.g2_msm_prepared_dev
    return lambda p, k, n, out, s: f(h, first, k, n, out, s)


def test_wire_convention_on_edge_values(eng):
    """the records the known-logs helper hands to fr_decode_batch decode to the Montgomery rows of the same integers"""
    vals = [0, 1, R - 1]
    rows, st = eng.fr_decode_batch(KL.wire(KL.to_words(vals)))
    assert list(st) == [0, 0, 0] and np.array_equal(rows, FC.rows(vals))
    assert np.array_equal(KL.montgomery(eng, KL.to_words(vals)), FC.rows(vals))


@pytest.mark.parametrize("below", [True, False])
@pytest.mark.parametrize("g", [1, 2])
def test_crossover_plain(oracle, eng, te, sets, g, below):
    """n == crossover - 1: the segmented route (no bucket scope, the fold ran); n == crossover: digits, bucket and reduce once each - width 11
    (G1, 2^19) and 12 (G2, 2^18)"""
    assert eng.get_option_raw("msm_bucket_min") is None and eng.get_option_raw("msm_window_bits") is None and eng.get_option_raw("msm_chunk") is None
    n = _plain_min(eng, g) - (1 if below else 0)
    assert n + 1 >= {1: 1 << 19, 2: 1 << 18}[g] >= n
    ran = _check(oracle, eng, te, sets, g, 0, n, 3300 + 2 * g + below, eng.g1_msm_dev if g == 1 else eng.g2_msm_dev)
    assert [ran[s] for s in NEW] == ([0, 0, 0] if below else [1, 1, 1]), (n, ran)
    assert ran["fold"] >= 1 and [ran["p_" + s] for s in NEW] == [0, 0, 0], (n, ran)


@pytest.mark.parametrize("g", [1, 2])
def test_crossover_prepared(oracle, eng, te, sets, g):
    """one handle of crossover-many points at the default width (16); a call of one term less takes the small route on the handle's kept
    points (no g*_msmp_* scope), a call of all of them digits, bucket and reduce once each and no scope of the plain bucket route"""
    assert eng.get_option_raw("msm_bucket_min") is None and eng.get_option_raw("msm_chunk") is None
    m = _prepared_min(g)
    assert m == {1: 1 << 19, 2: 1 << 18}[g]
    h = _prepare(eng, te, sets, g, m)
    try:
        for n in (m - 1, m):
            ran = _check(oracle, eng, te, sets, g, 0, n, 3310 + 2 * g + (n == m), _prepared_call(eng, g, h))
            assert [ran["p_" + s] for s in NEW] == ([1, 1, 1] if n == m else [0, 0, 0]), (n, ran)
            assert [ran[s] for s in NEW] == [0, 0, 0] and ran["p_table"] == 0 and ran["fold"] >= 1, (n, ran)
    finally:
        h.close()


def test_width_14(oracle, eng, te, sets):
    """G1, 2^20 terms: the plain route at the width every larger call uses, in one pass"""
    assert eng.get_option_raw("msm_window_bits") is None and eng.get_option("msm_chunk") == 1 << 20
    ran = _check(oracle, eng, te, sets, 1, 0, 1 << 20, 3320, eng.g1_msm_dev)
    assert [ran[s] for s in NEW] == [1, 1, 1] and [ran["p_" + s] for s in NEW] == [0, 0, 0], ran


@pytest.mark.parametrize("prepared", [False, True])
def test_default_chunk_seam(oracle, eng, te, sets, prepared):
    """G1, 2^20 + 1000 terms under the default msm_chunk: two passes of digits and bucket - the second adds 1000 terms into buckets the
    first filled, P at index 2^20 - 1 and -P at 2^20 under one scalar among them - and ONE reduction; width 14 (plain) and 16 (prepared)"""
    n = (1 << 20) + 1000
    assert eng.get_option_raw("msm_chunk") is None and eng.get_option("msm_chunk") == KL.CHUNK == 1 << 20
    h = _prepare(eng, te, sets, 1, n) if prepared else None
    try:
        ran = _check(oracle, eng, te, sets, 1, 0, n, 3330 + prepared, _prepared_call(eng, 1, h) if prepared else eng.g1_msm_dev)
    finally:
        if h is not None:
            h.close()
    mine, other = ("p_", "") if prepared else ("", "p_")
    assert [ran[mine + s] for s in NEW] == [2, 2, 1] and [ran[other + s] for s in NEW] == [0, 0, 0], ran


@pytest.mark.parametrize("lg, c", [(15, 9), (16, 11)])
def test_widths_of_lowered_crossovers(oracle, eng, te, sets, lg, c):
    """G1 with msm_bucket_min = 0 and msm_window_bits unset: widths 9 and 11 at the sizes bn_msm_window_bits gives them (c: for the record)"""
    with eng.options(msm_bucket_min=0):
        assert eng.get_option_raw("msm_window_bits") is None
        ran = _check(oracle, eng, te, sets, 1, 0, 1 << lg, 3340 + lg, eng.g1_msm_dev)
    assert [ran[s] for s in NEW] == [1, 1, 1], (lg, c, ran)


def test_first_at_scale(oracle, eng, te, sets):
    """a G1 handle of 2^19 + 4096 points, calls of 2^19 terms at first = 4096 (up to the very end of the handle) and at first = 0: the sum
    over the same slice of the set"""
    n = 1 << 19
    assert n >= _prepared_min(1)
    h = _prepare(eng, te, sets, 1, n + FIRST)
    try:
        for first in (FIRST, 0):
            ran = _check(oracle, eng, te, sets, 1, first, n, 3350 + first, _prepared_call(eng, 1, h, first))
            assert [ran["p_" + s] for s in NEW] == [1, 1, 1] and [ran[s] for s in NEW] == [0, 0, 0], (first, ran)
    finally:
        h.close()
