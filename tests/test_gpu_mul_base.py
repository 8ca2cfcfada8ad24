"""Fixed-base scalar multiplication on an MI355X (run with -m gpu): bn254_g{1,2}_mul_base_batch, their _dev entry points and the Python
faces.  Small cases are compared with the oracle (oracle.g{1,2}_mul_batch on the tiled base, the point at infinity as G::zero():
conftest.canon_infinity), large ones device against device with bn254_g{1,2}_mul_batch on the tiled base, whose bytes the call is defined
to return.

One scalar beyond the issue's list: k = r - 2 (r mod 2^(c (W - 1))).  Going low window to high, the partial sum never equals +- the entry
that is added AS AN INTEGER, but mod r the top window can wrap: for that k the signed recoding gives the partial sum -t B (t = r mod
2^(c (W - 1))) and the top entry (r - t) B - the same point, so the last addition is a doubling.  The kernels therefore keep the complete
mixed addition, and test_edge_scalars holds that scalar for every width of the sweep."""
import ctypes as C

import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
from conftest import canon_infinity

pytestmark = pytest.mark.gpu

R = M.R_ORD


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def te(eng):
    import torch
    from bn_amd import distributed as D
    return D.TorchEngine(eng, torch.device("cuda", 0))


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_mul_base_window.argtypes = [C.c_int]; l.bn254_mul_base_window.restype = C.c_uint
    l.bn254_mul_base_slots.argtypes = []; l.bn254_mul_base_slots.restype = C.c_uint
    return l


def _dev(te, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(te.device)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _one(oracle, g):
    return oracle.g1_one() if g == 1 else oracle.g2_one()


def _want(oracle, g, base, K):
    """the oracle: Mul<Fr> of the tiled base, normalized, infinity as (0, 1, 0)"""
    mul = oracle.g1_mul_batch if g == 1 else oracle.g2_mul_batch
    return canon_infinity(mul(np.tile(base, (len(K), 1)), K))


def _mul_base(eng, g):
    return eng.g1_mul_base_batch if g == 1 else eng.g2_mul_base_batch


def _mul(eng, g, base, K):
    """the parent's way: the general kernel on the tiled base"""
    return (eng.g1_mul_batch if g == 1 else eng.g2_mul_batch)(np.tile(base, (len(K), 1)), K)


def _edge_values(c):
    W = (254 + c - 1) // c
    vals = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
    for j in range(1, 254):
        vals += [v for v in ((1 << j) - 1, 1 << j, (1 << j) + 1) if v < R]
    for d in ((1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1):          # the carry chains of the signed recoding
        vals.append(sum(d << (c * w) for w in range(W)) & ((1 << 253) - 1))
    for cc in (8, 10, 12, c):                                                                # the top window wraps mod r: a doubling (see above)
        vals.append(R - 2 * (R % (1 << (cc * ((254 + cc - 1) // cc - 1)))))
    rng = np.random.default_rng(2024)
    vals += [int.from_bytes(rng.bytes(40), "little") % R for _ in range(64)]
    return vals


@pytest.fixture(scope="module")
def edge(oracle, lib):
    """{g: (K, want)} for base = one(): about 850 scalars, the oracle side computed once"""
    out = {}
    for g in (1, 2):
        K = E.fr(oracle, _edge_values(lib.bn254_mul_base_window(g)))
        out[g] = (K, _want(oracle, g, _one(oracle, g), K))
    return out


@pytest.fixture(scope="module")
def points(oracle, te):
    """{g: 8 random subgroup points with z != 1}: the reference's own chain on the device, as the other GPU tests make them"""
    import torch
    rng = np.random.default_rng(77)
    out = {}
    for g in (1, 2):
        k = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") for _ in range(8)])
        P = _host((te.g1_mul if g == 1 else te.g2_mul)(_dev(te, np.tile(_one(oracle, g), (8, 1))), _dev(te, k), normalize=False))
        torch.cuda.synchronize()
        w = P.shape[1] // 3
        assert not np.array_equal(P[0, 2 * w:2 * w + 4], oracle.fp_from_int(E.FQ, 1))            # really z != 1
        out[g] = P
    return out


@pytest.fixture(scope="module")
def k70(oracle):
    rng = np.random.default_rng(70)
    return E.fr(oracle, [0, 1, R - 1] + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(67)])


@pytest.mark.parametrize("g", [1, 2])
def test_edge_scalars(eng, edge, g, oracle):
    K, want = edge[g]
    assert 800 < len(K) < 900
    got = _mul_base(eng, g)(_one(oracle, g), K)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad[:10]
    assert np.array_equal(got[0], oracle.g1_zero() if g == 1 else oracle.g2_zero())                # k = 0


@pytest.mark.parametrize("g", [1, 2])
def test_base_forms(eng, oracle, points, k70, g):
    P = points[g][0]
    want = _want(oracle, g, P, k70)
    assert np.array_equal(_mul_base(eng, g)(P, k70), want)                                       # z != 1
    neg = (oracle.g1_neg if g == 1 else oracle.g2_neg)(P)
    assert np.array_equal(_mul_base(eng, g)(neg, k70), _want(oracle, g, neg, k70))
    other = E.rescale_g1(oracle, P, 0x1234567) if g == 1 else E.rescale_g2(oracle, P, (3, 7))    # the same element, another representation
    assert not np.array_equal(other, P)
    assert np.array_equal(_mul_base(eng, g)(other, k70), want)
    zero = oracle.g1_zero() if g == 1 else oracle.g2_zero()
    for inf in (zero, np.concatenate([P[:2 * len(P) // 3], np.zeros(len(P) // 3, np.uint64)])):  # (0, 1, 0) and (x, y, 0)
        assert np.array_equal(_mul_base(eng, g)(inf, k70), np.tile(zero, (len(k70), 1)))


@pytest.mark.parametrize("g", [1, 2])
def test_device_against_device_at_size(eng, te, points, g):
    from bn_amd import distributed as D
    n = ((1 << 16) if g == 1 else (1 << 15)) + 37
    K = _host(D.synthetic_scalars_device(te, 0, n, g - 1))
    base = points[g][1]
    assert np.array_equal(_mul_base(eng, g)(base, K), _mul(eng, g, base, K))


@pytest.mark.parametrize("g", [1, 2])
def test_a_call_across_the_launch_cut(eng, te, points, g):
    """calls are cut into sub-launches of 2^22 scalars (BN_LAUNCH_MAX): one _dev call of 2^22 + 1, compared on the device"""
    import torch
    from bn_amd import distributed as D
    n = (1 << 22) + 1
    base = points[g][2]
    k = D.synthetic_scalars_device(te, 0, n, g - 1)
    got = (te.g1_mul_base if g == 1 else te.g2_mul_base)(base, k)
    tiled, one = te.empty(n, len(base)), _dev(te, base)
    eng.tile_dev(one.data_ptr(), 8 * len(base), n, tiled.data_ptr(), te._stream())
    want = (te.g1_mul if g == 1 else te.g2_mul)(tiled, k)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(got[-1:].cpu(), want[-1:].cpu())                                          # the one scalar of the second sub-launch


@pytest.mark.parametrize("g", [1, 2])
def test_cache(lib, oracle, points, g):
    import bn_amd
    eng = bn_amd.Engine(0)                                                                       # a context that has seen no base yet
    slots = lib.bn254_mul_base_slots()
    bases = points[g][:slots + 2]
    assert len(bases) == slots + 2 and len({b.tobytes() for b in bases}) == slots + 2
    rng = np.random.default_rng(33)
    K = E.fr(oracle, [int.from_bytes(rng.bytes(40), "little") % R for _ in range(33)])
    order = [0, 1, 0, 2, 3, 4, 5, 0]                                                             # A, B, A, C, D, E, F, A
    want = {i: _mul(eng, g, bases[i], K) for i in set(order)}
    other = bn_amd.Engine(0)
    lru = []                                                                                     # the model: least recently used first
    eng.profile(True); eng.profile_reset()
    try:
        built = 0
        for i in order:
            got = _mul_base(eng, g)(bases[i], K)
            assert np.array_equal(got, want[i]), i
            assert np.array_equal(_mul_base(other, g)(bases[i], K), got), i
            now = eng.kernel_stats(f"g{g}_base_table")[1]
            if i in lru:
                assert now == built, (i, "a cached base built a table")
                lru.remove(i)
            else:
                assert now >= built + 1, (i, "a new base built nothing")
                if len(lru) == slots:
                    lru.pop(0)
            lru.append(i)
            built = now
        assert eng.kernel_stats(f"g{g}_mul_base")[1] == len(order)
    finally:
        eng.profile(False)
        other.close(); eng.close()


@pytest.mark.parametrize("g", [1, 2])
def test_dev_reads_the_base_before_it_returns(eng, te, oracle, points, k70, g):
    import torch
    a, b = points[g][6], points[g][7]
    want = _mul(eng, g, a, k70)
    k = _dev(te, k70)
    buf = a.copy()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(te.device)
    with torch.cuda.stream(s):
        assert te._stream() == s.cuda_stream and s.cuda_stream != 0
        out = (te.g1_mul_base if g == 1 else te.g2_mul_base)(buf, k)
        buf[:] = b                                                                               # before the stream is synchronised
    s.synchronize()
    assert np.array_equal(_host(out), want)


@pytest.mark.parametrize("rotate", [2, 5])
@pytest.mark.parametrize("g", [1, 2])
def test_two_streams_on_one_context(eng, te, lib, oracle, points, k70, g, rotate):
    """two streams alternating two bases, 8 calls each (rotate = 2: every call after the first two is a hit); rotate = slots + 1 bases: every
    call rebuilds a slot that the other stream's launch may still be reading"""
    import torch
    assert rotate in (2, lib.bn254_mul_base_slots() + 1)
    bases = points[g][:rotate]
    want = [_mul(eng, g, b, k70) for b in bases]
    k = _dev(te, k70)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(te.device), torch.cuda.Stream(te.device)]
    outs = []
    for call in range(8):
        for j, s in enumerate(streams):
            i = (call + j) % rotate
            with torch.cuda.stream(s):
                outs.append((i, (te.g1_mul_base if g == 1 else te.g2_mul_base)(bases[i], k)))
    for s in streams:
        s.synchronize()
    assert len(outs) == 16
    for i, out in outs:
        assert np.array_equal(_host(out), want[i]), i


def test_faces(eng, te, oracle, edge):
    import torch
    import bn_amd
    for g, G, f in ((1, bn_amd.G1, bn_amd.g1_mul_base), (2, bn_amd.G2, bn_amd.g2_mul_base)):
        K, want = edge[g]
        K, want = K[:16], want[:16]
        ks = [bn_amd.Fr.from_limbs(k) for k in K]
        assert np.array_equal(np.stack([k.limbs for k in ks]), K)
        for got in (f(G.one(), ks), f(G.one(), ks, engine=eng), G.one().mul_base(ks), f(G.one().limbs, K)):
            assert [type(p) for p in got] == [G] * 16
            assert np.array_equal(np.stack([p.limbs for p in got]), want)
        out = (te.g1_mul_base if g == 1 else te.g2_mul_base)(_one(oracle, g), _dev(te, K))
        torch.cuda.synchronize()
        assert np.array_equal(_host(out), want)
        assert f(G.one(), []) == []
