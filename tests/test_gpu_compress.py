"""The compressed G1 / G2 encodings on an MI355X (run with -m gpu): bn254_g{1,2}_compress_batch, bn254_g{1,2}_decompress_batch and their _dev
twins against the integer model of compress_cases.py - every case in both layouts, the sizes around a wave, waves that are rejected whole and
in one lane, the seam between sub-launches - and against the uncompressed wire format byte for byte."""
import ctypes as C
import threading

import numpy as np
import pytest

import compress_cases as CC

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257]
FMTS = sorted(CC.FORMATS)
WORDS = {1: 12, 2: 24}


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_compress_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def points(eng):
    """per group: random points (normalised), raw Jacobian sums of neighbours, a cancelling sum and the point at infinity - made once"""
    import bn_amd
    rng = np.random.default_rng(77)
    out = {}
    for g, count, one, zero, mul, add in ((1, 200, bn_amd.G1.one(), bn_amd.G1.zero(), eng.g1_mul_batch, eng.g1_add_batch),
                                          (2, 100, bn_amd.G2.one(), bn_amd.G2.zero(), eng.g2_mul_batch, eng.g2_add_batch)):
        k = np.stack([bn_amd.Fr.random(rng).limbs for _ in range(count)])
        P = mul(np.tile(one.limbs, (count, 1)), k)
        sums = add(P[:-1], P[1:])                                               # Jacobian, z != 1
        doubles = add(P[:8], P[:8])
        cancel = add(P[:2], P[:2], negate_b=True)                               # infinity as the addition leaves it
        assert (sums[:, 2 * WORDS[g] // 3:] != P[:-1, 2 * WORDS[g] // 3:]).any()
        out[g] = np.concatenate([P, sums, doubles, cancel, zero.limbs[None]])
    return out


def _fns(eng, g):
    return ((eng.g1_compress_batch, eng.g1_decompress_batch, eng.g1_compress_batch_dev, eng.g1_decompress_batch_dev, eng.g1_encode_batch, eng.g1_decode_batch) if g == 1 else
            (eng.g2_compress_batch, eng.g2_decompress_batch, eng.g2_compress_batch_dev, eng.g2_decompress_batch_dev, eng.g2_encode_batch, eng.g2_decode_batch))


def _dev_decompress(eng, g, b, fmt, stream=None):
    """the _dev form: records up, points and statuses stay on the device until the call is over"""
    import torch
    n = b.shape[0]
    d_in = torch.from_numpy(np.ascontiguousarray(b).reshape(-1).copy()).to("cuda:0")
    d_out = torch.full((n * WORDS[g],), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    fn = _fns(eng, g)[3]
    if stream is None:
        fn(d_in.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), n, fmt)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            fn(d_in.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), n, fmt, stream=stream.cuda_stream)
        stream.synchronize()
    return d_out.cpu().numpy().view(np.uint64).reshape(n, WORDS[g]), d_st.cpu().numpy()


def _dev_compress(eng, g, p, fmt, stream=None):
    import torch
    n = p.shape[0]
    d_in = torch.from_numpy(np.ascontiguousarray(p).view(np.int64).reshape(-1).copy()).to("cuda:0")
    d_out = torch.full((n * 32 * g,), 0xa5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    fn = _fns(eng, g)[2]
    if stream is None:
        fn(d_in.data_ptr(), d_out.data_ptr(), n, fmt)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            fn(d_in.data_ptr(), d_out.data_ptr(), n, fmt, stream=stream.cuda_stream)
        stream.synchronize()
    return d_out.cpu().numpy().reshape(n, 32 * g)


def _check(got, want, what):
    (gp, gs), (wb, ws, wp) = got, want
    assert gs.dtype == np.int32 and gs.tolist() == ws.tolist(), (what, np.flatnonzero(gs != ws)[:8], gs[gs != ws][:8], ws[gs != ws][:8])
    assert gp.shape == wp.shape and gp.tobytes() == wp.tobytes(), (what, np.flatnonzero((gp != wp).any(axis=1))[:8])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("g", [1, 2])
def test_every_case_through_both_forms(eng, g, fmt):
    recs = CC.records(g, CC.FORMATS[fmt])
    want = CC.batch(g, CC.FORMATS[fmt], len(recs))
    _check(_fns(eng, g)[1](want[0], fmt), want, "host buffers")
    _check(_dev_decompress(eng, g, want[0], fmt), want, "_dev")
    assert set(want[1].tolist()) == ({0, 1, 3, 4} if g == 1 else {0, 1, 3, 4, 5})
    # compress(decompress(b)) == b on the accepted records, through both forms
    ok = want[1] == 0
    assert _fns(eng, g)[0](want[2][ok], fmt).tobytes() == want[0][ok].tobytes()
    assert _dev_compress(eng, g, want[2][ok], fmt).tobytes() == want[0][ok].tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("g", [1, 2])
def test_sizes_around_a_wave(eng, g, fmt, n):
    want = CC.batch(g, CC.FORMATS[fmt], n, start=n)
    _check(_fns(eng, g)[1](want[0], fmt), want, n)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("g", [1, 2])
def test_a_wave_rejected_whole_and_a_wave_with_one_rejected_lane(eng, g, fmt):
    f = CC.FORMATS[fmt]
    good, bad = CC.accepted(g, f), CC.rejected(g, f)
    rows = [good[i % len(good)] for i in range(64)] + [bad[i % len(bad)] for i in range(64)] + [good[(i + 3) % len(good)] for i in range(64)]
    rows[128 + 37] = bad[5 % len(bad)]                                           # the third wave: exactly one lane is rejected
    b = np.stack([np.frombuffer(r[1], np.uint8) for r in rows])
    want = (b, np.array([r[2] for r in rows], np.int32), np.stack([CC.words(g, r[3]) for r in rows]))
    assert (want[1][64:128] != 0).all() and np.flatnonzero(want[1][128:]).tolist() == [37] and not want[1][:64].any()
    _check(_fns(eng, g)[1](b, fmt), want, "host buffers")
    _check(_dev_decompress(eng, g, b, fmt), want, "_dev")


@pytest.mark.parametrize("g", [1, 2])
def test_the_seam_between_sub_launches(eng, lib, g):
    want = CC.batch(g, CC.ARK, 150, start=7)                                      # sub-launches of 64, 64 and 22 records
    try:
        assert lib.bn254_compress_set_launch_max(64) == 0
        got = _fns(eng, g)[1](want[0], "ark")
        dev = _dev_decompress(eng, g, want[0], "ark")
        ok = want[1] == 0
        back = _fns(eng, g)[0](want[2][ok], "ark")
    finally:
        assert lib.bn254_compress_set_launch_max(0) == 0
    _check(got, want, "host buffers"); _check(dev, want, "_dev")
    assert back.tobytes() == want[0][ok].tobytes()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("g", [1, 2])
def test_round_trip_equals_the_uncompressed_wire_format(eng, points, g, fmt):
    """decompress(compress(p)) == decode(encode(p)) byte for byte, for normalised points, raw Jacobian sums and infinity"""
    comp, decomp, _, _, enc, dec = _fns(eng, g)
    P = points[g]
    want, st0 = dec(enc(P))
    assert not st0.any()
    b = comp(P, fmt)
    got, st = decomp(b, fmt)
    assert not st.any() and got.tobytes() == want.tobytes()
    assert comp(got, fmt).tobytes() == b.tobytes()                                # canonical: the normalised image compresses to the same bytes
    assert not got[-1, 2 * WORDS[g] // 3:].any() and not got[-2, 2 * WORDS[g] // 3:].any()           # both infinities
    assert b[-1].tobytes() == b[-2].tobytes() == CC.compress(g, None, CC.FORMATS[fmt])
    # a flipped sign bit is the negative: y differs, x does not
    flipped = b.copy()
    if fmt == "ark":
        flipped[:-3, -1] ^= 0x80
    else:
        flipped[:-3, 0] ^= 0x40
    neg, st = decomp(flipped, fmt)
    w = WORDS[g] // 3
    assert not st.any() and neg[:-3, :w].tobytes() == got[:-3, :w].tobytes() and (neg[:-3, w:2 * w] != got[:-3, w:2 * w]).any(axis=1).all()


@pytest.mark.parametrize("g", [1, 2])
def test_the_dev_forms_on_a_stream_of_their_own(eng, points, g):
    import torch
    stream = torch.cuda.Stream()
    want = CC.batch(g, CC.GNARK, 130, start=3)
    _check(_dev_decompress(eng, g, want[0], "gnark", stream), want, "decompress on a stream")
    P = points[g][:70]
    assert _dev_compress(eng, g, P, "gnark", stream).tobytes() == _fns(eng, g)[0](P, "gnark").tobytes()


def test_an_unknown_format_and_an_empty_batch(eng):
    from bn_amd import _native
    with pytest.raises(_native.Bn254Error):
        eng.g1_decompress_batch(np.zeros((2, 32), np.uint8), 2)
    p, st = eng.g2_decompress_batch(np.zeros((0, 64), np.uint8))
    assert p.shape == (0, 24) and st.shape == (0,)
    assert eng.g1_compress_batch(np.zeros((0, 12), np.uint64)).shape == (0, 32)


def test_two_host_threads_alternate_groups_on_one_context(eng):
    """the host-buffer calls hold the context's mutex: two threads on the one context, each with both groups, get the model's bytes"""
    wants = {(g, f): CC.batch(g, CC.FORMATS[f], 70, start=11 * g) for g in (1, 2) for f in FMTS}
    errors = []

    def work(fmt):
        try:
            for _ in range(3):
                for g in (1, 2):
                    _check(_fns(eng, g)[1](wants[(g, fmt)][0], fmt), wants[(g, fmt)], (g, fmt))
        except BaseException as e:                                                # reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(f,)) for f in FMTS]
    for t in threads: t.start()
    for t in threads: t.join(120)
    assert not any(t.is_alive() for t in threads) and not errors, errors


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import G1, G2
    rng = np.random.default_rng(3)
    p, q = G1.random(rng), G2.random(rng)
    for fmt in FMTS:
        assert len(p.to_compressed(fmt)) == 32 and len(q.to_compressed(fmt)) == 64
        assert G1.from_compressed(p.to_compressed(fmt), fmt) == p and G2.from_compressed(q.to_compressed(fmt), fmt) == q
        assert (p + p).to_compressed(fmt) == (p + p).normalize().to_compressed(fmt)
    assert G1.one().to_compressed("ark").hex() == "01" + "00" * 31 and G1.one().to_compressed("gnark").hex() == "80" + "00" * 30 + "01"
    with pytest.raises(bn_amd.DecodeError) as err:
        G2.from_compressed(CC.render(2, list(CC.g2_outside_subgroup()[0]), "sign1", CC.ARK))
    assert err.value.status == 5
