"""Point validation on an MI355X (run with -m gpu): bn254_g1_validate_batch, bn254_g2_validate_batch and their _dev twins against the integer model
of subgroup_cases.py, whose membership is [r]P == 0 alone - every case, the sizes around a wave, the seam between sub-launches, a stream of its own,
two host threads - and against the existing wire decoder on the same device; then the Python face and bls_minpk.verify_batch(validate=True)."""
import ctypes as C
import threading

import numpy as np
import pytest

import hash_g2_cases as HC
import subgroup_cases as S

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 130]
WORDS = {1: 12, 2: 24}


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_validate_set_launch_max.argtypes = [C.c_size_t]
    return l


def _host(eng, g, rows):
    keep = rows.copy()
    st = (eng.g1_validate_batch if g == 1 else eng.g2_validate_batch)(rows)
    assert st.dtype == np.int32 and st.shape == (rows.shape[0],) and np.array_equal(rows, keep)
    return st


def _dev(eng, g, rows, stream=None):
    """the _dev form: records up, statuses stay on the device until the call is over; the records are not written"""
    import torch
    n = rows.shape[0]
    d_p = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64).reshape(-1).copy()).to("cuda:0")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    fn = eng.g1_validate_batch_dev if g == 1 else eng.g2_validate_batch_dev
    torch.cuda.synchronize()
    if stream is None:
        fn(d_p.data_ptr(), d_st.data_ptr(), n)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            fn(d_p.data_ptr(), d_st.data_ptr(), n, stream=stream.cuda_stream)
        stream.synchronize()
    assert d_p.cpu().numpy().view(np.uint64).reshape(n, WORDS[g]).tobytes() == rows.tobytes()
    return d_st.cpu().numpy()


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])


def _batch(g, n, start=0):
    return (S.g1_batch if g == 1 else S.g2_batch)(n, start)


@pytest.mark.parametrize("g", (1, 2))
def test_every_case_through_both_forms(eng, g):
    cases = S.g1_cases() if g == 1 else S.g2_cases()
    rows, want = _batch(g, len(cases))
    for form, got in (("host buffers", _host(eng, g, rows)), ("_dev", _dev(eng, g, rows))):
        bad = [(name, int(st), w) for (name, _, w), st in zip(cases, got) if st != w]
        assert not bad, (form, bad)


@pytest.mark.parametrize("g", (1, 2))
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_wave(eng, g, n):
    rows, want = _batch(g, n, start=n)
    _same(_host(eng, g, rows), want, ("host buffers", g, n))
    _same(_dev(eng, g, rows), want, ("_dev", g, n))


def test_the_seam_between_sub_launches(eng, lib):
    r1, w1 = _batch(1, 130, start=5)                                             # sub-launches of 64, 64 and 2 records
    r2, w2 = _batch(2, 130, start=9)
    try:
        assert lib.bn254_validate_set_launch_max(64) == 0
        got = (_host(eng, 1, r1), _dev(eng, 1, r1), _host(eng, 2, r2), _dev(eng, 2, r2))
    finally:
        assert lib.bn254_validate_set_launch_max(0) == 0
    _same(got[0], w1, "G1"); _same(got[1], w1, "G1 _dev"); _same(got[2], w2, "G2"); _same(got[3], w2, "G2 _dev")


def test_the_dev_forms_on_a_stream_of_their_own(eng):
    import torch
    stream = torch.cuda.Stream()
    for g in (1, 2):
        rows, want = _batch(g, 70, start=3)
        _same(_dev(eng, g, rows, stream), want, ("on a stream", g))


def test_two_host_threads_on_one_context(eng):
    """the host-buffer calls hold the context's mutex: two threads on the one context get the model's statuses"""
    r1, w1 = _batch(1, 70, start=1)
    r2, w2 = _batch(2, 70, start=2)
    errors = []

    def work(order):
        try:
            for _ in range(2):
                for g in order:
                    _same(_host(eng, g, r1 if g == 1 else r2), w1 if g == 1 else w2, ("thread", g))
        except BaseException as e:                                                # reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(o,)) for o in ((1, 2), (2, 1))]
    for t in threads: t.start()
    for t in threads: t.join(120)
    assert not any(t.is_alive() for t in threads) and not errors, errors


def test_an_empty_batch_and_the_error_paths(eng):
    assert eng.g1_validate_batch(np.zeros((0, 12), np.uint64)).shape == (0,) and eng.g2_validate_batch(np.zeros((0, 24), np.uint64)).shape == (0,)
    eng.g1_validate_batch_dev(None, None, 0); eng.g2_validate_batch_dev(None, None, 0)
    lib = eng._lib
    rows = _batch(2, 1)[0]; st = np.full(1, -7, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for name in ("bn254_g1_validate_batch", "bn254_g2_validate_batch"):
        f, fd = getattr(lib, name), getattr(lib, name + "_dev")
        assert f(eng._h, None, p(st), 1) == -2 and f(eng._h, p(rows), None, 1) == -2 and f(eng._h, p(rows), p(st), (1 << 40) + 1) == -2
        assert fd(eng._h, None, p(st), 1, None) == -2 and fd(eng._h, p(rows), None, 1, None) == -2
    assert st[0] == -7


def test_the_wire_decoder_reports_5_exactly_where_validation_does(eng):
    """a cross-check against existing code: every on-curve, in-range, finite case, normalised, through g2_encode_batch and g2_decode_batch"""
    cases = [(n, r, s) for n, r, s in S.g2_cases() if s in (S.OK, S.E_SUBGROUP) and S.g2_point(r)[2] != HC.ZERO]
    assert {s for _, _, s in cases} == {S.OK, S.E_SUBGROUP}
    rows = np.stack([r for _, r, _ in cases])
    mine = _host(eng, 2, rows)
    norm = eng.g2_normalize(rows)
    _same(_host(eng, 2, norm), mine, "the normalised points")
    back, st = eng.g2_decode_batch(eng.g2_encode_batch(norm))
    bad = [(n, int(a), int(b)) for (n, _, _), a, b in zip(cases, mine, st) if (a == 5) != (b == 5) or a not in (0, 5) or b not in (0, 5)]
    assert not bad, bad
    ok = mine == 0
    assert back[ok].tobytes() == norm[ok].tobytes()
    # ... and through the compressed decoder, which runs the same membership test
    _, st_c = eng.g2_decompress_batch(eng.g2_compress_batch(norm))
    _same(st_c, st, "g2_decompress_batch")


def test_the_python_face_and_bls_minpk_with_validation(eng):
    import bn_amd
    from bn_amd import Fr, G1, G2, bls_minpk as bls
    assert G2.one().is_valid() and G2.zero().is_valid() and G1.one().is_valid() and G1.zero().is_valid()
    mapped = bn_amd.g2_map_to_curve_batch([(0, 1), (2, 0)])
    assert [p.is_valid() for p in mapped] == [False, False]
    assert [p.is_valid() for p in bn_amd.g2_clear_cofactor_batch(mapped)] == [True, True]
    _same(bn_amd.g2_validate_batch(mapped + [G2.one()]), np.array([5, 5, 0], np.int32), "g2_validate_batch")
    off = G1.one().limbs.copy(); off[4] ^= np.uint64(1)
    _same(bn_amd.g1_validate_batch([G1.one(), G1(off)]), np.array([0, 4], np.int32), "g1_validate_batch")
    sks = [Fr(101 + 13 * i) for i in range(5)]
    pks = bls.public_keys(sks)
    msgs = [bytes([65 + i]) * 6 for i in range(5)]
    sigs = bls.sign_batch(sks, msgs)
    assert bls.verify_batch(pks, msgs, sigs, validate=True).tolist() == [True] * 5
    spoiled = list(sigs); spoiled[2] = mapped[0]                                 # on the twist, outside G2
    assert bls.verify_batch(pks, msgs, spoiled, validate=True).tolist() == [True, True, False, True, True]
    no_key = list(pks); no_key[4] = G1.zero()
    assert bls.verify_batch(no_key, msgs, sigs, validate=True).tolist() == [True, True, True, True, False]
