"""Transforms over G1 and G2 on an MI355X (run with -m gpu): bn254_g{1,2}_ntt_batch, their _dev entry points and the Python faces.  The
model is the O(n^2) sum of the definition with the oracle's chains (tests/group_ntt_cases.py); a second, independent check needs no model
of the new code at all: for in[j] = [a_j] G the output is [fr_ntt(a)_k] G - up to 2^10 with the device's Fr transform, at 2^13 (the
smallest size at which both halves of the root and shift table pairs take part) with the transform on Python integers.  Expected bytes are
exact: every output is normalised."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as FC
import group_ntt_cases as GC
import ntt_cases as NC

pytestmark = pytest.mark.gpu
GROUPS = [1, 2]


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_group_ntt_set_launch_max.argtypes = [C.c_size_t]
    return l


class capped:
    """the launch cap forced to `units` butterflies / points for the length of a with block"""
    def __init__(self, lib, units): self.lib, self.units = lib, units
    def __enter__(self): assert self.lib.bn254_group_ntt_set_launch_max(self.units) == 0
    def __exit__(self, *exc): assert self.lib.bn254_group_ntt_set_launch_max(0) == 0


def _shift(sh):
    return None if sh is None else FC.rows([sh])[0]


def _ntt(eng, g, P, log_n, inverse=False, sh=None):
    return (eng.g1_ntt_batch if g == 1 else eng.g2_ntt_batch)(P, log_n, inverse, _shift(sh))


def _diff(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8]


def _gen(g):
    return GC.oracle().g1_one() if g == 1 else GC.oracle().g2_one()


def _base_multiples(eng, g, scalars):
    """[a] G for the Montgomery rows a, normalised, by the fixed-base call"""
    return (eng.g1_mul_base_batch if g == 1 else eng.g2_mul_base_batch)(_gen(g), scalars)


@pytest.mark.parametrize("g", GROUPS)
def test_against_the_model_with_the_launch_cap_at_four(eng, lib, g):
    """log_n 0..3, one and three transforms, both directions, the three shifts; a cap of 4 makes every transform of 8 a group of its own and
    cuts its passes and its normalisation into two sub-launches"""
    with capped(lib, 4):
        for log_n in GC.LOGS:
            for count in (1, 3):
                P = GC.batch(g, log_n, count, seed=100 + 10 * log_n + count)
                for inverse in (False, True):
                    for sh in NC.SHIFTS:
                        got = _ntt(eng, g, P, log_n, inverse, sh)
                        want = GC.model(g, P, log_n, inverse, sh)
                        assert got.shape == P.shape and got.dtype == np.uint64
                        assert got.tobytes() == want.tobytes(), (g, log_n, count, inverse, sh, _diff(got, want))


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("log_n, cap", [(7, 4), (10, 0)])
def test_the_transform_of_multiples_of_the_generator_is_the_transform_of_their_scalars(eng, lib, g, log_n, cap):
    """in[j] = [a_j] G  =>  out[k] = [fr_ntt(a)_k] G, byte for byte: the right side runs none of the new code"""
    n = 1 << log_n
    vals = FC.values(n, seed=200 + log_n)
    vals[3] = 0; vals[4] = vals[5]                                              # infinity and two equal points among the inputs
    a = FC.rows(vals)
    P = _base_multiples(eng, g, a)
    with capped(lib, cap):
        for inverse, sh in ((False, None), (True, None), (False, NC.SHIFT_RANDOM), (True, 5)):
            got = _ntt(eng, g, P, log_n, inverse, sh)
            want = _base_multiples(eng, g, eng.fr_ntt_batch(a, log_n, inverse, _shift(sh)))
            assert got.tobytes() == want.tobytes(), (g, log_n, inverse, sh, _diff(got, want))


BIG_LOG = 13                                                # the smallest size whose twiddle exponents have a low part and whose shift powers a high one
BIG_MODES = ((False, None), (True, None), (False, NC.SHIFT_RANDOM), (True, 5))
_big = {}


def _big_scalars():
    """8192 scalars: zero at 3 and 4096 (and at 5000, where the record is made garbage with z == 0), equal ones at 4 and 5, a and r - a at 6 and 7"""
    if "scalars" not in _big:
        vals = FC.values(1 << BIG_LOG, seed=213)
        vals[3] = vals[4096] = vals[5000] = 0
        vals[5] = vals[4]
        vals[7] = (FC.R - vals[6]) % FC.R
        assert vals[4] and vals[6]
        _big["scalars"] = vals
    return _big["scalars"]


def _big_transform(inverse, sh):
    """the transform of the scalars on Python integers, once per mode for both groups"""
    key = ("ntt", inverse, sh)
    if key not in _big:
        _big[key] = FC.rows(NC.ntt(_big_scalars(), inverse, sh))
    return _big[key]


def _big_input(eng, g):
    """[a_j] G; every eighth point (and those at 4 and 6) moved to (x l^2, y l^3, l) with l random or q - 1 on host integers; garbage with z == 0 at 5000"""
    if ("in", g) not in _big:
        P = _base_multiples(eng, g, FC.rows(_big_scalars())).copy()
        rng = np.random.default_rng(130 + g)
        comps = GC.WORDS[g] // 4
        moved = 0
        for i in [4, 6] + list(range(1, len(P), 8)):
            c = [GC.M.from_mont_limbs([int(w) for w in P[i, 4 * k:4 * k + 4]]) for k in range(comps)]
            x, y, z = c if g == 1 else ((c[0], c[1]), (c[2], c[3]), (c[4], c[5]))
            if z == GC.ZC.OPS[g].zero:
                continue
            assert z == GC.ZC.OPS[g].one                                        # the fixed-base call normalises
            P[i] = GC.ZC.rows(g, [GC.ZC.rep(g, (x, y), GC.ZC.lam_of(rng, 2 * (i // 8 % 2)))])[0]
            moved += 1
        assert moved >= len(P) // 8
        P[5000] = GC.ZC.rows(g, [GC.ZC.garbage(g, rng)])[0]
        _big["in", g] = P
    return _big["in", g]


@pytest.mark.parametrize("inverse, sh", BIG_MODES, ids=("forward", "inverse", "forward coset", "inverse coset"))
@pytest.mark.parametrize("g", GROUPS)
def test_all_8192_outputs_of_a_transform_of_multiples_of_the_generator(eng, g, inverse, sh):
    """in[j] = [a_j] G  =>  out = [ntt(a)] G at 2^13, where stage 12 takes twiddles with a low part of the exponent and the pass takes shift
    powers with a high one; the transform of the scalars is done on Python integers, so no device transform takes part in the expectation"""
    got = _ntt(eng, g, _big_input(eng, g), BIG_LOG, inverse, sh)
    want = _base_multiples(eng, g, _big_transform(inverse, sh))
    assert got.tobytes() == want.tobytes(), (g, inverse, sh, _diff(got, want))


@pytest.mark.parametrize("g", GROUPS)
def test_a_transform_of_8192_in_sub_launches_of_a_thousand(eng, lib, g):
    """the inverse coset transform again under a cap of 1000 units: sub-launches that are no whole waves, with offsets above a wave, in every
    stage, in the pass and in the normalisation"""
    inverse, sh = BIG_MODES[3]
    with capped(lib, 1000):
        got = _ntt(eng, g, _big_input(eng, g), BIG_LOG, inverse, sh)
    want = _base_multiples(eng, g, _big_transform(inverse, sh))
    assert got.tobytes() == want.tobytes(), (g, _diff(got, want))


@pytest.mark.parametrize("g", GROUPS)
def test_round_trip_of_8192_on_a_coset(eng, g):
    P = GC.batch(g, BIG_LOG, 1, seed=6)                                         # the set with points at infinity between the others
    back = _ntt(eng, g, _ntt(eng, g, P, BIG_LOG, False, NC.SHIFT_RANDOM), BIG_LOG, True, NC.SHIFT_RANDOM)
    want = GC.normalize(g, P)
    assert back.tobytes() == want.tobytes(), (g, _diff(back, want))


@pytest.mark.parametrize("g", GROUPS)
def test_constant_delta_and_all_infinity(eng, g):
    log_n, n = 5, 32
    sets = GC.inputs(g, log_n, seed=3)
    zero = GC.normalize(g, sets["all infinity"][:1])[0]
    P = sets["constant"]
    out = _ntt(eng, g, P, log_n)
    want0 = _ntt(eng, g, (eng.g1_mul_batch if g == 1 else eng.g2_mul_batch)(P[:1], FC.rows([n])), 0)[0]      # [n] P
    assert out[0].tobytes() == want0.tobytes() and not np.array_equal(out[0], zero)
    assert all(r.tobytes() == zero.tobytes() for r in out[1:])
    delta = np.concatenate([sets["random"][:1], sets["all infinity"][1:]])
    out = _ntt(eng, g, delta, log_n)
    p0 = GC.normalize(g, delta[:1])[0]
    assert all(r.tobytes() == p0.tobytes() for r in out)
    for inverse, sh in ((False, None), (True, 5)):
        out = _ntt(eng, g, sets["all infinity"], log_n, inverse, sh)
        assert all(r.tobytes() == zero.tobytes() for r in out)


@pytest.mark.parametrize("g", GROUPS)
def test_round_trip(eng, g):
    log_n = 4
    P = GC.batch(g, log_n, 3, seed=5)
    for sh in (None, NC.SHIFT_RANDOM):
        back = _ntt(eng, g, _ntt(eng, g, P, log_n, False, sh), log_n, True, sh)
        assert back.tobytes() == GC.normalize(g, P).tobytes(), (g, sh, _diff(back, GC.normalize(g, P)))


@pytest.mark.parametrize("g", GROUPS)
def test_in_place_on_the_host_and_on_a_stream(eng, lib, g):
    """out == in through the host call; through the _dev call on a stream that is not the default one, out of place and in place, for an odd
    and an even number of stages, with the host `shift` overwritten as soon as the call has returned"""
    import torch
    from bn_amd import _native
    host = eng._lib.bn254_g1_ntt_batch if g == 1 else eng._lib.bn254_g2_ntt_batch
    dev = eng.g1_ntt_batch_dev if g == 1 else eng.g2_ntt_batch_dev
    for log_n, count, inverse in ((3, 3, True), (4, 2, False)):
        P = GC.batch(g, log_n, count, seed=300 + log_n)
        want = _ntt(eng, g, P, log_n, inverse, NC.SHIFT_RANDOM)
        if log_n == 3:
            assert want.tobytes() == GC.model(g, P, log_n, inverse, NC.SHIFT_RANDOM).tobytes()
        buf = P.copy()
        p = buf.ctypes.data_as(C.c_void_p)
        sh = _shift(NC.SHIFT_RANDOM).copy()
        _native.check(host(eng._h, p, p, log_n, count, int(inverse), sh.ctypes.data_as(C.c_void_p)))
        assert buf.tobytes() == want.tobytes(), ("host, in place", g, log_n, _diff(buf, want))
        stream = torch.cuda.Stream()
        d_in = torch.from_numpy(P.view(np.int64)).cuda()
        d_out = torch.zeros_like(d_in)
        d_io = d_in.clone()
        torch.cuda.synchronize()
        with capped(lib, 8 if log_n == 3 else 0):
            with torch.cuda.stream(stream):
                dev(d_in.data_ptr(), d_out.data_ptr(), log_n, count, inverse, sh, stream.cuda_stream)
                sh[:] = 7                                                        # read before the call returned
                sh2 = _shift(NC.SHIFT_RANDOM).copy()
                dev(d_io.data_ptr(), d_io.data_ptr(), log_n, count, inverse, sh2, stream.cuda_stream)
                sh2[:] = 0
            stream.synchronize()
        assert d_out.cpu().numpy().view(np.uint64).tobytes() == want.tobytes(), ("stream, out of place", g, log_n)
        assert d_io.cpu().numpy().view(np.uint64).tobytes() == want.tobytes(), ("stream, in place", g, log_n)
        assert d_in.cpu().numpy().view(np.uint64).tobytes() == P.tobytes(), "the input was written"


def test_two_streams_of_one_context_give_the_bytes_of_each_call_alone(eng):
    """one fresh context, two streams, no synchronisation between the calls: G1 and G2 transforms with two different shifts and both
    directions alternate on the streams, so every call finds the scratch - workspace, window tables, prefix products, the shift's table
    pair - as another call on the other stream left it"""
    import bn_amd
    import torch
    forms = []
    for i, (g, log_n, count, inverse, sh) in enumerate(((1, 6, 2, False, 5), (2, 5, 1, True, 7), (1, 4, 5, True, 5), (2, 6, 1, False, None), (1, 6, 2, False, 7), (2, 4, 3, True, 5))):
        P = GC.batch(g, log_n, count, seed=400 + i)
        forms.append((g, log_n, count, inverse, sh, P, _ntt(eng, g, P, log_n, inverse, sh), torch.from_numpy(P.view(np.int64)).cuda()))
    outs = [torch.zeros_like(f[7]) for f in forms]
    e = bn_amd.Engine(0)
    s = (torch.cuda.Stream(), torch.cuda.Stream())
    torch.cuda.synchronize()
    for lap in range(2):
        for i, (g, log_n, count, inverse, sh, _, _, d_in) in enumerate(forms):
            dev = e.g1_ntt_batch_dev if g == 1 else e.g2_ntt_batch_dev
            dev(d_in.data_ptr(), outs[i].data_ptr(), log_n, count, inverse, _shift(sh), s[(i + lap) & 1].cuda_stream)
    torch.cuda.synchronize()
    for i, f in enumerate(forms):
        assert outs[i].cpu().numpy().view(np.uint64).tobytes() == f[6].tobytes(), ("interleaved", i, f[:5])
        assert f[7].cpu().numpy().view(np.uint64).tobytes() == f[5].tobytes(), ("input", i)
    e.close()


def test_python_faces(eng):
    import bn_amd
    from bn_amd import G1, G2
    for g, cls, one, batch in ((1, G1, bn_amd.g1_ntt, bn_amd.g1_ntt_batch), (2, G2, bn_amd.g2_ntt, bn_amd.g2_ntt_batch)):
        P = GC.batch(g, 2, 2, seed=500 + g)
        want = GC.model(g, P, 2, False, 5)
        got = batch([cls(r) for r in P], 2, shift=5, engine=eng)
        assert np.stack([x.limbs for x in got]).tobytes() == want.tobytes()
        got = one(P[:4], inverse=True, engine=eng)
        assert np.stack([x.limbs for x in got]).tobytes() == GC.model(g, P[:4], 2, True).tobytes()
        assert batch([], 3, engine=eng) == []
        with pytest.raises(ValueError, match="power of two"):
            one(P[:3], engine=eng)
        with pytest.raises(ValueError, match="whole transforms"):
            batch(P[:6], 2, engine=eng)
        with pytest.raises(ValueError, match="non-zero"):
            one(P[:4], shift=0, engine=eng)
