"""Batched Fr arithmetic on an MI355X (run with -m gpu): bn254_fr_{add,mul,inverse,pow,interpret}_batch, their _dev entry points, the Python
faces and groth16.verify_aggregate.  The model is Python integers (tests/fr_cases.py): the expected bytes are the limbs of v * 2^256 mod r.
Sizes, with K the shipped run length of the inversion: 1, K - 1, K, K + 1, 2 K + 3, 255, 256, 257 and 256 K + 1 (the first lane of a second
workgroup of inverse), and the seam between sub-launches through the library's internal test hook (three sub-launches of 20, 20 and 5)."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_inverse_run.argtypes = []; l.bn254_fr_inverse_run.restype = C.c_uint
    l.bn254_fr_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def K(lib):
    return int(lib.bn254_fr_inverse_run())


def _sizes(K):
    return sorted({1, max(1, K - 1), K, K + 1, 2 * K + 3, 255, 256, 257, 256 * K + 1})


@pytest.fixture(scope="module")
def binary_cases(K):
    """{n: (a, b, A, B)} and {n: (a, e, A, E)}: integers and their rows, built once"""
    pairs, pows = {}, {}
    for n in _sizes(K):
        a, b = FC.pairs(n, seed=10 + n)
        pairs[n] = (a, b, FC.rows(a), FC.rows(b))
        a, e = FC.pow_cases(n, seed=20 + n)
        pows[n] = (a, e, FC.rows(a), FC.rows(e))
    return pairs, pows


def _want(fn, a, b):
    return FC.rows([fn(x, y) for x, y in zip(a, b)])


def test_add_sub_mul_against_the_model(eng, binary_cases, K):
    for n, (a, b, A, B) in binary_cases[0].items():
        for name, got, fn in (("add", eng.fr_add_batch(A, B), lambda x, y: x + y), ("sub", eng.fr_add_batch(A, B, negate_b=True), lambda x, y: x - y),
                              ("mul", eng.fr_mul_batch(A, B), lambda x, y: x * y)):
            assert got.shape == (n, 4) and got.dtype == np.uint64
            assert got.tobytes() == _want(fn, a, b).tobytes(), (name, n, np.nonzero((got != _want(fn, a, b)).any(axis=1))[0][:8])
    assert set(binary_cases[0]) == set(_sizes(K))


def test_pow_against_the_model(eng, binary_cases):
    for n, (a, e, A, E) in binary_cases[1].items():
        got = eng.fr_pow_batch(A, E)
        want = _want(lambda x, y: pow(x, y, FC.R), a, e)
        assert got.tobytes() == want.tobytes(), (n, np.nonzero((got != want).any(axis=1))[0][:8])
    one = FC.rows([1])[0]
    got = eng.fr_pow_batch(FC.rows([0, 0, 5, FC.R - 1]), FC.rows([0, 7, FC.R - 1, FC.R - 1]))
    assert (got[0] == one).all() and not got[1].any() and (got[2] == one).all() and (got[3] == one).all()      # 0^0, 0^e, a^(r-1)


def test_inverse_against_the_model(eng, K):
    seen = set()
    for n in _sizes(K):
        for phase in (range(6) if n <= 2 * K + 3 else (n % 6,)):
            vals = FC.inverse_values(n, K, phase, seed=1000 + 10 * n + phase)
            want, want_ok = FC.model_inverse(vals)
            A = FC.rows(vals)
            got, ok = eng.fr_inverse_batch(A)
            assert ok.dtype == np.bool_ and np.array_equal(ok, want_ok != 0), (n, phase)
            assert got.tobytes() == want.tobytes(), (n, phase, np.nonzero((got != want).any(axis=1))[0][:8])
            # pow by r - 2 gives the same bytes (zero included: 0^(r-2) = 0), and a * a^-1 is one where ok is set
            assert eng.fr_pow_batch(A, np.tile(FC.rows([FC.R - 2]), (n, 1))).tobytes() == got.tobytes(), (n, phase)
            prod = eng.fr_mul_batch(A, got)
            assert (prod[ok] == FC.rows([1])[0]).all() and not prod[~ok].any(), (n, phase)
        seen.add(n)
    assert seen == set(_sizes(K))


def test_interpret_against_the_model(eng, K):
    for n in _sizes(K):
        buf, ints = FC.interpret_buffers(n, seed=30 + n)
        got = eng.fr_interpret_batch(buf)
        assert got.tobytes() == FC.rows([v % FC.R for v in ints]).tobytes(), n


def test_across_sub_launches(eng, lib, K):
    """three sub-launches (20, 20, 5 elements) through the internal hook; the inversion cuts its own runs in every one"""
    a, b = FC.pairs(45, seed=45)
    A, B = FC.rows(a), FC.rows(b)
    vals = FC.inverse_values(45, K, 3, seed=46)
    buf, ints = FC.interpret_buffers(45, seed=47)
    pa, pe = FC.pow_cases(45, seed=48)
    eng.profile(True); eng.profile_reset()
    assert lib.bn254_fr_set_launch_max(20) == 0
    try:
        got = [eng.fr_add_batch(A, B), eng.fr_add_batch(A, B, negate_b=True), eng.fr_mul_batch(A, B), eng.fr_pow_batch(FC.rows(pa), FC.rows(pe)),
               eng.fr_inverse_batch(FC.rows(vals)), eng.fr_interpret_batch(buf)]
        launches = {s: eng.kernel_stats(s)[1] for s in ("fr_add", "fr_mul", "fr_pow", "fr_inverse", "fr_interpret")}
    finally:
        assert lib.bn254_fr_set_launch_max(0) == 0
        eng.profile(False)
    assert launches == {"fr_add": 6, "fr_mul": 3, "fr_pow": 3, "fr_inverse": 3, "fr_interpret": 3}
    assert got[0].tobytes() == _want(lambda x, y: x + y, a, b).tobytes() and got[1].tobytes() == _want(lambda x, y: x - y, a, b).tobytes()
    assert got[2].tobytes() == _want(lambda x, y: x * y, a, b).tobytes()
    assert got[3].tobytes() == _want(lambda x, y: pow(x, y, FC.R), pa, pe).tobytes()
    want, want_ok = FC.model_inverse(vals)
    assert got[4][0].tobytes() == want.tobytes() and np.array_equal(got[4][1], want_ok != 0)
    assert got[5].tobytes() == FC.rows([v % FC.R for v in ints]).tobytes()
    assert lib.bn254_fr_set_launch_max((1 << 22) + 1) == -2


def test_kernel_stats_show_every_scope(eng):
    A = FC.rows(FC.values(9, seed=3))
    eng.profile(True); eng.profile_reset()
    try:
        eng.fr_add_batch(A, A); eng.fr_mul_batch(A, A); eng.fr_pow_batch(A, A); eng.fr_inverse_batch(A); eng.fr_interpret_batch(np.zeros((2, 64), np.uint8))
        stats = {s: eng.kernel_stats(s) for s in ("fr_add", "fr_mul", "fr_inverse", "fr_pow", "fr_interpret")}
    finally:
        eng.profile(False)
    for s, (ms, launches) in stats.items():
        assert launches >= 1 and ms > 0, (s, ms, launches)


def test_in_place_on_the_host_and_on_a_stream(eng, K):
    """out == a and out == b through the host calls; through the _dev calls on a stream that is not the default one; ok == NULL"""
    import torch
    n = 2 * K + 3
    a, b = FC.pairs(n, seed=7)
    a = [x or 5 for x in a]; a[K // 2] = 0; a[K] = 0                       # zeros for the inversion, everything else invertible
    A, B = FC.rows(a), FC.rows(b)
    l = eng._lib
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    want = {"add": _want(lambda x, y: x + y, a, b), "sub": _want(lambda x, y: x - y, a, b), "mul": _want(lambda x, y: x * y, a, b),
            "pow": _want(lambda x, y: pow(x, y, FC.R), a, b)}
    host = {"add": lambda x, y, o: l.bn254_fr_add_batch(eng._h, x, y, o, n, 0), "sub": lambda x, y, o: l.bn254_fr_add_batch(eng._h, x, y, o, n, 1),
            "mul": lambda x, y, o: l.bn254_fr_mul_batch(eng._h, x, y, o, n), "pow": lambda x, y, o: l.bn254_fr_pow_batch(eng._h, x, y, o, n)}
    for name, fn in host.items():
        x, y = A.copy(), B.copy()
        assert fn(p(x), p(y), p(x)) == 0 and x.tobytes() == want[name].tobytes(), ("host out == a", name)
        x, y = A.copy(), B.copy()
        assert fn(p(x), p(y), p(y)) == 0 and y.tobytes() == want[name].tobytes(), ("host out == b", name)
    inv, inv_ok = FC.model_inverse(a)
    x = A.copy(); ok = np.full(n, -7, np.int32)
    assert l.bn254_fr_inverse_batch(eng._h, p(x), p(x), p(ok), n) == 0 and x.tobytes() == inv.tobytes() and np.array_equal(ok, inv_ok)
    x = A.copy()
    assert l.bn254_fr_inverse_batch(eng._h, p(x), p(x), None, n) == 0 and x.tobytes() == inv.tobytes()              # ok == NULL
    # device-resident, on a stream of its own
    stream = torch.cuda.Stream()
    dev = lambda arr: torch.from_numpy(arr.view(np.int64).copy()).to("cuda:0")
    back = lambda t: t.cpu().numpy().view(np.uint64).reshape(n, 4)
    calls = {"add": lambda x, y, o: eng.fr_add_batch_dev(x, y, o, n, False, stream.cuda_stream), "sub": lambda x, y, o: eng.fr_add_batch_dev(x, y, o, n, True, stream.cuda_stream),
             "mul": lambda x, y, o: eng.fr_mul_batch_dev(x, y, o, n, stream.cuda_stream), "pow": lambda x, y, o: eng.fr_pow_batch_dev(x, y, o, n, stream.cuda_stream)}
    for name, fn in calls.items():
        da, db, da2, db2, o = dev(A), dev(B), dev(A), dev(B), torch.zeros(n * 4, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            fn(da.data_ptr(), db.data_ptr(), o.data_ptr())                   # out of place,
            fn(da.data_ptr(), db.data_ptr(), da.data_ptr())                  # out == a,
            fn(da2.data_ptr(), db2.data_ptr(), db2.data_ptr())               # out == b
        stream.synchronize()
        for what, t in (("fresh", o), ("out == a", da), ("out == b", db2)):
            assert back(t).tobytes() == want[name].tobytes(), ("dev", name, what)
    da, o = dev(A), torch.zeros(n * 4, dtype=torch.int64, device="cuda:0")
    dok = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    dbuf = torch.from_numpy(FC.interpret_buffers(n, seed=8)[0]).to("cuda:0"); di = torch.zeros(n * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        eng.fr_inverse_batch_dev(da.data_ptr(), o.data_ptr(), dok.data_ptr(), n, stream.cuda_stream)
        eng.fr_inverse_batch_dev(da.data_ptr(), da.data_ptr(), None, n, stream.cuda_stream)                       # in place, ok == NULL
        eng.fr_interpret_batch_dev(dbuf.data_ptr(), di.data_ptr(), n, stream.cuda_stream)
    stream.synchronize()
    assert back(o).tobytes() == inv.tobytes() and back(da).tobytes() == inv.tobytes() and dok.cpu().numpy().tolist() == inv_ok.tolist()
    assert back(di).tobytes() == FC.rows([v % FC.R for v in FC.interpret_buffers(n, seed=8)[1]]).tobytes()


def test_the_python_faces(eng):
    import bn_amd
    from bn_amd import Fr
    rng = np.random.default_rng(5)
    a = [Fr.random(rng) for _ in range(5)] + [Fr.zero()]
    b = [Fr.random(rng) for _ in range(6)]
    assert bn_amd.fr_add_batch(a, b) == [x + y for x, y in zip(a, b)] and bn_amd.fr_sub_batch(a, b) == [x - y for x, y in zip(a, b)]
    assert bn_amd.fr_neg_batch(a) == [-x for x in a] and bn_amd.fr_mul_batch(a, b) == [x * y for x, y in zip(a, b)]
    assert bn_amd.fr_pow_batch(a, b) == [x.pow(y) for x, y in zip(a, b)]
    assert bn_amd.fr_inverse_batch(a) == [x.inverse() for x in a] and bn_amd.fr_inverse_batch(a)[5] is None
    assert bn_amd.fr_mul_batch(np.stack([x.limbs for x in a]), np.stack([x.limbs for x in b])) == [x * y for x, y in zip(a, b)]      # (n,4) arrays
    bufs = [rng.bytes(64), b"\xff" * 64, bytes(64)]
    assert bn_amd.fr_interpret_batch(bufs) == [Fr.interpret(x) for x in bufs] == [Fr(int.from_bytes(x, "big")) for x in bufs]
    assert bn_amd.fr_add_batch([], []) == [] and bn_amd.fr_inverse_batch([]) == []


class _Spy:
    """an engine that records the scalars of every g1_mul_batch call (the r_j of verify_aggregate)"""
    def __init__(self, eng): self._eng = eng; self.scalars = []
    def g1_mul_batch(self, p, k): self.scalars.append(np.array(k, copy=True)); return self._eng.g1_mul_batch(p, k)
    def __getattr__(self, name): return getattr(self._eng, name)


@pytest.mark.parametrize("l", [1, 9])
def test_groth16_verify_aggregate(l):
    import bn_amd
    from bn_amd import Fr, G1, groth16
    from test_gpu_msm import _groth16_setup
    rng = np.random.default_rng(130 + l)
    vk, prove = _groth16_setup(rng, l)
    m = 5
    inputs = [[Fr.random(rng) for _ in range(l)] for _ in range(m)]
    proofs = prove(inputs)
    assert groth16.verify_aggregate(vk, proofs, inputs) is True
    assert groth16.verify_aggregate(vk, proofs, inputs) == bool(groth16.verify_batch(vk, proofs, inputs).all())
    bad_inputs = [list(a) for a in inputs]; bad_inputs[1][1 % l] = bad_inputs[1][1 % l] + Fr.one()
    assert groth16.verify_aggregate(vk, proofs, bad_inputs) is False                                   # a wrong public input
    swapped = list(proofs); swapped[2] = (proofs[2][0], proofs[2][1], proofs[3][2])
    assert groth16.verify_aggregate(vk, swapped, inputs) is False                                      # a swapped C
    no_a = list(proofs); no_a[4] = (G1.zero(), proofs[4][1], proofs[4][2])
    assert groth16.verify_aggregate(vk, no_a, inputs) is False                                         # A = G1.zero()
    assert not groth16.verify_batch(vk, no_a, inputs).all()
    assert groth16.verify_aggregate(vk, [], []) is True                                                # an empty block
    # a fixed rng makes the call reproducible: the same r_j, and 128-bit ones; without it they are fresh every time
    spies = [_Spy(bn_amd.api.default_engine()) for _ in range(4)]
    assert groth16.verify_aggregate(vk, proofs, inputs, engine=spies[0], rng=np.random.default_rng(1)) is True
    assert groth16.verify_aggregate(vk, proofs, inputs, engine=spies[1], rng=np.random.default_rng(1)) is True
    assert groth16.verify_aggregate(vk, proofs, inputs, engine=spies[2]) is True and groth16.verify_aggregate(vk, proofs, inputs, engine=spies[3]) is True
    r = [s.scalars[0] for s in spies]
    assert r[0].shape == (m, 4) and np.array_equal(r[0], r[1]) and not np.array_equal(r[2], r[3]) and not np.array_equal(r[0], r[2])
    assert all(Fr.from_limbs(x).v < 1 << 128 for x in r[0]) and len({Fr.from_limbs(x).v for x in r[0]}) == m
    with pytest.raises(ValueError):
        groth16.verify_aggregate(vk, proofs, inputs[:-1])
    with pytest.raises(ValueError):
        groth16.verify_aggregate(vk, proofs, [a[:-1] for a in inputs])
