"""The bodies of bn254_fr_{add,mul,inverse,pow,interpret}_batch and of the synthetic-scalar generator (bn_amd/csrc/fr_ops.hpp over fr.hpp) on
the CPU: tests/hostsim/hostsim_fr.cpp runs the kernels' own code over host arrays, for every run length of the inversion and every window
width of pow the library can be built with, against Python integers (tests/fr_cases.py).  The inputs are those of tests/test_gpu_fr.py at
n <= 40."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import fr_cases as FC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
RUNS = (1, 4, 8, 16)
WINDOWS = (1, 2, 4)
N = 40
_U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def sim():
    """compiled the way hostsim_lib.py compiles its library: g++, rebuilt when a source is newer"""
    out = HERE / "libhostsim_fr.so"
    srcs = [HERE / "hostsim_fr.cpp"] + sorted(CSRC.glob("*.hpp"))
    if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_fr.cpp")])
    lib = C.CDLL(str(out))
    lib.hsf_shipped_run.restype = C.c_uint32; lib.hsf_shipped_window.restype = C.c_uint32
    return lib


def _p(a):
    return a.ctypes.data_as(_U32P)


def _binary(call, A, B, where):
    """out of place, out == a, out == b"""
    A = np.ascontiguousarray(A); B = np.ascontiguousarray(B)
    if where == "fresh":
        out = np.full_like(A, 0x5a5a5a5a5a5a5a5a); call(_p(A), _p(B), _p(out)); return out
    a, b = A.copy(), B.copy()
    if where == "a":
        call(_p(a), _p(b), _p(a)); return a
    call(_p(a), _p(b), _p(b)); return b


def test_the_shipped_choices_are_covered(sim):
    assert sim.hsf_shipped_run() in RUNS and sim.hsf_shipped_window() in WINDOWS


@pytest.mark.parametrize("where", ["fresh", "a", "b"])
def test_add_sub_mul_against_the_model(sim, where):
    a, b = FC.pairs(N, seed=1)
    assert N > FC.N_PAIR_HEAD                                                # every special pair is in
    A, B = FC.rows(a), FC.rows(b)
    for name, call, want in (
            ("add", lambda x, y, o: sim.hsf_add(x, y, C.c_uint32(N), C.c_int(0), o), [x + y for x, y in zip(a, b)]),
            ("sub", lambda x, y, o: sim.hsf_add(x, y, C.c_uint32(N), C.c_int(1), o), [x - y for x, y in zip(a, b)]),
            ("mul", lambda x, y, o: sim.hsf_mul(x, y, C.c_uint32(N), o), [x * y for x, y in zip(a, b)])):
        got = _binary(call, A, B, where)
        assert np.array_equal(got, FC.rows(want)), (name, where, np.nonzero((got != FC.rows(want)).any(axis=1))[0])
    zero = np.zeros_like(B)                                                  # Neg is 0 - b
    assert np.array_equal(_binary(lambda x, y, o: sim.hsf_add(x, y, C.c_uint32(N), C.c_int(1), o), zero, B, "fresh"), FC.rows([-y for y in b]))


@pytest.mark.parametrize("wb", WINDOWS)
def test_pow_against_the_model(sim, wb):
    a, e = FC.pow_cases(N + 8, seed=2)
    n = len(a)
    A, E = FC.rows(a), FC.rows(e)
    want = FC.rows([pow(x, y, FC.R) for x, y in zip(a, e)])
    assert (want[0] == FC.rows([1])[0]).all() and not want[1].any()             # 0^0 = 1, 0^1 = 0
    for where in ("fresh", "a", "b"):
        got = _binary(lambda x, y, o: sim.hsf_pow(x, y, C.c_uint32(n), C.c_uint32(wb), o), A, E, where)
        assert np.array_equal(got, want), (wb, where, np.nonzero((got != want).any(axis=1))[0])


def _inverse(sim, A, K, wb, in_place=False, with_ok=True):
    A = np.ascontiguousarray(A)
    out = A.copy() if in_place else np.full_like(A, 0x5a5a5a5a5a5a5a5a)
    src = out if in_place else A
    ok = np.full(A.shape[0], -7, np.int32)
    assert sim.hsf_inverse(_p(src), C.c_uint32(A.shape[0]), C.c_uint32(K), C.c_uint32(wb), _p(out), ok.ctypes.data_as(C.POINTER(C.c_int32)) if with_ok else None) == 0
    return out, ok


@pytest.mark.parametrize("K", RUNS)
def test_inverse_against_the_model(sim, K):
    wb = int(sim.hsf_shipped_window())
    for n in sorted({1, max(1, K - 1), K, K + 1, min(N, 2 * K + 3), N}):
        for phase in range(6):
            vals = FC.inverse_values(n, K, phase, seed=100 * K + phase)
            want, want_ok = FC.model_inverse(vals)
            A = FC.rows(vals)
            got, ok = _inverse(sim, A, K, wb)
            assert np.array_equal(got, want) and np.array_equal(ok, want_ok), (K, n, phase)
            got, ok = _inverse(sim, A, K, wb, in_place=True)
            assert np.array_equal(got, want) and np.array_equal(ok, want_ok), ("in place", K, n, phase)
            got, ok = _inverse(sim, A, K, wb, with_ok=False)
            assert np.array_equal(got, want) and (ok == -7).all(), ("ok == NULL", K, n, phase)


def test_the_bytes_depend_on_neither_the_run_length_nor_the_width(sim):
    vals = FC.inverse_values(37, 5, 2, seed=9)
    outs = [_inverse(sim, FC.rows(vals), K, wb) for K in RUNS + (3, 37, 64) for wb in WINDOWS]
    for o, ok in outs[1:]:
        assert np.array_equal(o, outs[0][0]) and np.array_equal(ok, outs[0][1])
    # inverse is pow by r - 2, and a * a^-1 is one where ok is set
    A = FC.rows(vals)
    E = FC.rows([FC.R - 2] * 37)
    p = np.zeros_like(A); assert sim.hsf_pow(_p(A), _p(E), C.c_uint32(37), C.c_uint32(2), _p(p)) == 0
    assert np.array_equal(p, outs[0][0])
    prod = np.zeros_like(A); sim.hsf_mul(_p(A), _p(outs[0][0]), C.c_uint32(37), _p(prod))
    assert np.array_equal(prod[outs[0][1] != 0], FC.rows([1] * int((outs[0][1] != 0).sum()))) and not prod[outs[0][1] == 0].any()


def test_interpret_against_the_model(sim):
    buf, ints = FC.interpret_buffers(N, seed=4)
    out = np.zeros((N, 4), np.uint64)
    sim.hsf_interpret(buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint32(N), _p(out))
    assert np.array_equal(out, FC.rows([v % FC.R for v in ints]))
    assert not out[0].any() and not out[2].any()                               # 0 and r are zero


def _raw_rows(values):
    """256-bit integers as they are (no reduction, no Montgomery form) -> (n, 4) uint64"""
    return np.array([[(v >> (64 * j)) & ((1 << 64) - 1) for j in range(4)] for v in values], np.uint64)


def test_mul_with_a_non_canonical_left_operand(sim):
    """fr_mul's precondition (fr.hpp): ONE operand below r is enough, the other may be any 256-bit value - what wire decode of a rejected
    record and both halves of fr_from_wide rely on.  a * b / 2^256 mod r from Python integers, canonical"""
    left = [FC.R, FC.R + 1, 1 << 255, (1 << 256) - 1]
    right = [0, 1, FC.MONT % FC.R, FC.MONT * FC.MONT % FC.R, FC.R - 1]
    a = [x for x in left for _ in right]; b = [y for _ in left for y in right]
    n = len(a)
    out = np.full((n, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
    sim.hsf_mul(_p(_raw_rows(a)), _p(_raw_rows(b)), C.c_uint32(n), _p(out))
    inv = pow(FC.MONT, -1, FC.R)
    want = _raw_rows([x * y * inv % FC.R for x, y in zip(a, b)])
    assert np.array_equal(out, want), np.nonzero((out != want).any(axis=1))[0]


@pytest.mark.parametrize("which", [0, 1])
def test_synthetic_scalars_equal_the_numpy_generator(sim, which):
    """fr_synthetic_body (the body of bn254_synthetic_scalars_k) == bn_amd.distributed.synthetic_scalars word for word"""
    from bn_amd import distributed as D
    for lo, hi in ((0, 40), (1 << 24, (1 << 24) + 40), ((1 << 25) - 3, (1 << 25) + 3)):
        out = np.full((hi - lo, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
        sim.hsf_synthetic(C.c_uint64(D.SEED), C.c_uint64(lo), C.c_uint32(hi - lo), C.c_uint32(which), _p(out))
        want = D.synthetic_scalars(lo, hi, which)
        assert np.array_equal(out, want), (which, lo, np.nonzero((out != want).any(axis=1))[0])
