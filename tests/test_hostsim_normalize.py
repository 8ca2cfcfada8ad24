"""The bodies of bn254_g{1,2}_normalize_batch and bn254_g{1,2}_eq_batch (bn_amd/csrc/group_ops.hpp normalize_body, eq_body) on the CPU:
tests/hostsim/hostsim_normalize.cpp runs the kernels' own code over host arrays, G2 on simulated lane pairs, with the run-time enforcement
of every limb / value bound on (-DBN_BOUNDS: a violated bound aborts the process), for every run length the library can be built with,
against bn_model's exact arithmetic.  The inputs are those of tests/test_gpu_normalize.py at n <= 40."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import normalize_cases as NC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
RUNS = (1, 4, 8, 16)
_U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def sim():
    """compiled the way hostsim_lib.py compiles its library: g++, -DBN_BOUNDS, rebuilt when a source is newer"""
    out = HERE / "libhostsim_normalize_bounds.so"
    srcs = [HERE / "hostsim_normalize.cpp", HERE / "lanepair.hpp", HERE / "lanequad.hpp"] + sorted(CSRC.glob("*.hpp"))
    if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_normalize.cpp")])
    lib = C.CDLL(str(out))
    assert lib.hsn_bounds_enabled() == 1
    return lib


def _normalize(lib, g, P, K, in_place=False):
    P = np.ascontiguousarray(P, np.uint64)
    out = P.copy() if in_place else np.full_like(P, 0x5a5a5a5a5a5a5a5a)
    src = out if in_place else P
    lib.hsn_normalize(C.c_int(g), src.ctypes.data_as(_U32P), C.c_uint32(P.shape[0]), C.c_uint32(K), out.ctypes.data_as(_U32P))
    return out


def test_the_shipped_run_length_is_covered(sim):
    sim.hsn_shipped_run.restype = C.c_uint32
    assert sim.hsn_shipped_run() in RUNS


@pytest.mark.parametrize("K", RUNS)
@pytest.mark.parametrize("g", [1, 2])
def test_normalize_body_against_the_model(sim, g, K):
    sizes = sorted({1, max(1, K - 1), K, K + 1, min(40, 2 * K + 3), 40})
    for n in sizes:
        for phase in range(6):
            pts = NC.points(g, n, K, phase, seed=100 * K + phase)
            P = NC.rows(g, pts)
            want = NC.rows(g, [NC.model_normalize(g, p) for p in pts])
            got = _normalize(sim, g, P, K)
            assert np.array_equal(got, want), (g, K, n, phase, np.nonzero((got != want).any(axis=1))[0])
            assert np.array_equal(_normalize(sim, g, P, K, in_place=True), want), ("in place", g, K, n, phase)


@pytest.mark.parametrize("g", [1, 2])
def test_the_bytes_do_not_depend_on_the_run_length(sim, g):
    P = NC.rows(g, NC.points(g, 37, 5, 2, seed=9))
    outs = [_normalize(sim, g, P, K) for K in RUNS + (3, 37, 64)]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


@pytest.mark.parametrize("g", [1, 2])
def test_eq_body_against_the_model(sim, g):
    a, b = NC.pairs(g, 40, seed=5)
    want = np.array([NC.model_eq(g, x, y) for x, y in zip(a, b)], np.int32)
    assert want.tolist()[:6] == [1, 0, 0, 1, 0, 0]
    A, Bm = NC.rows(g, a), NC.rows(g, b)
    for X, Y, w in ((A, Bm, want), (Bm, A, want), (A, A, np.ones(40, np.int32))):
        got = np.full(40, -7, np.int32)
        sim.hsn_eq(C.c_int(g), X.ctypes.data_as(_U32P), Y.ctypes.data_as(_U32P), C.c_uint32(40), got.ctypes.data_as(C.POINTER(C.c_int32)))
        assert np.array_equal(got, w), (g, np.nonzero(got != w)[0])
    # eq(a, b) == (normalize(a) == normalize(b) bytewise)
    na, nb = _normalize(sim, g, A, 8), _normalize(sim, g, Bm, 8)
    assert np.array_equal((na == nb).all(axis=1), want != 0)
