"""The bodies of bn254_fr_ntt_batch (bn_amd/csrc/ntt_ops.hpp over fr.hpp, planned by host_plan.hpp) on the CPU: tests/hostsim/hostsim_ntt.cpp
runs the kernels' own code over host arrays - table build, load, stages, store, the groups, passes and sub-launches of the device unit -
for small tile logs, so that a transform of a few hundred elements takes up to nine passes, against Python integers (tests/ntt_cases.py).
The tile accessor counts every access out of range."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import fr_cases as FC
import ntt_cases as NC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P = C.POINTER(C.c_uint32)
_U64P = C.POINTER(C.c_uint64)
TILE_LOGS = (1, 2, 3, 4)
LOG_NS = tuple(range(10))
BIG_STEP = 1 << 22


@pytest.fixture(scope="module")
def sim():
    """compiled the way test_hostsim_fr.py compiles its library: g++, rebuilt when a source is newer"""
    out = HERE / "libhostsim_ntt.so"
    srcs = [HERE / "hostsim_ntt.cpp"] + sorted(CSRC.glob("*.hpp"))
    if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_ntt.cpp")])
    lib = C.CDLL(str(out))
    lib.hsn_shipped_tile_log.restype = C.c_uint32
    lib.hsn_passes.restype = C.c_uint32
    lib.hsn_passes.argtypes = [C.c_uint32, C.c_uint32]
    lib.hsn_ntt.argtypes = [_U32P, _U32P, C.c_uint32, C.c_size_t, C.c_int, _U64P, C.c_uint32, C.c_size_t]
    return lib


def _run(sim, rows, log_n, count, inverse, shift, T, step=BIG_STEP, in_place=False):
    src = np.ascontiguousarray(rows).copy()
    out = src if in_place else np.full_like(src, 0x5a5a5a5a5a5a5a5a)
    sh = NC.shift_row(shift)
    errors = sim.hsn_ntt(src.ctypes.data_as(_U32P), out.ctypes.data_as(_U32P), log_n, count, int(inverse), None if sh is None else sh.ctypes.data_as(_U64P), T, step)
    assert errors == 0, "tile accesses out of range: %d" % errors
    if not in_place:
        assert np.array_equal(src, np.ascontiguousarray(rows)), "the input was written"
    return out


@pytest.fixture(scope="module")
def cases():
    """(log_n, count) -> (values, rows, {(inverse, shift): expected rows}), computed once"""
    out = {}
    for log_n in LOG_NS:
        for count in (1, 3):
            vals = NC.batch(log_n, count, seed=10 * log_n + count)
            want = {(inv, sh): FC.rows(NC.ntt_batch(vals, log_n, inv, sh)) for inv in (False, True) for sh in NC.SHIFTS}
            out[log_n, count] = (vals, FC.rows(vals), want)
    return out


def test_the_plan_covers_the_shipped_tile(sim):
    T = sim.hsn_shipped_tile_log()
    assert 1 <= T <= 12
    for log_n in range(25):
        for t in list(TILE_LOGS) + [T]:
            assert sim.hsn_passes(log_n, t) == max(1, -(-log_n // t)), (log_n, t)


def test_the_host_arithmetic_of_the_plan(sim):
    """root, product and inverse the entry point computes on the host (shift^-1, n^-1, the roots of the tables)"""
    out = np.zeros(4, np.uint64)
    for log_n in range(29):
        assert sim.hsn_root(log_n, out.ctypes.data_as(_U64P)) == 0
        assert np.array_equal(out, FC.rows([NC.root(log_n)])[0]), log_n
    assert sim.hsn_root(29, out.ctypes.data_as(_U64P)) == -2 and sim.hsn_root(-1, out.ctypes.data_as(_U64P)) == -2
    a, b = FC.pairs(30, seed=3)
    for x, y in zip(a, b):
        X, Y = FC.rows([x])[0], FC.rows([y])[0]
        sim.hsn_host_mul(X.ctypes.data_as(_U64P), Y.ctypes.data_as(_U64P), out.ctypes.data_as(_U64P))
        assert np.array_equal(out, FC.rows([x * y])[0]), (x, y)
        if x:
            sim.hsn_host_inverse(X.ctypes.data_as(_U64P), out.ctypes.data_as(_U64P))
            assert np.array_equal(out, FC.rows([pow(x, -1, FC.R)])[0]), x


@pytest.mark.parametrize("T", TILE_LOGS)
@pytest.mark.parametrize("inverse", [False, True])
def test_against_the_model(sim, cases, T, inverse):
    for (log_n, count), (_, rows, want) in cases.items():
        for sh in NC.SHIFTS:
            for in_place in (False, True):
                got = _run(sim, rows, log_n, count, inverse, sh, T, in_place=in_place)
                assert np.array_equal(got, want[inverse, sh]), (T, log_n, count, inverse, sh, in_place, np.nonzero((got != want[inverse, sh]).any(axis=1))[0][:8])


def test_the_special_inputs_give_their_closed_forms(sim):
    """a delta at 0 gives a constant, a constant gives n delta_0, a delta at 1 the powers of w; all zero stays zero"""
    log_n, n = 5, 32
    sets = NC.inputs(log_n, seed=5)
    c = sets["constant"][0]
    for T in (2, 4):
        assert np.array_equal(_run(sim, FC.rows(sets["delta 0"]), log_n, 1, False, None, T), FC.rows([c] * n))
        assert np.array_equal(_run(sim, FC.rows(sets["constant"]), log_n, 1, False, None, T), FC.rows([n * c] + [0] * (n - 1)))
        assert np.array_equal(_run(sim, FC.rows(sets["delta 1"]), log_n, 1, False, None, T), FC.rows([c * pow(NC.root(log_n), k, FC.R) for k in range(n)]))
        assert not _run(sim, FC.rows(sets["zero"]), log_n, 1, False, 5, T).any()
        want = FC.rows(NC.ntt(sets["minus one"]))
        assert np.array_equal(_run(sim, FC.rows(sets["minus one"]), log_n, 1, False, None, T), want)


def test_the_bytes_depend_on_neither_the_tile_log_nor_the_sub_launch_size(sim, cases):
    shipped = sim.hsn_shipped_tile_log()
    for log_n, count in ((7, 3), (9, 1)):
        _, rows, want = cases[log_n, count]
        for inverse, sh in ((False, 5), (True, NC.SHIFT_RANDOM), (False, None)):
            for T in TILE_LOGS + (5, 7, shipped):
                for step in (BIG_STEP, 64, 16):                            # 16 elements: a transform is cut between tiles, in every pass
                    for in_place in (False, True):
                        got = _run(sim, rows, log_n, count, inverse, sh, T, step, in_place)
                        assert np.array_equal(got, want[inverse, sh]), (log_n, count, inverse, sh, T, step, in_place)


def test_inverse_of_forward_is_the_identity(sim, cases):
    for log_n in (0, 1, 6, 9):
        _, rows, _ = cases[log_n, 3]
        for sh in NC.SHIFTS:
            fwd = _run(sim, rows, log_n, 3, False, sh, 3)
            assert np.array_equal(_run(sim, fwd, log_n, 3, True, sh, 4), rows), (log_n, sh)
