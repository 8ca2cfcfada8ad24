"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_mle_open.cpp (the quotient body of bn_amd/csrc/mle_ops.hpp and the check and passes of
host_plan.hpp, compiled with g++) as Python calls over integer lists, for tests/test_hostsim_mle_open.py and tests/test_host_plan_mle_open.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

import fr_cases as FC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _U64P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
PATTERN = 0x5a5a5a5a5a5a5a5a
_lib = None


def lib():
    """compiled the way hostsim_mle_lib.py compiles its library: g++, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_mle_open.so"
        srcs = [HERE / "hostsim_mle_open.cpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_mle_open.cpp")])
        l = C.CDLL(str(out))
        l.hso_shipped_levels.restype = C.c_uint32; l.hso_levels_max.restype = C.c_uint32
        l.hso_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        l.hso_plan.restype = C.c_size_t
        l.hso_plan.argtypes = [C.c_uint, C.c_uint, _U64P, C.c_size_t, _SZP]
        l.hso_quotients.argtypes = [_U32P, C.c_int, C.c_void_p, C.c_uint, C.c_size_t, _U32P, _SZP]
        _lib = l
    return _lib


def quotients(table, z, rho, step=1 << 22):
    """the device form over lists of integers -> ((2^nv, 4) uint64 heap, the input array as the call left it, sub-launches)"""
    A = FC.rows(table)
    Z = FC.rows(z) if z else np.zeros((1, 4), np.uint64)
    out = np.full((len(table), 4), PATTERN, np.uint64)
    n = C.c_size_t()
    rc = lib().hso_quotients(A.ctypes.data_as(_U32P), len(z), Z.ctypes.data, rho, step, out.ctypes.data_as(_U32P), C.byref(n))
    assert rc == 0, rc
    return out, A, n.value


def plan(nv, rho):
    """(passes as (levels, vars, lanes, first, last) rows, scratch records)"""
    slots = C.c_size_t()
    rows = np.zeros((64, 5), np.uint64)
    count = lib().hso_plan(nv, rho, rows.ctypes.data_as(_U64P), 64, C.byref(slots))
    return [tuple(int(v) for v in r) for r in rows[:count]], slots.value
