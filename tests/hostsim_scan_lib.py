"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_scan.cpp (the bodies of bn_amd/csrc/scan_ops.hpp and the planner bn_scan_plan of host_plan.hpp,
compiled with g++) as Python calls over integer lists, for tests/test_host_plan_scan.py and tests/test_hostsim_scan.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

import fr_cases as FC
import scan_cases as SC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _U64P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
KINDS = ("reduce", "up", "down", "apply")
_lib = None


def lib():
    """compiled the way hostsim_lib.py compiles its library: g++, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_scan.so"
        srcs = [HERE / "hostsim_scan.cpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_scan.cpp")])
        l = C.CDLL(str(out))
        l.hss_shipped_piece.restype = C.c_uint32; l.hss_shipped_fan.restype = C.c_uint32
        l.hss_plan.restype = C.c_size_t
        l.hss_plan.argtypes = [_SZP, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _U64P, C.c_size_t, _U64P, C.c_size_t, _SZP, _SZP]
        l.hss_scan.argtypes = [_U32P, _U32P, _U32P, _SZP, C.c_size_t, C.c_uint, C.c_size_t, C.c_size_t, C.c_size_t, _U32P, _SZP]
        l.hss_check.argtypes = [C.c_void_p, C.c_void_p, _SZP, C.c_size_t, C.c_uint, C.c_void_p]
        _lib = l
    return _lib


def scan(a, b, offsets, init, P, F, step=1 << 22, alias=None, **flags):
    """the device form over integer lists (a, b, init may be None) -> ((n, 4) uint64, sub-launches per kind).  alias: "a" or "b" - out IS that
    operand's array"""
    sim = lib()
    o = np.ascontiguousarray(offsets, np.uint64)
    m, n = o.size - 1, int(o[-1])
    A, B, I = (None if v is None else FC.rows(v) for v in (a, b, init))
    out = {"a": A, "b": B}[alias] if alias else np.full((n, 4), 0x5a5a5a5a5a5a5a5a, np.uint64)
    assert out.shape == (n, 4)
    ptr = lambda v: None if v is None else v.ctypes.data_as(_U32P)
    launches = (C.c_size_t * 4)()
    rc = sim.hss_scan(ptr(A), ptr(B), ptr(I), o.ctypes.data_as(_SZP), m, SC.flag_bits(**flags), P, F, step, out.ctypes.data_as(_U32P), launches)
    assert rc == 0, rc
    return out, tuple(launches)


def plan(offsets, P, F, reverse=False):
    """(pieces as (first, len, flag, seg, slot) rows, levels as (kind, first, count) rows, slots)"""
    sim = lib()
    o = np.ascontiguousarray(offsets, np.uint64)
    nl, slots = C.c_size_t(), C.c_size_t()
    count = sim.hss_plan(o.ctypes.data_as(_SZP), o.size - 1, P, F, int(reverse), None, 0, None, 0, C.byref(nl), C.byref(slots))
    pieces = np.zeros((count, 5), np.uint64); levels = np.zeros((nl.value, 3), np.uint64)
    assert sim.hss_plan(o.ctypes.data_as(_SZP), o.size - 1, P, F, int(reverse), pieces.ctypes.data_as(_U64P), count, levels.ctypes.data_as(_U64P), nl.value, C.byref(nl), C.byref(slots)) == count
    return pieces.astype(np.int64), levels.astype(np.int64), slots.value
