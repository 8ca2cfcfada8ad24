"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_leaf.cpp (the CPU twins of the GPU's inline-asm leaves: every leaf of tests/leafprobe/leaf_list.hpp
on raw limbs, compiled with g++ and -DBN_BOUNDS) as Python calls, for tests/test_hostsim_leaf.py and tests/test_gpu_leaf.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
LIST = HERE.parent / "leafprobe" / "leaf_list.hpp"
_U32P = C.POINTER(C.c_uint32)
_I32P = C.POINTER(C.c_int32)
_lib = None


def lib():
    """compiled the way hostsim_wide_lib.py compiles its bounds-checked library: g++, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_leaf.so"
        srcs = [HERE / "hostsim_leaf.cpp", HERE / "rawleaf.hpp", LIST] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_leaf.cpp")])
        _lib = C.CDLL(str(out))
        assert _lib.hsl_bounds_enabled() == 1
        _lib.hsl_leaf_info.restype = C.c_char_p
        _lib.hsl_run.argtypes = [C.c_int, C.c_int, _U32P, _U32P, _I32P, _U32P]
    return _lib


def leaf_table():
    """[(name, kinds, output limbs)] as compiled into the library"""
    l = lib()
    out = []
    for i in range(l.hsl_leaf_count()):
        name, kinds, outw = l.hsl_leaf_info(i).decode().split(":")
        out.append((name, kinds, int(outw)))
    return out


def run(leaf_id, ops, bounds, flags, outw):
    """every case of one leaf through its twin: ops uint32 [n, stride], bounds uint32 [n, 3 per operand], flags int32 [n] -> uint32 [n, outw].
    A case outside the leaf's contract, or a result outside the bounds the leaf states, ABORTS the process (BN_BOUNDS)."""
    ops = np.ascontiguousarray(ops, np.uint32); bounds = np.ascontiguousarray(bounds, np.uint32); flags = np.ascontiguousarray(flags, np.int32)
    n = ops.shape[0]
    assert bounds.shape[0] == n and flags.shape == (n,)
    out = np.full((n, outw), 0xffffffff, np.uint32)
    rc = lib().hsl_run(int(leaf_id), n, ops.ctypes.data_as(_U32P), bounds.ctypes.data_as(_U32P), flags.ctypes.data_as(_I32P), out.ctypes.data_as(_U32P))
    assert rc == 0, rc
    return out
