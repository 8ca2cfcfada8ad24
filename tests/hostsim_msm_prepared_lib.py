"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_msm_prepared.cpp (the bodies of the multi-scalar multiplication against prepared bases of
bn_amd/csrc/group_ops.hpp and its planner and checks of host_plan.hpp, compiled with g++ and -DBN_BOUNDS) as Python calls over numpy
arrays, for tests/test_hostsim_msm_prepared.py and tests/test_host_plan_msm_prepared.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_lib = None


def lib():
    """compiled the way hostsim_lib.py compiles its bounds library: g++ -O1 -DBN_BOUNDS, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_msm_prepared.so"
        src = HERE / "hostsim_msm_prepared.cpp"
        srcs = [src] + sorted(HERE.glob("*.hpp")) + sorted(CSRC.glob("*.hpp")) + [CSRC.parents[1] / "include" / "bn254_hip.h"]
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-pthread", "-o", str(out), str(src)])
        l = C.CDLL(str(out))
        assert l.hsp_bounds_enabled() == 1
        for name in ("hsp_piece", "hsp_signed_digits", "hsp_window_bits", "hsp_level_len"):
            getattr(l, name).restype = C.c_uint32
        l.hsp_signed_digits.argtypes = [U32P, C.c_uint32, U32P, U32P]
        l.hsp_record.argtypes = [U32P, U32P, C.c_uint32, U32P, C.c_uint32]
        l.hsp_double.argtypes = [C.c_int, U32P, C.c_uint32, C.c_uint32]
        l.hsp_table.argtypes = [C.c_int, U32P, C.c_uint32, C.c_uint32, U32P, U32P]
        l.hsp_acc.argtypes = [C.c_int, U32P, U32P, U32P, C.c_uint32, U32P, U32P]
        l.hsp_route.argtypes = [C.c_int, U32P, C.c_uint32, C.c_uint32, U32P, C.c_uint32, C.c_uint32, C.c_uint32, U32P, U32P]
        l.hsp_plan.argtypes = [C.c_uint, C.c_size_t, C.c_size_t, C.c_size_t, U64P, U64P, C.c_size_t]
        l.hsp_tail_scalars.restype = C.c_size_t
        l.hsp_tail_scalars.argtypes = [C.c_uint, U64P, C.c_size_t]
        l.hsp_window_bits.argtypes = [C.c_size_t]
        l.hsp_level_len.argtypes = [C.c_uint32, C.c_uint32]
        l.hsp_prepare_check.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        l.hsp_prepared_check.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        _lib = l
    return _lib


def p32(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(U32P)


def windows(c):
    return (254 + c - 1) // c


def signed_digits(k, c):
    """the device's recoding of the integer k < r -> ([(|d|, negative)] per window, carry out of the top window)"""
    raw = np.frombuffer(int(k).to_bytes(32, "little"), np.uint32).copy()
    W = windows(c)
    mag, neg = np.zeros(W, np.uint32), np.zeros(W, np.uint32)
    carry = lib().hsp_signed_digits(p32(raw), c, p32(mag), p32(neg))
    return [(int(m), bool(n)) for m, n in zip(mag, neg)], int(carry)


def plan(cb, chunk, V, L=16):
    """the workspace plan as a dict: the head fields, and levels = [(out_slots, o_points, o_keys)]"""
    head = np.zeros(15, np.uint64)
    levels = np.zeros((64, 3), np.uint64)
    assert lib().hsp_plan(cb, chunk, V, L, head.ctypes.data_as(U64P), levels.ctypes.data_as(U64P), 64) == 1
    names = "W G groups K count n0max o_counts o_tiles o_n0 o_idx o_keys o_buckets o_terms bytes nlevels".split()
    p = {k: int(v) for k, v in zip(names, head)}
    p["levels"] = [tuple(int(v) for v in r) for r in levels[:p["nlevels"]]]
    return p


def tail_scalars(cb):
    """the tail's scalars as Montgomery images -> (2 * groups, 4) uint64"""
    need = lib().hsp_tail_scalars(cb, None, 0)
    out = np.zeros(need, np.uint64)
    assert lib().hsp_tail_scalars(cb, out.ctypes.data_as(U64P), need) == need
    return out.reshape(-1, 4)
