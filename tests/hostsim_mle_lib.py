"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_mle.cpp (the bodies of bn_amd/csrc/mle_ops.hpp and the checks and level arithmetic of
host_plan.hpp, compiled with g++) as Python calls over integer lists, for tests/test_hostsim_mle.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

import fr_cases as FC
import mle_cases as MC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _U64P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
PATTERN = 0x5a5a5a5a5a5a5a5a
_lib = None


def lib():
    """compiled the way hostsim_lib.py compiles its library: g++, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_mle.so"
        srcs = [HERE / "hostsim_mle.cpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_mle.cpp")])
        l = C.CDLL(str(out))
        l.hsm_shipped_piece.restype = C.c_uint32; l.hsm_shipped_fan.restype = C.c_uint32
        l.hsm_plan.restype = C.c_size_t
        l.hsm_plan.argtypes = [C.c_size_t, C.c_uint, C.c_size_t, C.c_size_t, _U64P, C.c_size_t, _SZP, _SZP]
        l.hsm_eq.argtypes = [_U32P, C.c_int, C.c_size_t, _U32P, _SZP]
        l.hsm_fold.argtypes = [_U32P, C.c_size_t, C.c_void_p, C.c_size_t, _U32P, _SZP]
        l.hsm_round.argtypes = [_U32P, C.c_size_t, C.c_size_t, _SZP, _U64P, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, _U32P, _SZP]
        _lib = l
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def eq(z, step=1 << 22):
    """the device form over a list of integers -> ((2^nv, 4) uint64, sub-launches)"""
    Z = FC.rows(z)
    out = np.full((1 << len(z), 4), PATTERN, np.uint64)
    n = C.c_size_t()
    rc = lib().hsm_eq(_u32(Z), len(z), step, _u32(out), C.byref(n))
    assert rc == 0, rc
    return out, n.value


def fold(table, r, step=1 << 22, in_place=False):
    """the device form over integers (or rows of integers: index-major tables) -> (the whole output ARRAY, sub-launches): len / 2 records, or -
    in place - all len records, the upper half as the fold left it"""
    T = MC.limbs(table).reshape(-1, 4) if table and isinstance(table[0], (list, tuple)) else FC.rows(table)
    length = T.shape[0]
    out = T if in_place else np.full((length // 2, 4), PATTERN, np.uint64)
    rr = FC.rows([r])
    n = C.c_size_t()
    rc = lib().hsm_fold(_u32(T), length, rr.ctypes.data, step, _u32(out), C.byref(n))
    assert rc == 0, rc
    return out, n.value


def round_(rows, groups, degree, P, F, step=1 << 22):
    """the device form over rows of integers -> ((degree + 1, 4) uint64, (round sub-launches, sum sub-launches))"""
    T = MC.limbs(rows)
    n, k = T.shape[0], T.shape[1]
    off = np.concatenate([[0], np.cumsum([len(m) for _, m in groups])]).astype(np.uint64)
    members = np.array([j for _, m in groups for j in m], np.uint64)
    coeff = FC.rows([c for c, _ in groups])
    out = np.full((degree + 1, 4), PATTERN, np.uint64)
    launches = (C.c_size_t * 2)()
    rc = lib().hsm_round(_u32(T), n, k, off.ctypes.data_as(_SZP), members.ctypes.data_as(_U64P), coeff.ctypes.data, len(groups), degree, P, F, step, _u32(out), launches)
    assert rc == 0, rc
    return out, tuple(launches)


def plan(h, degree, P, F):
    """(lanes of the round kernel, levels as (cnt, lanes, src, dst, to_out) rows, slots)"""
    sim = lib()
    lanes, slots = C.c_size_t(), C.c_size_t()
    levels = np.zeros((64, 5), np.uint64)
    count = sim.hsm_plan(h, degree, P, F, levels.ctypes.data_as(_U64P), 64, C.byref(lanes), C.byref(slots))
    return lanes.value, levels[:count].astype(np.int64), slots.value
