"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_fold_round.cpp (the fused fold-then-round body of bn_amd/csrc/mle_ops.hpp and the check, piece
length and level arithmetic of host_plan.hpp, compiled with g++) as Python calls over integer lists, for tests/test_hostsim_fold_round.py,
tests/test_host_plan_fold_round.py and tests/test_fold_round_abi.py."""
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
GUARD = 4                                                   # pattern records behind folded and out: nothing beyond them may be written
_lib = None


def lib():
    """compiled the way hostsim_mle_open_lib.py compiles its library: g++, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_fold_round.so"
        srcs = [HERE / "hostsim_fold_round.cpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_fold_round.cpp")])
        l = C.CDLL(str(out))
        l.hfr_shipped_piece.restype = C.c_uint32; l.hfr_shipped_fan.restype = C.c_uint32
        l.hfr_fill.restype = C.c_size_t; l.hfr_fill.argtypes = [C.c_size_t]
        l.hfr_piece.restype = C.c_size_t; l.hfr_piece.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t]
        l.hfr_check.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
        l.hfr_fold_round.argtypes = [_U32P, C.c_size_t, C.c_size_t, C.c_void_p, _SZP, _U64P, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, _U32P, _U32P, _SZP]
        _lib = l
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def fold_round(rows, r, groups, degree, P, F, step=1 << 22, in_place=False):
    """the device form over rows of integers -> (the tables as the call left them, (n, k, 4); the folded ARRAY with its guard records - or, in
    place, None: the folded rows are rows [0, n/2) of the tables; the out ARRAY of degree + 1 records with its guard; (fused sub-launches, sum
    sub-launches)).  folded and out are pre-filled with a pattern."""
    T = MC.limbs(rows)
    n, k = T.shape[0], T.shape[1]
    off = np.concatenate([[0], np.cumsum([len(m) for _, m in groups])]).astype(np.uint64)
    members = np.array([j for _, m in groups for j in m], np.uint64)
    coeff = FC.rows([c for c, _ in groups])
    rr = FC.rows([r])
    folded = None if in_place else np.full((n // 2 * k + GUARD, 4), PATTERN, np.uint64)
    out = np.full((degree + 1 + GUARD, 4), PATTERN, np.uint64)
    launches = (C.c_size_t * 2)()
    rc = lib().hfr_fold_round(_u32(T), n, k, rr.ctypes.data, off.ctypes.data_as(_SZP), members.ctypes.data_as(_U64P), coeff.ctypes.data, len(groups), degree, P, F, step,
                              _u32(T if in_place else folded), _u32(out), launches)
    assert rc == 0, rc
    return T, folded, out, tuple(launches)
