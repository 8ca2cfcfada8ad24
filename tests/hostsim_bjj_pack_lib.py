"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_bjj_pack.cpp (the bodies of bn_amd/csrc/fr_sqrt_ops.hpp and the packing bodies of babyjub_ops.hpp,
compiled with g++ and -DBN_BOUNDS) as Python calls over the arrays of the C ABI, for tests/test_hostsim_bjj_pack.py.  Both forms of the square
root are in the one library."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _I32P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
PATTERN = 0x5a5a5a5a5a5a5a5a
_lib = None


def lib():
    """compiled the way hostsim_babyjub_lib.py compiles its library: g++ -DBN_BOUNDS, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_bjj_pack.so"
        srcs = [HERE / "hostsim_bjj_pack.cpp", HERE / "lanepair.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_bjj_pack.cpp")])
        l = C.CDLL(str(out))
        l.hsp_sqrt.argtypes = [C.c_int, _U32P, _U32P, _I32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsp_sqrt_ratio.argtypes = [C.c_int, _U32P, _U32P, _U32P, _I32P, C.c_size_t]
        l.hsp_pack.argtypes = [_U32P, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsp_unpack.argtypes = [C.c_int, _U32P, _U32P, _I32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsp_verify_packed.argtypes = [C.c_int, _U32P, _U32P, _U32P, _I32P, C.c_size_t, C.c_size_t, _SZP]
        assert l.hsp_bounds_enabled() == 1
        _lib = l
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def _c(a, dtype=np.uint64):
    return np.ascontiguousarray(a, dtype)


def sqrt(A, form, step=1 << 22, in_place=False, with_ok=True):
    """(n,4) uint64 -> ((n,4) uint64, (n,) int32 or None, sub-launches)"""
    A = _c(A).copy(); out = A if in_place else np.full_like(A, PATTERN); ok = np.full(A.shape[0], -1, np.int32) if with_ok else None; n = C.c_size_t()
    assert lib().hsp_sqrt(form, _u32(A), _u32(out), ok.ctypes.data_as(_I32P) if with_ok else None, A.shape[0], step, C.byref(n)) == 0
    return out, ok, n.value


def sqrt_ratio(U, V, form):
    U, V = _c(U), _c(V); out = np.full_like(U, PATTERN); ok = np.full(U.shape[0], -1, np.int32)
    assert lib().hsp_sqrt_ratio(form, _u32(U), _u32(V), _u32(out), ok.ctypes.data_as(_I32P), U.shape[0]) == 0
    return out, ok


def pack(P, step=1 << 22):
    """(n,2,4) uint64 -> ((n,32) uint8, sub-launches)"""
    P = _c(P); out = np.full((P.shape[0], 32), 0x5a, np.uint8); n = C.c_size_t()
    assert lib().hsp_pack(_u32(P), _u32(out), P.shape[0], step, C.byref(n)) == 0
    return out, n.value


def unpack(B, form, step=1 << 22):
    """(n,32) uint8 -> ((n,2,4) uint64, (n,) int32, sub-launches)"""
    B = _c(B, np.uint8); out = np.full((B.shape[0], 2, 4), PATTERN, np.uint64); st = np.full(B.shape[0], -1, np.int32); n = C.c_size_t()
    assert lib().hsp_unpack(form, _u32(B), _u32(out), st.ctypes.data_as(_I32P), B.shape[0], step, C.byref(n)) == 0
    return out, st, n.value


def verify_packed(A32, SIG, M, form, step=1 << 22):
    A32, SIG, M = _c(A32, np.uint8), _c(SIG, np.uint8), _c(M); st = np.full(M.shape[0], -1, np.int32); n = C.c_size_t()
    assert lib().hsp_verify_packed(form, _u32(A32), _u32(SIG), _u32(M), st.ctypes.data_as(_I32P), M.shape[0], step, C.byref(n)) == 0
    return st, n.value
