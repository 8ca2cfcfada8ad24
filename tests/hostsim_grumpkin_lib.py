"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_grumpkin.cpp (the bodies of bn_amd/csrc/grumpkin_ops.hpp and the replay of the segmented sum over
bn_dot_plan, compiled with g++ and -DBN_BOUNDS) as Python calls over the arrays of the C ABI, for tests/test_hostsim_grumpkin.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _I32P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
PATTERN = 0x5a5a5a5a5a5a5a5a
_libs = {}


def lib(window=4):
    """compiled the way hostsim_lib.py compiles its bound-enforcing library: g++ -DBN_BOUNDS, rebuilt when a source is newer; one library
    per window of [k]P (4 ships, 5 is the buildable variant)"""
    if window not in _libs:
        out = HERE / ("libhostsim_grumpkin.so" if window == 4 else "libhostsim_grumpkin_w%d.so" % window)
        srcs = [HERE / "hostsim_grumpkin.cpp", HERE / "lanepair.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-DBN254_GRUMPKIN_MUL_WINDOW=%d" % window,
                                   "-o", str(out), str(HERE / "hostsim_grumpkin.cpp")])
        l = C.CDLL(str(out))
        l.hsg_validate.argtypes = [_U32P, _I32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsg_add.argtypes = [_U32P, _U32P, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsg_mul.argtypes = [_U32P, _U32P, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsg_double_vs_add.argtypes = [_U32P, _U32P, _I32P, C.c_size_t]
        l.hsg_msm.argtypes = [_U32P, _U32P, _SZP, C.c_size_t, _U32P, C.c_size_t, _SZP, _SZP, _SZP]
        l.hsg_fan.restype = C.c_uint
        assert l.hsg_bounds_enabled() == 1 and l.hsg_window() == window
        _libs[window] = l
    return _libs[window]


def _u32(a):
    return a.ctypes.data_as(_U32P)


def _c(a):
    return np.ascontiguousarray(a, np.uint64)


def validate(P, step=1 << 22):
    """(n,2,4) uint64 -> ((n,) int32, sub-launches)"""
    P = _c(P); st = np.full(P.shape[0], -1, np.int32); n = C.c_size_t()
    assert lib().hsg_validate(_u32(P), st.ctypes.data_as(_I32P), P.shape[0], step, C.byref(n)) == 0
    return st, n.value


def add(P, Q, step=1 << 22, in_place=False):
    P, Q = _c(P).copy(), _c(Q); out = P if in_place else np.full_like(P, PATTERN); n = C.c_size_t()
    assert lib().hsg_add(_u32(P), _u32(Q), _u32(out), P.shape[0], step, C.byref(n)) == 0
    return out, n.value


def mul(P, K, step=1 << 22, in_place=False, window=4):
    """points and (n,4) uint64 plain scalars"""
    P, K = _c(P).copy(), _c(K); out = P if in_place else np.full_like(P, PATTERN); n = C.c_size_t()
    assert lib(window).hsg_mul(_u32(P), _u32(K), _u32(out), P.shape[0], step, C.byref(n)) == 0
    return out, n.value


def double_vs_add(P):
    """-> (the affine doublings, (n,) int32: bit 0 double(P) == add(P, P), bit 1 the same one doubling later)"""
    P = _c(P); out = np.full_like(P, PATTERN); ok = np.full(P.shape[0], -1, np.int32)
    assert lib().hsg_double_vs_add(_u32(P), _u32(out), ok.ctypes.data_as(_I32P), P.shape[0]) == 0
    return out, ok


def msm(P, K, offsets, step=1 << 22):
    """-> ((m,2,4) uint64, (slots, levels, launches)) or the error number of the checks"""
    P, K = _c(P).reshape(-1, 2, 4), _c(K).reshape(-1, 4); o = np.ascontiguousarray(offsets, np.uint64); m = o.size - 1
    out = np.full((m, 2, 4), PATTERN, np.uint64); s, lv, n = C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = lib().hsg_msm(_u32(P), _u32(K), o.ctypes.data_as(_SZP), m, _u32(out), step, C.byref(s), C.byref(lv), C.byref(n))
    return (out, (s.value, lv.value, n.value)) if rc == 0 else rc
