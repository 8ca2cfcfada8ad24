"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_babyjub.cpp (the bodies of bn_amd/csrc/babyjub_ops.hpp and the width-6 permutation, compiled with
g++ and -DBN_BOUNDS) as Python calls over the arrays of the C ABI, for tests/test_hostsim_babyjub.py.  Two libraries: the width-6 matrix row
as fr_dot<5> plus a product (split=False, what ships) and as two fr_dot<3> (split=True); both joint windows of the verifier are in each."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _I32P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
PATTERN = 0x5a5a5a5a5a5a5a5a
_libs = {}


def lib(split=False):
    """compiled the way hostsim_lib.py compiles its bound-enforcing library: g++ -DBN_BOUNDS, rebuilt when a source is newer"""
    if split not in _libs:
        out = HERE / ("libhostsim_babyjub_split.so" if split else "libhostsim_babyjub.so")
        srcs = [HERE / "hostsim_babyjub.cpp", HERE / "lanepair.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-DBN254_POSEIDON_ROW6_SPLIT=%d" % int(split),
                                   "-o", str(out), str(HERE / "hostsim_babyjub.cpp")])
        l = C.CDLL(str(out))
        l.hsb_validate.argtypes = [_U32P, _I32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsb_add.argtypes = [_U32P, _U32P, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsb_mul.argtypes = [_U32P, _U32P, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsb_mul_raw.argtypes = [_U32P, _U32P, _U32P, C.c_size_t]
        l.hsb_challenge.argtypes = [_U32P, _U32P, _U32P, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsb_verify.argtypes = [C.c_int, _U32P, _U32P, _U32P, _U32P, _I32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsb_permute6.argtypes = [_U32P, _U32P, C.c_size_t]
        assert l.hsb_bounds_enabled() == 1 and l.hsb_row6_split() == int(split)
        _libs[split] = l
    return _libs[split]


def _u32(a):
    return a.ctypes.data_as(_U32P)


def _c(a):
    return np.ascontiguousarray(a, np.uint64)


def validate(P, step=1 << 22, split=False):
    """(n,2,4) uint64 -> ((n,) int32, sub-launches)"""
    P = _c(P); st = np.full(P.shape[0], -1, np.int32); n = C.c_size_t()
    assert lib(split).hsb_validate(_u32(P), st.ctypes.data_as(_I32P), P.shape[0], step, C.byref(n)) == 0
    return st, n.value


def add(P, Q, step=1 << 22, in_place=False):
    P, Q = _c(P).copy(), _c(Q); out = P if in_place else np.full_like(P, PATTERN); n = C.c_size_t()
    assert lib().hsb_add(_u32(P), _u32(Q), _u32(out), P.shape[0], step, C.byref(n)) == 0
    return out, n.value


def mul(P, K, step=1 << 22, in_place=False):
    P, K = _c(P).copy(), _c(K); out = P if in_place else np.full_like(P, PATTERN); n = C.c_size_t()
    assert lib().hsb_mul(_u32(P), _u32(K), _u32(out), P.shape[0], step, C.byref(n)) == 0
    return out, n.value


def mul_raw(P, ks):
    """points and plain integers below 2^256 -> (n,2,4) uint64"""
    P = _c(P); K = np.array([[(k >> (64 * j)) & ((1 << 64) - 1) for j in range(4)] for k in ks], np.uint64); out = np.full_like(P, PATTERN)
    assert lib().hsb_mul_raw(_u32(P), _u32(K), _u32(out), P.shape[0]) == 0
    return out


def challenge(A, R8, M, step=1 << 22, split=False):
    A, R8, M = _c(A), _c(R8), _c(M); out = np.full_like(M, PATTERN); n = C.c_size_t()
    assert lib(split).hsb_challenge(_u32(A), _u32(R8), _u32(M), _u32(out), M.shape[0], step, C.byref(n)) == 0
    return out, n.value


def verify(A, R8, S, M, window, step=1 << 22, split=False):
    A, R8, S, M = _c(A), _c(R8), _c(S), _c(M); st = np.full(M.shape[0], -1, np.int32); n = C.c_size_t()
    assert lib(split).hsb_verify(window, _u32(A), _u32(R8), _u32(S), _u32(M), st.ctypes.data_as(_I32P), M.shape[0], step, C.byref(n)) == 0
    return st, n.value


def permute6(X, split=False):
    """(n,6,4) uint64 states -> the permuted states"""
    X = _c(X); out = np.full_like(X, PATTERN)
    assert lib(split).hsb_permute6(_u32(X), _u32(out), X.shape[0]) == 0
    return out
