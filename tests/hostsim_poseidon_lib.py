"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_poseidon.cpp (the bodies of bn_amd/csrc/poseidon_ops.hpp and the checks and level arithmetic of
host_plan.hpp, compiled with g++ and -DBN_BOUNDS) as Python calls over integer lists, for tests/test_hostsim_poseidon.py and
tests/test_poseidon_abi.py.  Two libraries, whichever of the two the product ships: the plain matrix rows, and (fused=True) the rows as the product-sum fr_dot of fr.hpp."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

import poseidon_cases as PC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _U64P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
PATTERN = 0x5a5a5a5a5a5a5a5a
_libs = {}


def lib(fused=False):
    """compiled the way hostsim_lib.py compiles its bound-enforcing library: g++ -DBN_BOUNDS, rebuilt when a source is newer"""
    if fused not in _libs:
        out = HERE / ("libhostsim_poseidon_fused.so" if fused else "libhostsim_poseidon.so")
        srcs = [HERE / "hostsim_poseidon.cpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden"] + ["-DBN254_POSEIDON_FUSED_ROW=%d" % int(fused)] +
                                  ["-o", str(out), str(HERE / "hostsim_poseidon.cpp")])
        l = C.CDLL(str(out))
        l.hsp_poseidon_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        l.hsp_merkle_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        l.hsp_merkle_plan.restype = C.c_size_t
        l.hsp_merkle_plan.argtypes = [C.c_int, C.c_size_t, _U64P, C.c_size_t]
        l.hsp_hash.argtypes = [_U32P, C.c_int, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsp_permute.argtypes = [_U32P, C.c_int, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hsp_merkle.argtypes = [_U32P, C.c_int, _U32P, C.c_size_t, _SZP]
        l.hsp_dot.argtypes = [C.c_int, _U32P, _U32P, _U32P]
        assert l.hsp_bounds_enabled() == 1 and l.hsp_fused_row() == int(fused)
        _libs[fused] = l
    return _libs[fused]


def _u32(a):
    return a.ctypes.data_as(_U32P)


def hash_(inputs, step=1 << 22, fused=False):
    """rows of `arity` integers -> ((n, 4) uint64, sub-launches)"""
    arity = len(inputs[0])
    X = PC.rows(inputs)
    out = np.full((len(inputs), 4), PATTERN, np.uint64)
    n = C.c_size_t()
    rc = lib(fused).hsp_hash(_u32(X), arity, _u32(out), len(inputs), step, C.byref(n))
    assert rc == 0, rc
    return out, n.value


def permute(states, step=1 << 22, in_place=False, fused=False):
    """states of t integers -> ((n * t, 4) uint64, sub-launches)"""
    t = len(states[0])
    X = PC.rows(states)
    out = X if in_place else np.full((len(states) * t, 4), PATTERN, np.uint64)
    n = C.c_size_t()
    rc = lib(fused).hsp_permute(_u32(X), t, _u32(out), len(states), step, C.byref(n))
    assert rc == 0, rc
    return out, n.value


def merkle(leaves, step=1 << 22, fused=False):
    """2^k integers -> ((n - 1, 4) uint64, sub-launches)"""
    log_n = len(leaves).bit_length() - 1
    X = PC.rows(leaves)
    out = np.full((max(len(leaves) - 1, 1), 4), PATTERN, np.uint64)
    n = C.c_size_t()
    rc = lib(fused).hsp_merkle(_u32(X), log_n, _u32(out), step, C.byref(n))
    assert rc == 0, rc
    return out[:len(leaves) - 1], n.value


def merkle_plan(log_n, step=1 << 22):
    """levels as (cnt, src, dst, parts, from_leaves) rows"""
    levels = np.zeros((64, 5), np.uint64)
    count = lib().hsp_merkle_plan(log_n, step, levels.ctypes.data_as(_U64P), 64)
    return levels[:count].astype(np.int64)


def dot(a, b):
    """sum a[k] b[k] mod r through fr_dot<len(a)> under its bound checks -> (4,) uint64"""
    A, B = PC.rows(a), PC.rows(b)
    out = np.zeros((1, 4), np.uint64)
    rc = lib(True).hsp_dot(len(a), _u32(A), _u32(B), _u32(out))
    assert rc == 0, rc
    return out[0]
