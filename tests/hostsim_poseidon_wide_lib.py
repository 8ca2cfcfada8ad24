"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_poseidon_wide.cpp (the bodies of bn_amd/csrc/poseidon_wide_ops.hpp, the table derivation of
poseidon_wide_table.hpp and the checks of host_plan.hpp, compiled with g++ and -DBN_BOUNDS) as Python calls over integer lists, for
tests/test_hostsim_poseidon_wide.py and tests/test_poseidon_wide_abi.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

import poseidon_wide_cases as WC

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _SZP = C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)
PATTERN = 0x5a5a5a5a5a5a5a5a
_lib = None


def lib():
    """compiled the way hostsim_lib.py compiles its bound-enforcing library: g++ -DBN_BOUNDS, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_poseidon_wide.so"
        srcs = [HERE / "hostsim_poseidon_wide.cpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_poseidon_wide.cpp")])
        l = C.CDLL(str(out))
        l.hspw_table_elems.restype = C.c_size_t
        l.hspw_table_elems.argtypes = [C.c_int]
        l.hspw_rounds_partial.argtypes = [C.c_int]
        l.hspw_table.argtypes = [C.c_int, _U32P]
        l.hspw_ex_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]
        l.hspw_chain_check.argtypes = [C.c_void_p, _SZP, C.c_size_t, C.c_int, C.c_void_p, C.c_int]
        l.hspw_ex.argtypes = [C.c_int, _U32P, C.c_int, _U32P, C.c_int, _U32P, C.c_size_t, C.c_size_t, _SZP]
        l.hspw_chain.argtypes = [C.c_int, _U32P, _SZP, C.c_size_t, C.c_int, _U32P, C.c_size_t, _SZP]
        assert l.hspw_bounds_enabled() == 1
        _lib = l
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def table(t):
    """the C++ derivation of width t -> (C, M) as Python integers (out of Montgomery form)"""
    n = lib().hspw_table_elems(t)
    raw = np.zeros((n, 4), np.uint64)
    assert lib().hspw_table(t, _u32(raw)) == 0
    return split_table(t, raw)


def split_table(t, raw):
    """(table_elems, 4) uint64 Montgomery images -> (C, M): the round constants and the matrix rows as integers"""
    inv = pow(1 << 256, -1, WC.R)
    vals = [sum(int(w) << (64 * i) for i, w in enumerate(r)) for r in np.asarray(raw, np.uint64).reshape(-1, 4)]
    assert all(v < WC.R for v in vals), "a table entry is not canonical"
    vals = [v * inv % WC.R for v in vals]
    nc = (WC.FULL + WC.PARTIAL[t]) * t
    assert len(vals) == nc + t * t
    return vals[:nc], [vals[nc + i * t:nc + (i + 1) * t] for i in range(t)]


def ex(G, inputs, init=None, n_outs=1, step=1 << 22):
    """rows of n_inputs integers (and one init per row, or None) -> ((n * n_outs, 4) uint64, sub-launches)"""
    n_inputs = len(inputs[0])
    X = WC.rows(inputs)
    I = WC.rows(init) if init is not None else None
    out = np.full((len(inputs) * n_outs, 4), PATTERN, np.uint64)
    n = C.c_size_t()
    rc = lib().hspw_ex(G, _u32(X), n_inputs, _u32(I) if I is not None else None, n_outs, _u32(out), len(inputs), step, C.byref(n))
    assert rc == 0, rc
    return out, n.value


def chain(G, flat, offsets, rate, step=1 << 22):
    """records as (flat integers, offsets) -> ((m, 4) uint64, sub-launches)"""
    X = WC.rows(flat)
    off = np.ascontiguousarray(offsets, np.uint64)
    m = len(off) - 1
    out = np.full((max(m, 1), 4), PATTERN, np.uint64)
    n = C.c_size_t()
    rc = lib().hspw_chain(G, _u32(X) if len(flat) else None, off.ctypes.data_as(_SZP), m, rate, _u32(out), step, C.byref(n))
    assert rc == 0, rc
    return out[:m], n.value
