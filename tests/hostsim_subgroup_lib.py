"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_subgroup.cpp (the bodies of bn_amd/csrc/subgroup_ops.hpp and the G2 decoders of io_wire.hpp and
io_compress.hpp, compiled with g++ and -DBN_BOUNDS) as Python calls over arrays and bytes, for tests/test_hostsim_subgroup.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _U8P, _I32P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
_lib = None


def lib():
    """compiled the way hostsim_hash_g2_lib.py compiles its bound-enforcing library: g++ -DBN_BOUNDS, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_subgroup.so"
        srcs = [HERE / "hostsim_subgroup.cpp", HERE / "lanepair.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_subgroup.cpp")])
        l = C.CDLL(str(out))
        l.hss_g1_validate.argtypes = [_U32P, _I32P, C.c_size_t]
        l.hss_g2_validate.argtypes = [_U32P, _I32P, C.c_size_t]
        l.hss_g1_validate.restype = l.hss_g2_validate.restype = None
        for f in (l.hss_endo, l.hss_chain, l.hss_decoder_test):
            f.argtypes = [_U32P]
        l.hss_g2_decode.argtypes = [_U8P, _U32P]
        l.hss_g2_decompress.argtypes = [C.c_int, _U8P, C.c_int, _U32P]
        assert l.hss_bounds_enabled() == 1
        _lib = l
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def decoders_use_endo():
    return bool(lib().hss_decoders_use_endo())


def validate(g, rows):
    """(n, 12 g) uint64 records -> (n,) int32 statuses; the records come back untouched"""
    p = np.ascontiguousarray(rows, np.uint64).reshape(-1, 12 * g).copy()
    keep = p.copy()
    st = np.full(p.shape[0], -1, np.int32)
    (lib().hss_g1_validate if g == 1 else lib().hss_g2_validate)(_u32(p), st.ctypes.data_as(_I32P), p.shape[0])
    assert np.array_equal(p, keep)
    return st


def endo(row):
    """the endomorphism test on one (24,) uint64 Jacobian record"""
    return bool(lib().hss_endo(_u32(np.ascontiguousarray(row, np.uint64).copy())))


def chain(xy):
    """the r - 1 chain on one affine pair: (16,) uint64, x then y"""
    return bool(lib().hss_chain(_u32(np.ascontiguousarray(xy, np.uint64).copy())))


def decoder_test(xy):
    """g2_in_subgroup as the decoders call it"""
    return bool(lib().hss_decoder_test(_u32(np.ascontiguousarray(xy, np.uint64).copy())))


def g2_decode(record):
    """one 129-byte wire record -> (status, (24,) uint64)"""
    b = np.frombuffer(bytes(record), np.uint8).copy()
    out = np.zeros(24, np.uint64)
    return lib().hss_g2_decode(b.ctypes.data_as(_U8P), _u32(out)), out


def g2_decompress(record, fmt, form):
    """one 64-byte compressed record -> (status, (24,) uint64)"""
    b = np.frombuffer(bytes(record), np.uint8).copy()
    out = np.zeros(24, np.uint64)
    return lib().hss_g2_decompress(form, b.ctypes.data_as(_U8P), fmt, _u32(out)), out
