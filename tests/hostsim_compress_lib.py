"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_compress.cpp (the square roots of bn_amd/csrc/sqrt_ops.hpp and the record bodies of
io_compress.hpp, compiled with g++ and -DBN_BOUNDS) as Python calls over integers and bytes, for tests/test_hostsim_compress.py.  `form`
selects the exponentiation chain: 0 square-and-multiply, 1 the fixed 4-bit window."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

import bn_model as M

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P, _U8P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
_lib = None


def lib():
    """compiled the way hostsim_lib.py compiles its bound-enforcing library: g++ -DBN_BOUNDS, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_compress.so"
        srcs = [HERE / "hostsim_compress.cpp", HERE / "lanepair.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_compress.cpp")])
        l = C.CDLL(str(out))
        l.hsc_fe_sqrt_cand.argtypes = [C.c_int, _U32P, _U32P, _U32P, _U32P]
        l.hsc_f2_sqrt.argtypes = [C.c_int, _U32P, _U32P]
        l.hsc_fe_sign.argtypes = [_U32P]
        l.hsc_f2_sign.argtypes = [_U32P]
        l.hsc_g1_compress.argtypes = [_U32P, C.c_int, _U8P]
        l.hsc_g2_compress.argtypes = [_U32P, C.c_int, _U8P]
        l.hsc_g1_decompress.argtypes = [C.c_int, _U8P, C.c_int, _U32P]
        l.hsc_g2_decompress.argtypes = [C.c_int, _U8P, C.c_int, _U32P]
        assert l.hsc_bounds_enabled() == 1
        _lib = l
    return _lib


def _mont(*ints):
    return np.array([l for a in ints for l in M.to_mont_limbs(a % M.Q)], np.uint64)


def _ints(a):
    return [M.from_mont_limbs(a[4 * i:4 * i + 4]) for i in range(len(a) // 4)]


def _u32(a):
    return a.ctypes.data_as(_U32P)


def _u8(a):
    return a.ctypes.data_as(_U8P)


def fe_sqrt_cand(a, form):
    """-> (t, y, chi) as canonical integers"""
    x = _mont(a); out = [np.zeros(4, np.uint64) for _ in range(3)]
    lib().hsc_fe_sqrt_cand(form, _u32(x), *[_u32(o) for o in out])
    return tuple(_ints(o)[0] for o in out)


def f2_sqrt(a, form):
    """-> (root, is_square)"""
    x = _mont(*a); out = np.zeros(8, np.uint64)
    sq = lib().hsc_f2_sqrt(form, _u32(x), _u32(out))
    return tuple(_ints(out)), bool(sq)


def fe_sign(a):
    return lib().hsc_fe_sign(_u32(_mont(a)))


def f2_sign(a):
    return lib().hsc_f2_sign(_u32(_mont(*a)))


def compress(g, point_words, fmt):
    p = np.ascontiguousarray(point_words, np.uint64)
    out = np.zeros(32 * g, np.uint8)
    (lib().hsc_g1_compress if g == 1 else lib().hsc_g2_compress)(_u32(p), fmt, _u8(out))
    return out.tobytes()


def decompress(g, record, fmt, form):
    """-> (status, 12 / 24 uint64)"""
    b = np.frombuffer(bytes(record), np.uint8).copy()
    out = np.zeros(12 * g, np.uint64)
    st = (lib().hsc_g1_decompress if g == 1 else lib().hsc_g2_decompress)(form, _u8(b), fmt, _u32(out))
    return st, out
