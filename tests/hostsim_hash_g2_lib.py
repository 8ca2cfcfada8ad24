"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_hash_g2.cpp (the bodies of bn_amd/csrc/hash_g2_ops.hpp, compiled with g++ and -DBN_BOUNDS) as
Python calls over integers, bytes and arrays, for tests/test_hostsim_hash_g2.py."""
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
        out = HERE / "libhostsim_hash_g2.so"
        srcs = [HERE / "hostsim_hash_g2.cpp", HERE / "lanepair.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_hash_g2.cpp")])
        l = C.CDLL(str(out))
        l.hsg_field.argtypes = [_U8P, _U32P]
        l.hsg_field.restype = C.c_uint32
        l.hsg_inv0.argtypes = [_U32P, _U32P]
        l.hsg_inv0.restype = C.c_int
        l.hsg_map.argtypes = [_U8P, _U32P, C.c_size_t]
        l.hsg_clear.argtypes = [_U32P, _U32P, C.c_size_t]
        l.hsg_psi.argtypes = [C.c_int, _U32P, _U32P]
        l.hsg_hash_uniform.argtypes = [_U8P, _U32P, C.c_size_t]
        l.hsg_hash_msg.argtypes = [_U8P, C.c_size_t, _U8P, C.c_uint32, _U32P, C.c_size_t]
        l.hsg_expand.argtypes = [_U8P, C.c_size_t, _U8P, C.c_uint32, _U8P]
        for f in (l.hsg_map, l.hsg_clear, l.hsg_psi, l.hsg_hash_uniform, l.hsg_hash_msg, l.hsg_expand):
            f.restype = None
        assert l.hsg_bounds_enabled() == 1
        _lib = l
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def _u8(a):
    return a.ctypes.data_as(_U8P)


def _bytes(b):
    a = np.frombuffer(bytes(b), np.uint8).copy()
    return a if a.size else np.zeros(1, np.uint8)


def _f2_words(a):
    return np.array(M.to_mont_limbs(a[0] % M.Q) + M.to_mont_limbs(a[1] % M.Q), np.uint64)


def _f2_of(row):
    return (M.from_mont_limbs(row[0:4]), M.from_mont_limbs(row[4:8]))


def field(c0, c1):
    """two 48-byte integers -> ((c0 mod q, c1 mod q), sgn0), through the device's reduction"""
    out = np.zeros(8, np.uint64)
    s = lib().hsg_field(_u8(_bytes(int(c0).to_bytes(48, "big") + int(c1).to_bytes(48, "big"))), _u32(out))
    return _f2_of(out), int(s)


def inv0(a):
    """-> (inv0(a), is_square(a))"""
    x = _f2_words(a); out = np.zeros(8, np.uint64)
    sq = lib().hsg_inv0(_u32(x), _u32(out))
    return _f2_of(out), bool(sq)


def map_to_curve(u):
    """(n, 96) uint8 -> (n, 24) uint64"""
    u = np.ascontiguousarray(u, np.uint8).reshape(-1, 96)
    out = np.zeros((u.shape[0], 24), np.uint64)
    lib().hsg_map(_u8(u), _u32(out), u.shape[0])
    return out


def clear_cofactor(p, in_place=False):
    """(n, 24) uint64 Jacobian points -> (n, 24) uint64"""
    p = np.ascontiguousarray(p, np.uint64).reshape(-1, 24).copy()
    out = p if in_place else np.zeros_like(p)
    lib().hsg_clear(_u32(p), _u32(out), p.shape[0])
    return out


def psi(j, p):
    """one (24,) uint64 Jacobian point -> psi^j of it, as it stands"""
    p = np.ascontiguousarray(p, np.uint64).copy(); out = np.zeros(24, np.uint64)
    lib().hsg_psi(j, _u32(p), _u32(out))
    return out


def hash_uniform(uniform):
    """(n, 192) uint8 -> (n, 24) uint64"""
    b = np.ascontiguousarray(uniform, np.uint8).reshape(-1, 192)
    out = np.zeros((b.shape[0], 24), np.uint64)
    lib().hsg_hash_uniform(_u8(b), _u32(out), b.shape[0])
    return out


def hash_msgs(msgs, dst):
    """(n, msg_len) uint8, DST -> (n, 24) uint64"""
    msgs = np.ascontiguousarray(msgs, np.uint8)
    n, ml = msgs.shape
    dp = _bytes(bytes(dst) + bytes([len(dst)]))
    out = np.zeros((n, 24), np.uint64)
    lib().hsg_hash_msg(_u8(msgs if msgs.size else np.zeros(1, np.uint8)), ml, _u8(dp), len(dst) + 1, _u32(out), n)
    return out


def expand(msg, dst):
    """expand_message_xmd(msg, dst, 192)"""
    dp = _bytes(bytes(dst) + bytes([len(dst)]))
    out = np.zeros(192, np.uint8)
    lib().hsg_expand(_u8(_bytes(msg)), len(msg), _u8(dp), len(dst) + 1, _u8(out))
    return out.tobytes()
