"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_hash.cpp (the bodies of bn_amd/csrc/hash_ops.hpp, compiled with g++ and -DBN_BOUNDS) as Python
calls over integers, bytes and arrays, for tests/test_hostsim_hash.py.  `inv0` selects the form of inv0: 0 fe_inverse_fermat, 1 the candidate
chain."""
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
        out = HERE / "libhostsim_hash.so"
        srcs = [HERE / "hostsim_hash.cpp", HERE / "lanepair.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_hash.cpp")])
        l = C.CDLL(str(out))
        l.hsh_field.argtypes = [_U8P, _U32P]
        l.hsh_inv0.argtypes = [C.c_int, _U32P, _U32P]
        l.hsh_map.argtypes = [C.c_int, _U8P, _U32P, C.c_size_t]
        l.hsh_hash_uniform.argtypes = [C.c_int, _U8P, _U32P, C.c_size_t]
        l.hsh_hash_msg.argtypes = [C.c_int, _U8P, C.c_size_t, _U8P, C.c_uint32, _U32P, C.c_size_t]
        l.hsh_expand.argtypes = [_U8P, C.c_size_t, _U8P, C.c_uint32, _U8P]
        for f in (l.hsh_field, l.hsh_inv0, l.hsh_map, l.hsh_hash_uniform, l.hsh_hash_msg, l.hsh_expand):
            f.restype = None
        assert l.hsh_bounds_enabled() == 1
        _lib = l
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def _u8(a):
    return a.ctypes.data_as(_U8P)


def _bytes(b):
    a = np.frombuffer(bytes(b), np.uint8).copy()
    return a if a.size else np.zeros(1, np.uint8)


def field(v):
    """a 48-byte integer -> its value mod q, through the device's reduction"""
    out = np.zeros(4, np.uint64)
    lib().hsh_field(_u8(_bytes(int(v).to_bytes(48, "big"))), _u32(out))
    return M.from_mont_limbs(out)


def inv0(a, form):
    x = np.array(M.to_mont_limbs(a % M.Q), np.uint64); out = np.zeros(4, np.uint64)
    lib().hsh_inv0(form, _u32(x), _u32(out))
    return M.from_mont_limbs(out)


def map_to_curve(u, form):
    """(n, 48) uint8 -> (n, 12) uint64"""
    u = np.ascontiguousarray(u, np.uint8).reshape(-1, 48)
    out = np.zeros((u.shape[0], 12), np.uint64)
    lib().hsh_map(form, _u8(u), _u32(out), u.shape[0])
    return out


def hash_uniform(uniform, form):
    """(n, 96) uint8 -> (n, 12) uint64"""
    b = np.ascontiguousarray(uniform, np.uint8).reshape(-1, 96)
    out = np.zeros((b.shape[0], 12), np.uint64)
    lib().hsh_hash_uniform(form, _u8(b), _u32(out), b.shape[0])
    return out


def hash_msgs(msgs, dst, form):
    """(n, msg_len) uint8, DST -> (n, 12) uint64"""
    msgs = np.ascontiguousarray(msgs, np.uint8)
    n, ml = msgs.shape
    dp = _bytes(bytes(dst) + bytes([len(dst)]))
    out = np.zeros((n, 12), np.uint64)
    lib().hsh_hash_msg(form, _u8(msgs if msgs.size else np.zeros(1, np.uint8)), ml, _u8(dp), len(dst) + 1, _u32(out), n)
    return out


def expand(msg, dst):
    """expand_message_xmd(msg, dst, 96)"""
    dp = _bytes(bytes(dst) + bytes([len(dst)]))
    out = np.zeros(96, np.uint8)
    lib().hsh_expand(_u8(_bytes(msg)), len(msg), _u8(dp), len(dst) + 1, _u8(out))
    return out.tobytes()
