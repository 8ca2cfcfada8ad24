"""TEST INFRASTRUCTURE - tests/hostsim/hostsim_wide.cpp (the double-width leaves of bn_amd/csrc/fe.hpp and the lazily reduced tower products
of tower.hpp on a simulated lane pair, compiled with g++ and -DBN_BOUNDS) as Python calls, for tests/test_hostsim_wide.py."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent / "hostsim"
CSRC = HERE.parents[1] / "bn_amd" / "csrc"
_U32P = C.POINTER(C.c_uint32)
MASK29 = (1 << 29) - 1
_lib = None


def lib():
    """compiled the way hostsim_lib.py compiles its bounds-checked library: g++, rebuilt when a source is newer"""
    global _lib
    if _lib is None:
        out = HERE / "libhostsim_wide.so"
        srcs = [HERE / "hostsim_wide.cpp", HERE / "rawleaf.hpp", HERE / "lanepair.hpp", HERE / "lanequad.hpp"] + sorted(CSRC.glob("*.hpp"))
        if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
            subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(HERE / "hostsim_wide.cpp")])
        _lib = C.CDLL(str(out))
        assert _lib.hsw_bounds_enabled() == 1
    return _lib


def _u32(a):
    return a.ctypes.data_as(_U32P)


def limbs9(v, signed=False):
    """an integer as nine limbs: 29 bits each, the top limb takes the rest; `signed`: every limb of a NEGATIVE value is negated (the form of
    fe_sdiff: each limb an int32 of magnitude below 2^29)"""
    neg = signed and v < 0
    m = -v if neg else v
    l = [(m >> (29 * i)) & MASK29 for i in range(8)] + [m >> 232]
    assert l[8] < (1 << 31)
    return np.array([(-x if neg else x) & 0xffffffff for x in l], np.uint32)


def limbs_value(l, signed_limbs=False, top_signed=False):
    """sum l[i] 2^(29 i); `signed_limbs`: every limb an int32; `top_signed`: only the top one"""
    n = len(l)
    out = 0
    for i, x in enumerate(int(x) for x in l):
        if (signed_limbs or (top_signed and i == n - 1)) and x >> 31:
            x -= 1 << 32
        out += x << (29 * i)
    return out


def limbs18(v):
    """a (signed) integer as the 18-limb wide form: limbs 0..16 in [0, 2^29), the sign in the top limb"""
    l = [(v >> (29 * i)) & MASK29 for i in range(17)] + [v >> (29 * 17)]
    assert -(1 << 31) <= l[17] < (1 << 31)
    return np.array([x & 0xffffffff for x in l], np.uint32)


def wmul2(signed, a, u, c, v, bounds):
    """18 limbs of a*u + c*v; a, u, c, v: nine-limb arrays, bounds: (lb, vb) x 4"""
    o = np.zeros(18, np.uint32)
    b = np.array(bounds, np.uint32).reshape(8)
    lib().hsw_wmul2(int(signed), _u32(a), _u32(u), _u32(c), _u32(v), _u32(b), _u32(o))
    return o


def wadd(x, y, bounds):
    o = np.zeros(18, np.uint32)
    b = np.array(bounds, np.uint32).reshape(4)
    lib().hsw_wadd(_u32(x), _u32(y), _u32(b), _u32(o))
    return o


def wred(xi, sub, n, x, px, neg, d, bounds):
    """nine limbs of reduce(n + [xi](9 x -+ px)) - [sub] d; bounds: (lb, wb) of n, x, px and (lb, vb) of d"""
    o = np.zeros(9, np.uint32)
    b = np.array(bounds, np.uint32).reshape(8)
    lib().hsw_wred(int(xi), int(sub), _u32(n), _u32(x), _u32(px), int(neg), _u32(d), _u32(b), _u32(o))
    return o


def _call(fn, *args, words=96):
    o = np.zeros(words // 2, np.uint64)
    conv, keep = [], []
    for a in args:
        if isinstance(a, (int, np.integer)):
            conv.append(C.c_int(int(a)))
        else:
            a = np.ascontiguousarray(a, dtype=np.uint64); keep.append(a)
            conv.append(a.ctypes.data_as(_U32P))
    getattr(lib(), fn)(*conv, o.ctypes.data_as(_U32P))
    return o


def _f6(a):
    """an Fq6 (24 words of uint64) as the c0 half of an Fq12 record"""
    return np.concatenate([np.asarray(a, np.uint64), np.zeros(24, np.uint64)])


def fq6_mul(a, b, wide=True): return _call("hsw_fq6_mul", int(wide), _f6(a), _f6(b))[:24]
def fq6_mul_sub(a, b, d): return _call("hsw_fq6_mul_sub", _f6(a), _f6(b), _f6(d))[:24]
def fq12_mul(a, b, wide=True, conj=False): return _call("hsw_fq12_mul", int(wide), int(conj), a, b)
def fq12_sqr(a, wide=True, reduced_c1=False): return _call("hsw_fq12_sqr", int(wide), int(reduced_c1), a)
def fq12_sqr_chain(a, n, reduced_c1): return _call("hsw_fq12_sqr_chain", int(reduced_c1), int(n), a)


def _call2(fn, *args):
    """two outputs: the even and the odd slot"""
    oe, oo = np.zeros(48, np.uint64), np.zeros(48, np.uint64)
    conv, keep = [], []
    for a in args:
        if isinstance(a, (int, np.integer)):
            conv.append(C.c_int(int(a)))
        else:
            a = np.ascontiguousarray(a, dtype=np.uint64); keep.append(a)
            conv.append(a.ctypes.data_as(_U32P))
    getattr(lib(), fn)(*conv, oe.ctypes.data_as(_U32P), oo.ctypes.data_as(_U32P))
    return oe, oo


# two lane pairs side by side (the even and the odd slot of a batch), each with its own operands: (result of the even slot, of the odd slot)
def fq12_mul_slots(a_even, b_even, a_odd, b_odd): return _call2("hsw_fq12_mul_slots", a_even, b_even, a_odd, b_odd)
def fq12_sqr_slots(a_even, a_odd, reduced_c1=False): return _call2("hsw_fq12_sqr_slots", int(reduced_c1), a_even, a_odd)
def fq6_mul_slots(a_even, b_even, a_odd, b_odd): return tuple(r[:24] for r in _call2("hsw_fq6_mul_slots", _f6(a_even), _f6(b_even), _f6(a_odd), _f6(b_odd)))


def macs(what, a, b):
    """multiply instructions per lane of: 0 f6_mul_lazy, 1 f6_mul, 2 / 3 f12_mul lazy / eager, 4 / 5 f12_sqr lazy / eager"""
    m = C.c_ulong()
    a = np.ascontiguousarray(a, np.uint64); b = np.ascontiguousarray(b, np.uint64)
    lib().hsw_counts(int(what), _u32(a), _u32(b), C.byref(m))
    return m.value
