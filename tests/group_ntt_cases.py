"""TEST INFRASTRUCTURE - the model and the inputs of the tests of bn254_g{1,2}_ntt_batch (tests/test_hostsim_group_ntt.py on the CPU,
tests/test_gpu_group_ntt.py on the GPU).  The model is the direct O(n^2) sum of the definition with the oracle's g*_mul / g*_add /
g*_normalize (oracle/bn_oracle.py, the reference's own chains in C); the roots are those of tests/ntt_cases.py.  Expected bytes are
normalised points, hence unique: (x / z^2, y / z^3, 1), the point at infinity as (0, 1, 0)."""
import functools

import numpy as np

import bn_model as M
import fr_cases as FC
import normalize_cases as ZC
import ntt_cases as NC

R = FC.R
WORDS = ZC.WORDS
LOGS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def oracle():
    import bn_oracle
    bn_oracle.build()
    return bn_oracle.Oracle()


@functools.lru_cache(maxsize=None)
def hostsim():
    """tests/hostsim/hostsim_group_ntt.cpp compiled the way hostsim_lib.py compiles its library: g++, -DBN_BOUNDS, rebuilt when a source is newer"""
    import ctypes as C
    import pathlib
    import subprocess
    here = pathlib.Path(__file__).resolve().parent / "hostsim"
    csrc = here.parents[1] / "bn_amd" / "csrc"
    out = here / "libhostsim_group_ntt_bounds.so"
    srcs = [here / "hostsim_group_ntt.cpp", here / "lanepair.hpp", here / "lanequad.hpp", here.parents[1] / "include" / "bn254_hip.h"] + sorted(csrc.glob("*.hpp"))
    if (not out.exists()) or out.stat().st_mtime < max(s.stat().st_mtime for s in srcs):
        subprocess.check_call(["g++", "-DBN_BOUNDS", "-std=c++17", "-O1", "-fPIC", "-shared", "-fvisibility=hidden", "-o", str(out), str(here / "hostsim_group_ntt.cpp")])
    lib = C.CDLL(str(out))
    assert lib.hsg_bounds_enabled() == 1
    lib.hsg_chains.restype = C.c_size_t
    lib.hsg_plan.restype = C.c_size_t
    return lib


def _ops(g):
    o = oracle()
    return (o.g1_mul_batch, o.g1_add, o.g1_normalize, o.g1_zero()) if g == 1 else (o.g2_mul_batch, o.g2_add, o.g2_normalize, o.g2_zero())


def normalize(g, P):
    """rows -> their normalised rows; z == 0 is the point at infinity whatever x and y hold"""
    _, _, norm, zero = _ops(g)
    P = np.ascontiguousarray(P, np.uint64)
    third = WORDS[g] // 3
    return np.stack([norm(r) if r[2 * third:].any() else zero for r in P]) if len(P) else P.copy()


def coefficients(log_n, k, inverse=False, shift=None):
    """the n scalars output k sums its inputs with: s^j w^(j k) forward, n^-1 s^-k w^(-j k) inverse"""
    n = 1 << log_n
    s = 1 if shift is None else shift % R
    w = NC.root(log_n)
    if not inverse:
        return [pow(s, j, R) * pow(w, j * k % n, R) % R for j in range(n)]
    wi, c = pow(w, -1, R), pow(n, -1, R) * pow(pow(s, -1, R), k, R) % R
    return [c * pow(wi, j * k % n, R) % R for j in range(n)]


def model(g, P, log_n, inverse=False, shift=None):
    """len(P) / 2^log_n transforms of the rows P as include/bn254_hip.h defines bn254_g{1,2}_ntt_batch: every output the sum of its n terms"""
    mul, add, _, zero = _ops(g)
    P = np.ascontiguousarray(P, np.uint64)
    n = 1 << log_n
    assert P.shape[0] % n == 0 and P.shape[1] == WORDS[g]
    out = np.empty_like(P)
    for t in range(P.shape[0] // n):
        X = P[t * n:(t + 1) * n]
        for k in range(n):
            acc = zero
            for term in mul(X, FC.rows(coefficients(log_n, k, inverse, shift)), 1):
                acc = add(acc, term)
            out[t * n + k] = acc
    return normalize(g, out)


def inputs(g, log_n, seed):
    """{name: (n, words) rows}: distinct points in random representations (z = 1 and z = q - 1 among them); the same with points at
    infinity - (0, 1, 0) and garbage coordinates - between them; a constant vector (ONE group element in n representations: it doubles at
    every stage and cancels everywhere but at index 0); a single point that is not infinity (at index 1 where there is one); all infinity"""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    aff = ZC.affine(g)
    zero = M.g_zero(ZC.OPS[g])
    reg = lambda i: ZC.rep(g, aff[(5 * i + seed) % ZC.MULTIPLES], ZC.lam_of(rng, i))
    inf = lambda i: zero if i % 4 == 0 else ZC.garbage(g, rng)
    one = ZC.rep(g, aff[seed % ZC.MULTIPLES], ZC.lam_of(rng, 0))
    sets = {
        "random": [reg(i) for i in range(n)],
        "with infinity": [inf(i) if i % 2 == 0 else reg(i) for i in range(n)],
        "constant": [ZC.rep(g, aff[(seed + 3) % ZC.MULTIPLES], ZC.lam_of(rng, i)) for i in range(n)],
        "single": [one if i == min(1, n - 1) else inf(i) for i in range(n)],
        "all infinity": [inf(i) for i in range(n)],
    }
    return {name: ZC.rows(g, pts) for name, pts in sets.items()}


def batch(g, log_n, count, seed):
    """count transforms back to back: the input sets in turn, from a different one for every seed"""
    sets = inputs(g, log_n, seed)
    names = list(sets)
    return np.concatenate([sets[names[(seed + t) % len(names)]] for t in range(count)])


def shift_row(shift):
    return NC.shift_row(shift)
