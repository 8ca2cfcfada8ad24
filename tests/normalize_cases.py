"""TEST INFRASTRUCTURE - inputs and expected values of the normalize / eq tests (tests/test_hostsim_normalize.py on the CPU,
tests/test_gpu_normalize.py on the GPU), built with bn_model's exact arithmetic from known affine points (small multiples of the
generators): a point (x, y) is re-represented as (l^2 x, l^3 y, l z) with l random, l = 1 (z = 1) and l = q - 1."""
import functools

import numpy as np

import bn_model as M

Q = M.Q
OPS = {1: M.FQ_OPS, 2: M.FQ2_OPS}
WORDS = {1: 12, 2: 24}
_G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
            11559732032986387107991004021392285783925812861821192530917403151452391805634),
           (8495653923123431417604973247489272438418190587263600148770280649306958101930,
            4082367875863433681332203403145435568316851327593401208105741076214120093531))
MULTIPLES = 24


def _scalar(g, v):
    return v % Q if g == 1 else (v % Q, 0)


@functools.lru_cache(maxsize=None)
def affine(g):
    """(x, y) of j * generator for j = 1 .. MULTIPLES, at index j - 1"""
    o = OPS[g]
    gen = (1, 2, 1) if g == 1 else (_G2_GEN[0], _G2_GEN[1], M.F2_ONE)
    out, acc = [], gen
    for _ in range(MULTIPLES):
        out.append(M.g_to_affine(o, acc))
        acc = M.g_add(o, acc, gen)
    return out


def rep(g, xy, lam):
    """(l^2 x, l^3 y, l): another Jacobian representation of the affine point"""
    o = OPS[g]
    l = _scalar(g, lam)
    l2 = o.mul(l, l)
    return (o.mul(xy[0], l2), o.mul(xy[1], o.mul(l2, l)), l)


def lam_of(rng, kind):
    return (int.from_bytes(rng.bytes(40), "little") % (Q - 2) + 2, 1, Q - 1)[kind % 3]


def garbage(g, rng):
    """a point at infinity whose x and y hold arbitrary non-zero values"""
    r = lambda: int.from_bytes(rng.bytes(40), "little") % (Q - 1) + 1
    return (r(), r(), 0) if g == 1 else ((r(), r()), (r(), r()), M.F2_ZERO)


def model_normalize(g, p):
    """lib.rs:88-95 with the point at infinity as G::zero(), whatever its x and y hold"""
    o = OPS[g]
    return M.g_zero(o) if M.g_is_zero(o, p) else M.g_normalize(o, p)


def model_eq(g, p, q):
    """PartialEq for G<P>, groups/mod.rs:83-109, restated"""
    o = OPS[g]
    pz, qz = M.g_is_zero(o, p), M.g_is_zero(o, q)
    if pz or qz:
        return pz and qz
    z1s, z2s = o.mul(p[2], p[2]), o.mul(q[2], q[2])
    if o.mul(p[0], z2s) != o.mul(q[0], z1s):
        return False
    return o.mul(p[1], o.mul(z2s, q[2])) == o.mul(q[1], o.mul(z1s, p[2]))


def rows(g, pts):
    """model points -> (n, 12 / 24) uint64 rows in the reference's memory image"""
    out = np.zeros((len(pts), WORDS[g]), np.uint64)
    for i, p in enumerate(pts):
        flat = list(p) if g == 1 else [c for two in p for c in two]
        out[i] = [w for c in flat for w in M.to_mont_limbs(c)]
    return out


def points(g, n, K, phase, seed):
    """n model points in runs of K; run r + phase (mod 6) is: 0 - distinct points, the three kinds of l in turn (so z = 1 is there);
    1 - all infinity, (0, 1, 0) and garbage coordinates alternating; 2 / 3 / 4 - infinity at the first / a middle / the last position;
    5 - the same point (the same bytes) K times"""
    rng = np.random.default_rng(seed)
    aff = affine(g)
    zero = M.g_zero(OPS[g])
    pts = []
    for i in range(n):
        r, pos = divmod(i, K)
        kind = (r + phase) % 6
        regular = rep(g, aff[i % MULTIPLES], lam_of(rng, i))
        inf = zero if i % 2 == 0 else garbage(g, rng)
        if kind == 0: p = regular
        elif kind == 1: p = inf
        elif kind == 2: p = inf if pos == 0 else regular
        elif kind == 3: p = inf if pos == K // 2 else regular
        elif kind == 4: p = inf if pos == K - 1 else regular
        else: p = rep(g, aff[r % MULTIPLES], 0x1234567 + r)
        pts.append(p)
    return pts


def pairs(g, n, seed):
    """n pairs (a, b), by i mod 6: the same point in two representations; P and -P; P and 2P; infinity and infinity with different
    garbage coordinates; infinity and P; P and infinity"""
    rng = np.random.default_rng(seed)
    aff = affine(g)
    o = OPS[g]
    a, b = [], []
    for i in range(n):
        j = i % (MULTIPLES // 2)                      # 2 (j + 1) - 1 < MULTIPLES
        P = rep(g, aff[j], lam_of(rng, i))
        kind = i % 6
        if kind == 0: pa, pb = P, rep(g, aff[j], lam_of(rng, i + 1))
        elif kind == 1: pa, pb = P, M.g_neg(o, rep(g, aff[j], lam_of(rng, i + 2)))
        elif kind == 2: pa, pb = P, rep(g, aff[2 * (j + 1) - 1], lam_of(rng, i + 1))
        elif kind == 3: pa, pb = garbage(g, rng), (garbage(g, rng) if i % 12 == 3 else M.g_zero(o))
        elif kind == 4: pa, pb = garbage(g, rng), P
        else: pa, pb = P, M.g_zero(o)
        a.append(pa); b.append(pb)
    return a, b
