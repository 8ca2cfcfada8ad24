"""TEST INFRASTRUCTURE - inputs and expected values of the Fr tests (tests/test_hostsim_fr.py on the CPU, tests/test_gpu_fr.py on the GPU).
The model is Python integers: the expected bytes of a value v are the four little-endian u64 limbs of v * 2^256 mod r, the reference's
memory image (fields/fp.rs:11-22), and they are unique because every result is canonical."""
import numpy as np

_U = 4965661367192848881
R = 36 * _U**4 + 36 * _U**3 + 18 * _U**2 + 6 * _U + 1
MONT = 1 << 256
_M64 = (1 << 64) - 1

# the edge values: 0, 1, 2, r-1, r-2, (r-1)/2, (r+1)/2, 2^253, 2^256 mod r (its Montgomery image's integer is 2^512 mod r), r - (2^256 mod r)
SPECIAL = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 253, MONT % R, R - MONT % R]


def rows(values):
    """integers mod r -> (n, 4) uint64 Montgomery images"""
    out = np.zeros((len(values), 4), np.uint64)
    for i, v in enumerate(values):
        m = v % R * MONT % R
        out[i] = [(m >> (64 * j)) & _M64 for j in range(4)]
    return out


def rand(rng):
    return int.from_bytes(rng.bytes(64), "little") % R


def values(n, seed):
    """n values: the edge values first (as many as fit), then random ones"""
    rng = np.random.default_rng(seed)
    return [SPECIAL[i] if i < len(SPECIAL) else rand(rng) for i in range(n)]


def pairs(n, seed):
    """n operand pairs (a, b).  The first ones, in turn: a + b = r, r - 1 and r + 1 (the sum just below, at and above the modulus), a = b,
    zero on either side, both zero, every edge value against a random one; then random pairs."""
    rng = np.random.default_rng(seed)
    x = rand(rng) % (R - 3) + 2
    head = [(x, R - x), (x, R - 1 - x), (x, R + 1 - x), (x, x), (R - 1, R - 1), (0, x), (x, 0), (0, 0), (1, R - 1), ((R + 1) // 2, (R + 1) // 2), ((R - 1) // 2, (R + 1) // 2)]
    head += [(s, rand(rng)) for s in SPECIAL] + [(rand(rng), s) for s in SPECIAL]
    out = [head[i] if i < len(head) else (rand(rng), rand(rng)) for i in range(n)]
    return [a for a, _ in out], [b for _, b in out]


N_PAIR_HEAD = 11 + 2 * len(SPECIAL)


def inverse_values(n, K, phase, seed):
    """n values in runs of K; run r + phase (mod 6) is: 0 - no zero, edge and random values in turn; 1 - a whole run of zeros; 2 / 3 / 4 - a
    zero at the first / an interior / the last position; 5 - two adjacent zeros (positions K // 2 and K // 2 + 1, the latter may be the
    next run's first for small K)"""
    rng = np.random.default_rng(seed)
    nz = [s for s in SPECIAL if s]
    out = []
    for i in range(n):
        r, pos = divmod(i, K)
        kind = (r + phase) % 6
        v = nz[i % len(nz)] if i % 3 == 0 else rand(rng) % (R - 1) + 1
        if kind == 1: v = 0
        elif kind == 2 and pos == 0: v = 0
        elif kind == 3 and pos == K // 2: v = 0
        elif kind == 4 and pos == K - 1: v = 0
        elif kind == 5 and pos in (K // 2, min(K - 1, K // 2 + 1)): v = 0
        out.append(v)
    return out


def model_inverse(vals):
    """(rows, ok): Option<Fr> with None as Fr::zero() and ok = 0"""
    return rows([pow(v, -1, R) if v else 0 for v in vals]), np.array([1 if v else 0 for v in vals], np.int32)


def pow_cases(n, seed):
    """(bases, exponents): 0^0, 0^1, 0^(r-1), then a in (1, 2, r-1, random) against e in (0, 1, 2, r-1, r-2, exponents whose top windows are
    zero: 3, 2^16 + 1, 2^64 - 1, 2^128 + 5, and 2^253, whose top window is the only non-zero one), then random pairs"""
    rng = np.random.default_rng(seed)
    x = rand(rng) % (R - 3) + 2
    exps = [0, 1, 2, R - 1, R - 2, 3, (1 << 16) + 1, (1 << 64) - 1, (1 << 128) + 5, 1 << 253]
    head = [(0, 0), (0, 1), (0, R - 1), (0, rand(rng))] + [(a, e) for e in exps for a in (x, 1, 2, R - 1)]
    out = [head[i] if i < len(head) else (rand(rng), rand(rng)) for i in range(n)]
    return [a for a, _ in out], [e for _, e in out]


def interpret_buffers(n, seed):
    """(n, 64) uint8: all 0x00, all 0xff, then r, r - 1, 2^256 and 2^256 r - 1 as 512-bit big-endian integers, then random bytes"""
    rng = np.random.default_rng(seed)
    head = [0, (1 << 512) - 1, R, R - 1, 1 << 256, (R << 256) - 1]
    ints = [head[i] if i < len(head) else int.from_bytes(rng.bytes(64), "big") for i in range(n)]
    return np.frombuffer(b"".join(v.to_bytes(64, "big") for v in ints), np.uint8).reshape(n, 64).copy(), ints
