"""TEST INFRASTRUCTURE - the integer model, the known answers and the inputs of the Poseidon tests (tests/test_poseidon_constants.py,
tests/test_hostsim_poseidon.py and tests/test_poseidon_abi.py on the CPU, tests/test_gpu_poseidon.py and tests/test_gpu_merkle.py on the GPU).

The model is written independently of bn_amd/poseidon.py: plain Python integers, its own Grain LFSR (an 80-bit integer shifted to the left, where
the package keeps a list of bits), its own round loop (three explicit phases).  The expected bytes of a value are tests/fr_cases.py rows():
the reference's Montgomery image, unique because every result is canonical."""
import functools

import numpy as np

import fr_cases as FC

R = FC.R
FULL = 8
PARTIAL = {2: 56, 3: 57, 4: 56, 5: 60}
_MASK80 = (1 << 80) - 1


def _grain(t):
    """generator of the FILTERED stream bits of the Grain LFSR for width t.  The state is an integer whose bit 79 is b[0], the oldest bit."""
    state = 0
    for value, width in ((1, 2), (0, 4), (254, 12), (t, 12), (FULL, 10), (PARTIAL[t], 10), ((1 << 30) - 1, 30)):
        state = state << width | value
    assert state >> 78 == 1 and state.bit_length() == 79

    def clock():
        nonlocal state
        tap = lambda i: (state >> (79 - i)) & 1
        new = tap(62) ^ tap(51) ^ tap(38) ^ tap(23) ^ tap(13) ^ tap(0)
        state = (state << 1 | new) & _MASK80
        return new
    for _ in range(160):
        clock()
    while True:
        first, second = clock(), clock()
        if first:
            yield second


def _draw(stream):
    v = 0
    for _ in range(254):
        v = 2 * v + next(stream)
    return v


@functools.lru_cache(maxsize=None)
def constants(t):
    """(C, M, xs, ys): round constants, the matrix as a list of rows, and the two halves of the matrix draw"""
    stream = _grain(t)
    C = []
    while len(C) < (FULL + PARTIAL[t]) * t:
        v = _draw(stream)
        if v < R:
            C.append(v)
    xs = [_draw(stream) % R for _ in range(t)]
    ys = [_draw(stream) % R for _ in range(t)]
    M = [[pow((x + y) % R, R - 2, R) for y in ys] for x in xs]
    return C, M, xs, ys


def permute(state):
    t = len(state)
    C, M, _, _ = constants(t)
    s = list(state)
    rnd = 0

    def finish(s):
        return [sum(m * x for m, x in zip(row, s)) % R for row in M]
    for _ in range(FULL // 2):
        s = finish([(x + C[rnd * t + i]) ** 5 % R for i, x in enumerate(s)]); rnd += 1
    for _ in range(PARTIAL[t]):
        s = [(x + C[rnd * t + i]) % R for i, x in enumerate(s)]
        s[0] = s[0] ** 5 % R
        s = finish(s); rnd += 1
    for _ in range(FULL // 2):
        s = finish([(x + C[rnd * t + i]) ** 5 % R for i, x in enumerate(s)]); rnd += 1
    assert rnd * t == len(C)
    return s


def hash_(inputs):
    return permute([0] + list(inputs))[0]


def tree(leaves):
    """the n - 1 inner nodes of the binary tree over n = 2^k leaves, level by level, the root last; [] for one leaf"""
    assert len(leaves) & (len(leaves) - 1) == 0 and leaves
    nodes, level = [], list(leaves)
    while len(level) > 1:
        level = [hash_(level[i:i + 2]) for i in range(0, len(level), 2)]
        nodes += level
    return nodes


def path(leaves, nodes, i):
    """the siblings from the leaf level up"""
    out, level, off, n = [], list(leaves), 0, len(leaves)
    while n > 1:
        out.append(level[i ^ 1])
        level = nodes[off:off + n // 2]; off += n // 2; n //= 2; i >>= 1
    return out


# ---- the known answers of the issue that introduced the family (the t = 2, 3, 5 hashes are circomlib's published vectors)
KNOWN_HASH = {
    (1,): 18586133768512220936620570745912940619677854269274689475585506675881198879027,
    (1, 2): 7853200120776062878684798364095072458815029376092732009249414926327459813530,
    (1, 2, 3): 6542985608222806190361240322586112750744169038454362455181422643027100751666,
    (1, 2, 3, 4): 18821383157269793795438455681495246036402687001665670618754263018637548127333,
    (0, 0): 14744269619966411208579211824598458697587494354926760081771325075741142829156,
    (R - 1, R - 1): 20092309280547939997162506796691455192771288143174894022739895715370814071035,
}
KNOWN_T3 = {
    "C0": 0x0ee9a592ba9a9518d05986d656f40c2114c4993c11bb29938d21d47304cd8e6e,
    "C194": 0x1da55cc900f0d21f4a3e694391918a1b3c23b2ac773c6b3ef88e2e4228325161,
    "M00": 0x109b7f411ba0e4c9b2b70caf5c36a7b194be7c11ad24378bfedb68592ba8118b,
    "M22": 0x19a3fc0a56702bf417ba7fee3802593fa644470307043f7773279cd71d25d5e0,
}
KNOWN_PERMUTE_012_1 = 0x0fca49b798923ab0239de1c9e7a4a9a2210312b6a2f616d18b5a87f9b628ae29
KNOWN_ROOT_8 = 11780650233517635876913804110234352847867393797952240856403268682492028497284           # leaves 0, 1, .. 7
# the last round constant of the other widths: (index, leading hex digits, trailing hex digits) of the 64-digit value
KNOWN_LAST = {2: (127, "269e4b5b", "ff8378f0"), 4: (255, "163ec732", "6a4486d5"), 5: (339, "29eb1de4", "1f63e572")}

# ---- inputs
EDGE = [0, 1, R - 1, FC.MONT % R]


def values(n, seed):
    rng = np.random.default_rng(seed)
    return [FC.rand(rng) for _ in range(n)]


def states(t, n, seed):
    """n states of width t: every edge value in every position (the others random), the all-edge states, then random states"""
    rng = np.random.default_rng(seed)
    out = [[e] * t for e in EDGE]
    for pos in range(t):
        for e in EDGE:
            s = [FC.rand(rng) for _ in range(t)]
            s[pos] = e
            out.append(s)
    while len(out) < n:
        out.append([FC.rand(rng) for _ in range(t)])
    return out[:n]


def hash_inputs(arity, n, seed):
    """n input rows of `arity` values: the known-answer input 1 .. arity first, then the edge cases as in states(), then random rows"""
    return ([list(range(1, arity + 1))] + states(arity, max(n - 1, 0), seed))[:n]


def rows(vals):
    """a list of states (or a flat list) -> (n, 4) uint64 Montgomery images, row-major"""
    flat = [v for s in vals for v in s] if vals and isinstance(vals[0], (list, tuple)) else list(vals)
    return FC.rows(flat)
