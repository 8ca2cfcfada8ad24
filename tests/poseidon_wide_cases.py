"""TEST INFRASTRUCTURE - the integer model, the known answers and the inputs of the wide Poseidon tests (tests/test_poseidon_wide_model.py,
tests/test_hostsim_poseidon_wide.py and tests/test_poseidon_wide_abi.py on the CPU, tests/test_gpu_poseidon_wide.py on the GPU).

The model is written independently of bn_amd/poseidon.py and imports nothing of the package: plain Python integers, its own Grain LFSR (a
bytearray used as a ring, where the package keeps a list it pops and tests/poseidon_cases.py an integer it shifts), its own round loop with
the matrix product written as column sums.  The expected bytes of a value are tests/fr_cases.py rows(): the Montgomery image, unique because
every result is canonical."""
import functools

import numpy as np

import fr_cases as FC

R = FC.R
FULL = 8
# R_P of t = 2 .. 17: circomlib's list
PARTIAL = dict(zip(range(2, 18), (56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68)))
INPUTS_MAX = 16
TAPS = (62, 51, 38, 23, 13, 0)


class _Ring:
    """the 80-bit LFSR of the Poseidon paper: ring[(head + i) % 80] is bit i"""

    def __init__(self, t):
        bits = ""
        for value, width in ((1, 2), (0, 4), (254, 12), (t, 12), (FULL, 10), (PARTIAL[t], 10), (2 ** 30 - 1, 30)):
            bits += format(value, "0%db" % width)
        assert len(bits) == 80
        self.ring = bytearray(int(c) for c in bits)
        self.head = 0
        for _ in range(160):
            self.clock()

    def clock(self):
        new = 0
        for tap in TAPS:
            new ^= self.ring[(self.head + tap) % 80]
        self.ring[self.head] = new
        self.head = (self.head + 1) % 80
        return new

    def filtered(self):
        while True:
            if self.clock():
                return self.clock()
            self.clock()

    def draw(self):
        return int("".join(str(self.filtered()) for _ in range(254)), 2)


@functools.lru_cache(maxsize=None)
def constants(t):
    """(C, M, xs, ys): round constants, the matrix as a list of rows, and the two halves of the matrix draw"""
    lfsr = _Ring(t)
    C = []
    while len(C) < (FULL + PARTIAL[t]) * t:
        v = lfsr.draw()
        if v < R:
            C.append(v)
    xs = [lfsr.draw() % R for _ in range(t)]
    ys = [lfsr.draw() % R for _ in range(t)]
    M = [[pow((x + y) % R, R - 2, R) for y in ys] for x in xs]
    return C, M, xs, ys


def permute(state):
    t = len(state)
    C, M, _, _ = constants(t)
    s = [x % R for x in state]
    first_partial, first_back = FULL // 2, FULL // 2 + PARTIAL[t]
    for rnd in range(FULL + PARTIAL[t]):
        s = [(x + C[rnd * t + i]) % R for i, x in enumerate(s)]
        if first_partial <= rnd < first_back:
            s[0] = pow(s[0], 5, R)
        else:
            s = [pow(x, 5, R) for x in s]
        new = [0] * t
        for j, x in enumerate(s):                    # column by column
            for i in range(t):
                new[i] += M[i][j] * x
        s = [v % R for v in new]
    return s


def hash_ex(inputs, init=0, n_outs=1):
    return permute([init] + list(inputs))[:n_outs]


def blocks(length, rate):
    return max(1, -(-length // rate))


def hash_chain(values, rate=16):
    """c = len; per block of `rate` values (zero padded; an empty record is one block of zeros) c = permute([c, block..])[0]"""
    values = list(values)
    c = len(values)
    for b in range(blocks(len(values), rate)):
        block = values[b * rate:(b + 1) * rate]
        c = permute([c] + block + [0] * (rate - len(block)))[0]
    return c


# ---- permute([0, 1, .., n])[0].  n = 1, 2: the answers the repository pinned before this family (tests/poseidon_cases.py KNOWN_HASH); n = 6 and
# n = 16: the values circomlibjs publishes in its own tests for [1..6] and [1..16] - the external anchor of the R_P list and of the wide
# matrix; EVERY OTHER ROW is this derivation's own output: a regression anchor, not an external vector.
KNOWN = {
    1: 18586133768512220936620570745912940619677854269274689475585506675881198879027,
    2: 7853200120776062878684798364095072458815029376092732009249414926327459813530,
    3: 6542985608222806190361240322586112750744169038454362455181422643027100751666,
    4: 18821383157269793795438455681495246036402687001665670618754263018637548127333,
    5: 6183221330272524995739186171720101788151706631170188140075976616310159254464,
    6: 20400040500897583745843009878988256314335038853985262692600694741116813247201,
    7: 12748163991115452309045839028154629052133952896122405799815156419278439301912,
    8: 18604317144381847857886385684060986177838410221561136253933256952257712543953,
    9: 13589767895268936107593642967621470491511464502761040466226072462545218539640,
    10: 3657500514307717306974218405144578736633140001277925127187636780142269815841,
    11: 3572015662710076994097916907865950486270383304442561406230608893458731714472,
    12: 2501997477381648492950318384533644783248002172679259592360114615426357826485,
    13: 7041832639553862712666971417715061873827921493498355005117622707743491651590,
    14: 8354478399926161176778659061636406690034081872658507739535256090879947077494,
    15: 4203130618016961831408770638653325366880478848856764494148034853759773445968,
    16: 9989051620750914585850546081941653841776809718687451684622678807385399211877,
}
EXTERNAL = (6, 16)          # circomlibjs
PINNED_BEFORE = (1, 2)

# ---- inputs
EDGE = [0, 1, R - 1]
# widths on both sides of every fr_dot chunk seam (5 | 6, 10 | 11, 15 | 16) and of every elements-per-lane seam of G = 4, 8, 16
SEAM_WIDTHS = (2, 5, 6, 7, 10, 11, 15, 16, 17)


def chain_lengths(rate):
    """L = 0, 1, rate - 1, rate, rate + 1, 3 rate + 2 (without repeats, in this order)"""
    out = []
    for L in (0, 1, rate - 1, rate, rate + 1, 3 * rate + 2):
        if L not in out:
            out.append(L)
    return out


def values(n, seed):
    rng = np.random.default_rng(seed)
    return [FC.rand(rng) for _ in range(n)]


def ex_rows(n_inputs, n, seed, edges=False):
    """n input rows: the known-answer row 1 .. n_inputs first, the all-edge rows, (edges=True: every edge value in every position of an otherwise
    random row,) then random rows"""
    rng = np.random.default_rng(seed)
    out = [list(range(1, n_inputs + 1))] + [[e] * n_inputs for e in EDGE]
    if edges:
        for pos in range(n_inputs):
            for e in EDGE:
                row = [FC.rand(rng) for _ in range(n_inputs)]
                row[pos] = e
                out.append(row)
    while len(out) < n:
        out.append([FC.rand(rng) for _ in range(n_inputs)])
    return out[:n]


def records(lengths, seed):
    """records of the given lengths -> (list of records, flat list, offsets)"""
    rng = np.random.default_rng(seed)
    recs = [[FC.rand(rng) for _ in range(L)] for L in lengths]
    flat = [v for r in recs for v in r]
    return recs, flat, np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def mixed_lengths(rate, count, seed):
    """`count` lengths drawn from 0 .. 3 rate + 2 with every length of chain_lengths(rate) among them, shuffled: neighbours run different numbers of blocks"""
    rng = np.random.default_rng(seed)
    base = chain_lengths(rate)
    out = base + [int(rng.integers(0, 3 * rate + 3)) for _ in range(max(count - len(base), 0))]
    out = out[:count] if count >= len(base) else base[:count]
    rng.shuffle(out)
    return [int(x) for x in out]


def rows(vals):
    """a list of rows (or a flat list) -> (n, 4) uint64 Montgomery images, row-major"""
    flat = [v for s in vals for v in s] if vals and isinstance(vals[0], (list, tuple)) else list(vals)
    return FC.rows(flat) if flat else np.zeros((0, 4), np.uint64)
