"""TEST INFRASTRUCTURE - inputs and expected values of the segmented scans over Fr (bn254_fr_scan_batch: tests/test_host_plan_scan.py and
tests/test_hostsim_scan.py on the CPU, tests/test_gpu_scan.py and tests/test_gpu_kzg.py on the GPU).  The model is Python integers
(tests/fr_cases.py): every product and sum is canonical, so the expected bytes are those of the integer recurrence whichever way a plan
cuts a segment."""
import itertools

import numpy as np

import fr_cases as FC

R = FC.R
REVERSE, EXCLUSIVE, A_PER_SEGMENT = 1, 2, 4
FLAG_SETS = [dict(reverse=r, exclusive=e, a_per_segment=s) for r, e, s in itertools.product((False, True), repeat=3)]


def flag_bits(reverse=False, exclusive=False, a_per_segment=False):
    return (REVERSE if reverse else 0) | (EXCLUSIVE if exclusive else 0) | (A_PER_SEGMENT if a_per_segment else 0)


def lengths(P, F):
    """segment lengths around every seam of a plan with pieces of P terms and levels of fan F: empty, one and two terms, around one piece, two
    pieces, exactly one down lane, one more (the first up level, a second down level), and F * F pieces and one term (a second up level,
    a third down level)"""
    return [0, 1, 2, P - 1, P, P + 1, 2 * P, F * P, F * P + 1, F * F * P + 1]


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def values(n, seed, kind="mixed"):
    """n integers.  mixed: seeded random ones with the edge values sprinkled in at co-prime strides - zero (a zero `a` resets the recurrence and
    makes the map of its piece constant), r - 1, one, and the other FC.SPECIAL values; ones; minus_ones (r - 1 everywhere)"""
    if kind == "ones":
        return [1] * n
    if kind == "minus_ones":
        return [R - 1] * n
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        v = FC.rand(rng)
        if t % 37 == 5 + seed % 3: v = 0
        elif t % 41 == 7: v = R - 1
        elif t % 13 == 3: v = 1
        elif t % 29 == 11: v = FC.SPECIAL[(t // 29) % len(FC.SPECIAL)]
        out.append(v)
    return out


def model(a, b, offsets, init=None, reverse=False, exclusive=False, a_per_segment=False):
    """the n outputs as integers: out[t] = a[t] * prev + b[t] over every segment in order (reverse: from its last term), prev from init[j] (None:
    zero with b, one without); exclusive: out[t] = prev.  a or b None: all ones / all zeros."""
    o = [int(v) for v in offsets]
    out = [None] * o[-1]
    for j in range(len(o) - 1):
        cur = init[j] if init is not None else (0 if b is not None else 1)
        ts = range(o[j], o[j + 1])
        for t in (reversed(ts) if reverse else ts):
            x = 1 if a is None else (a[j] if a_per_segment else a[t])
            y = 0 if b is None else b[t]
            nxt = (x * cur + y) % R
            out[t] = cur if exclusive else nxt
            cur = nxt
    return out


def up_levels(L, P, F):
    """up levels of a segment of L terms: how often k -> ceil(k / F) is taken while k > F, from k = ceil(L / P)"""
    k, u = -(-L // P), 0
    while k > F:
        k = -(-k // F); u += 1
    return u


def plan_levels(L, P, F):
    """levels a segment of L terms takes part in: none when empty, the apply level alone for at most P terms, else reduce, u up, u + 1 down, apply"""
    return 0 if L == 0 else 1 if L <= P else 2 * up_levels(L, P, F) + 3


def launches(lens, P, F, step):
    """sub-launches per kind (reduce, up, down, apply) of a call over segments of these lengths, `step` lanes per sub-launch at most"""
    parts = lambda lanes: -(-lanes // step)
    pieces = sum(-(-L // P) for L in lens)
    long = [-(-L // P) for L in lens if L > P]
    if not long:
        return (0, 0, 0, parts(pieces))
    ups, downs = [], []
    for k in long:
        tree = [k]
        while tree[-1] > F:
            tree.append(-(-tree[-1] // F))
        for u, lanes in enumerate(tree[1:]):
            ups += [0] * (u + 1 - len(ups)); ups[u] += lanes
        for d, lanes in enumerate([1] + tree[:0:-1]):
            downs += [0] * (d + 1 - len(downs)); downs[d] += lanes
    return (parts(pieces), sum(parts(x) for x in ups), sum(parts(x) for x in downs), parts(pieces))
