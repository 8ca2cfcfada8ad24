"""The plan of bn254_g{1,2}_ntt_batch without a device (bn_amd/csrc/host_plan.hpp bn_group_ntt_run / bn_group_ntt_group, compiled with g++
into tests/hostsim/hostsim_group_ntt.cpp): groups of transforms, the stages and the two passes, the buffer every step reads and writes,
the sub-launches - and the index arithmetic of a butterfly (group_ntt_ops.hpp group_ntt_index), replayed here in Python: composed to whole
transforms up to 2^6, against the closed form of the Stockham stage at 2^12, 2^13, 2^14 and 2^22.  From 2^13 on the twiddles (ntt_ops.hpp
ntt_root_power) and the factors of the passes (ntt_shift_power) take both halves of their table pairs; what the stage and pass bodies get
from them is checked against Python integers through hsg_twiddle and hsg_scale_factor."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import fr_cases as FC
import group_ntt_cases as GC

IN, OUT, WS = 0, 1, 2
SCALE, STAGE, NORMALIZE = 0, 1, 2
BIG = 1 << 22


@pytest.fixture(scope="module")
def sim():
    return GC.hostsim()


def _plan(sim, log_n, count, cap, chain_cap=BIG, shift=False, inverse=False):
    head = np.zeros(6, np.uint64)
    steps = np.zeros((4096, 8), np.uint64)
    k = sim.hsg_plan(C.c_uint32(log_n), C.c_size_t(count), C.c_size_t(cap), C.c_size_t(chain_cap), C.c_int(shift), C.c_int(inverse),
                     head.ctypes.data_as(C.c_void_p), steps.ctypes.data_as(C.c_void_p), C.c_size_t(len(steps)))
    assert k <= len(steps)
    keys = ("tr0", "kind", "stage", "src", "dst", "chain", "lo", "n")
    return dict(zip(("stages", "pre", "post", "per_group", "most", "ws_bufs"), (int(x) for x in head))), [dict(zip(keys, (int(x) for x in r))) for r in steps[:k]]


def _index(sim, log_n, stage, g):
    out = (C.c_uint32 * 5)()
    sim.hsg_index(C.c_uint32(log_n), C.c_uint32(stage), C.c_uint32(g), out)
    return tuple(out)


@pytest.mark.parametrize("log_n", range(1, 7))
def test_every_stage_reads_and_writes_every_record_once_with_the_twiddle_of_the_definition(sim, log_n):
    """three transforms back to back: the butterflies of a stage read every record exactly once and write every record exactly once, and the
    stages compose to the transform (checked on integers with the twiddle exponents the kernel uses)"""
    n, count = 1 << log_n, 3
    R = GC.R
    w24 = GC.NC.root(24)
    rng = np.random.default_rng(log_n)
    x = [int(v) for v in rng.integers(1, 1 << 62, count * n)]
    cur = list(x)
    for stage in range(log_n):
        reads, writes, nxt = [], [], [None] * (count * n)
        for g in range(count * n // 2):
            a, b, o0, o1, e = _index(sim, log_n, stage, g)
            assert a // n == b // n == o0 // n == o1 // n == g // (n // 2)                     # a butterfly stays inside its transform
            reads += [a, b]; writes += [o0, o1]
            if stage == 0:
                assert e == 0                                                                   # the stage that runs no chain
            t = cur[b] * pow(w24, e, R) % R
            nxt[o0], nxt[o1] = (cur[a] + t) % R, (cur[a] - t) % R
        assert sorted(reads) == sorted(writes) == list(range(count * n))
        cur = nxt
    for t in range(count):
        assert cur[t * n:(t + 1) * n] == GC.NC.ntt(x[t * n:(t + 1) * n])


TBL_LOG = 12                                                # ntt_ops.hpp NTT_TBL_LOG: a power of w_24 is wtbl[e & 4095] * wtbl[4096 + (e >> 12)]
SAMPLED_LOGS = (12, 14, 22)
COUNT = 3


def _closed_form(log_n, stage, g):
    """(a, b, o0, o1, e, k r') of butterfly g of a stage over transforms laid back to back, from the definition of the Stockham stage"""
    n = 1 << log_n
    rp = n >> (stage + 1)
    tr, bf = divmod(g, n // 2)
    k, rho = divmod(bf, rp)
    a = tr * n + rho + 2 * rp * k
    return a, a + rp, tr * n + bf, tr * n + bf + n // 2, (k * rp) << (24 - log_n), k * rp


def _sample(log_n, seed, count=COUNT):
    """butterflies of `count` transforms: the first and the last of every transform - both sides of every boundary - and 64 random ones"""
    half = 1 << (log_n - 1)
    rng = np.random.default_rng(seed)
    ends = [t * half + d for t in range(count) for d in (0, 1, half - 2, half - 1) if 0 <= d < half]
    return sorted(set(ends) | {int(v) for v in rng.integers(0, count * half, 64)})


def _low_part_stages(log_n):
    """the stages whose twiddles w_(2^(stage+1))^k have an order above 2^12, so that odd k carry a low part; none below log_n = 13"""
    return range(TBL_LOG, log_n)


@functools.lru_cache(maxsize=None)
def _root_power(log_n, x):
    return pow(GC.NC.root(log_n), x, GC.R)


def _check_index(sim, log_n, stage, gs):
    """hsg_index against the closed form for the butterflies gs; returns the exponents"""
    es = []
    for g in gs:
        *want, kr = _closed_form(log_n, stage, g)
        assert _index(sim, log_n, stage, g) == tuple(want), (log_n, stage, g)
        e = want[4]
        assert e < 1 << 24 and _root_power(24, e) == _root_power(log_n, kr), (log_n, stage, g)
        es.append(e)
    return es


def test_every_butterfly_of_three_transforms_of_2_to_the_13_against_the_closed_form(sim):
    """2^13 is the smallest size at which an exponent of w_24 has a low part (stage 12, odd k): records, outputs and exponent of every
    butterfly of every stage, and every stage reads and writes every record once"""
    log_n, n = 13, 1 << 13
    every = np.arange(COUNT * n)
    for stage in range(log_n):
        out = np.empty((COUNT * n // 2, 5), np.uint32)
        for g in range(len(out)):
            sim.hsg_index(C.c_uint32(log_n), C.c_uint32(stage), C.c_uint32(g), out[g].ctypes.data_as(C.c_void_p))
        g = np.arange(len(out), dtype=np.int64)
        rp = n >> (stage + 1)
        tr, bf = g // (n // 2), g % (n // 2)
        k, rho = bf // rp, bf % rp
        a = tr * n + rho + 2 * rp * k
        want = np.stack([a, a + rp, tr * n + bf, tr * n + bf + n // 2, (k * rp) << (24 - log_n)], axis=1)
        assert np.array_equal(out.astype(np.int64), want), (stage, np.nonzero((out != want).any(axis=1))[0][:8])
        assert np.array_equal(np.sort(out[:, :2].ravel()), every) and np.array_equal(np.sort(out[:, 2:4].ravel()), every)
        for kr in np.unique(k * rp):
            assert _root_power(24, int(kr) << (24 - log_n)) == _root_power(log_n, int(kr)), (stage, kr)
        low = (out[:, 4] & ((1 << TBL_LOG) - 1)) != 0
        assert np.array_equal(low, (k % 2 == 1) if stage in _low_part_stages(log_n) else np.zeros(len(out), bool)), stage


@pytest.mark.parametrize("log_n", SAMPLED_LOGS)
def test_sampled_butterflies_of_every_stage_against_the_closed_form(sim, log_n):
    """the first and last butterfly of three transforms, both sides of their boundaries and 64 random ones.  A twiddle of stage i is a root
    of order 2^(i+1), so its exponent of w_24 has low 12 bits exactly from stage 12 on, for odd k: the sample must hold such a butterfly in
    every one of those stages (and cannot in any other)"""
    for stage in range(log_n):
        es = _check_index(sim, log_n, stage, _sample(log_n, 1000 * log_n + stage))
        assert any(e & ((1 << TBL_LOG) - 1) for e in es) == (stage in _low_part_stages(log_n)), (log_n, stage)


def _words(fn, *args):
    out = (C.c_uint32 * 8)()
    fn(*args, out)
    return sum(int(w) << (32 * i) for i, w in enumerate(out))


def _mont(v):
    return v % GC.R * FC.MONT % GC.R


@pytest.mark.parametrize("log_n", (13,) + SAMPLED_LOGS)
def test_the_twiddle_of_the_stage_body_is_the_power_of_the_root_of_the_transform(sim, log_n):
    """ntt_root_power over the table pair, as group_ntt_stage_body calls it: w_n^(k r') forward and w_n^(-k r') inverse, the latter through
    (0 - e) & (2^24 - 1), which borrows through both halves of the pair whenever e has a low part"""
    for stage in range(1, log_n):                                                               # stage 0 runs no chain
        gs = _sample(log_n, 2000 * log_n + stage)
        if log_n == 13 and stage == 12:
            gs = sorted(set(gs) | set(range(0, COUNT << 12, 7)))                                # and every seventh butterfly of the stage with low parts
        lows = 0
        for g in gs:
            e, kr = _closed_form(log_n, stage, g)[4:]
            lows += (e & ((1 << TBL_LOG) - 1)) != 0
            for inverse in (0, 1):
                got = _words(sim.hsg_twiddle, C.c_uint32(log_n), C.c_uint32(stage), C.c_uint32(g), C.c_int(inverse))
                want = _root_power(log_n, ((1 << log_n) - kr) % (1 << log_n) if inverse else kr)
                assert got == _mont(want), (log_n, stage, g, inverse)
        assert (lows > 0) == (stage in _low_part_stages(log_n)), (log_n, stage)


@pytest.mark.parametrize("log_n", (13,) + SAMPLED_LOGS)
def test_the_factor_of_the_scale_body_is_the_power_of_the_shift(sim, log_n):
    """ntt_shift_power over the table pair, as group_ntt_scale_body calls it with j mod n: s^j before a forward transform, n^-1 s^-j after
    an inverse one, the constant n^-1 after an inverse one without a shift; above j = 4095 the high half of the pair takes part"""
    n, R = 1 << log_n, GC.R
    rng = np.random.default_rng(3000 + log_n)
    js = [0, 1, 4095, 4096, 4097, n - 1] + [int(v) for v in rng.integers(0, n, 32)]
    js += [j + t * n for t in (1, COUNT - 1) for j in (0, 4097 % n, n - 1)]                     # points of the transforms behind the first
    ni = pow(n, -1, R)
    for j in js:
        assert _words(sim.hsg_scale_factor, C.c_uint32(log_n), C.c_uint32(j), C.c_int(1), None) == _mont(ni), (log_n, j)
    for shift in (5, GC.NC.SHIFT_RANDOM):
        s = FC.rows([shift])[0]
        si = pow(shift, -1, R)
        for inverse in (0, 1):
            for j in js:
                got = _words(sim.hsg_scale_factor, C.c_uint32(log_n), C.c_uint32(j), C.c_int(inverse), s.ctypes.data_as(C.c_void_p))
                want = ni * pow(si, j % n, R) % R if inverse else pow(shift, j % n, R)
                assert got == _mont(want), (log_n, shift, inverse, j)


CASES = list(itertools.product(range(0, 6), (1, 3), (False, True), (False, True)))


@pytest.mark.parametrize("log_n, count, shift, inverse", CASES)
def test_the_buffers_of_a_call_at_a_launch_cap_of_four(sim, log_n, count, shift, inverse):
    """in place and out of place alike (the plan never writes IN and writes OUT only after IN has been read completely): every group ends
    with the normalisation into OUT, for odd and even numbers of stages"""
    n, cap = 1 << log_n, 4
    head, steps = _plan(sim, log_n, count, cap, BIG, shift, inverse)
    assert head["stages"] == log_n and head["per_group"] == max(1, cap >> log_n)
    assert head["most"] == min(count, head["per_group"]) * n and head["ws_bufs"] == (1 if log_n else 0)
    assert head["pre"] == (log_n > 0 and shift and not inverse) and head["post"] == (log_n > 0 and inverse)
    groups = [list(g) for _, g in itertools.groupby(steps, key=lambda s: s["tr0"])]
    assert [g[0]["tr0"] for g in groups] == list(range(0, count, head["per_group"]))
    for grp in groups:
        cnt = min(head["per_group"], count - grp[0]["tr0"])
        points = cnt * n
        assert points <= head["most"] or not head["ws_bufs"]
        # the steps of the group in order: consecutive sub-launches of one step share kind, stage and buffers
        runs = [list(r) for _, r in itertools.groupby(grp, key=lambda s: (s["kind"], s["stage"], s["src"], s["dst"]))]
        want = ([(SCALE, 0)] if head["pre"] else []) + [(STAGE, i) for i in range(log_n)] + ([(SCALE, 0)] if head["post"] else []) + [(NORMALIZE, 0)]
        assert [(r[0]["kind"], r[0]["stage"]) for r in runs] == want
        cur, in_read_completely = IN, False
        for r in runs:
            s = r[0]
            units = points // 2 if s["kind"] == STAGE else points
            # the sub-launches tile the step: every butterfly / point exactly once, none above the cap
            assert [x["lo"] for x in r] == list(range(0, units, cap))[:len(r)] and sum(x["n"] for x in r) == units
            assert all(0 < x["n"] <= cap for x in r)
            assert s["src"] == cur and s["dst"] != IN
            assert s["chain"] == (1 if s["kind"] == SCALE or (s["kind"] == STAGE and s["stage"] > 0) else 0)
            if s["kind"] == STAGE:
                assert s["dst"] != s["src"]                                                    # a stage is never in place
                assert not (s["src"] == IN and s["dst"] == OUT)                                # OUT may be IN
            if s["dst"] == OUT and not in_read_completely:
                assert s["src"] == IN and s["kind"] != STAGE                                   # lane-local: point j to point j
            if s["src"] == IN:
                in_read_completely = True
            cur = s["dst"]
        assert cur == OUT and runs[-1][0]["kind"] == NORMALIZE


def test_groups_at_the_shipped_cap_and_chain_launches_below_it(sim):
    head, steps = _plan(sim, 22, 2, BIG, 1 << 20)
    assert head["per_group"] == 1 and head["most"] == 1 << 22
    stage0 = [s for s in steps if s["tr0"] == 0 and s["kind"] == STAGE and s["stage"] == 0]
    stage1 = [s for s in steps if s["tr0"] == 0 and s["kind"] == STAGE and s["stage"] == 1]
    assert [(s["lo"], s["n"]) for s in stage0] == [(0, 1 << 21)]                               # no chain: one launch of n / 2 butterflies
    assert [(s["lo"], s["n"]) for s in stage1] == [(0, 1 << 20), (1 << 20, 1 << 20)]           # chains: at most 2^20 window tables
    head, steps = _plan(sim, 3, 1000, BIG)
    assert head["per_group"] == 1 << 19 and head["most"] == 8000 and len({s["tr0"] for s in steps}) == 1
    head, steps = _plan(sim, 2, 5, 8, 3, shift=True)                                           # two transforms per group, chain launches of 3
    assert head["per_group"] == 2 and [s["tr0"] for s in steps if s["kind"] == NORMALIZE] == [0, 2, 4]
    first = [s for s in steps if s["tr0"] == 0]
    assert [(s["kind"], s["stage"], s["lo"], s["n"]) for s in first] == [(SCALE, 0, 0, 3), (SCALE, 0, 3, 3), (SCALE, 0, 6, 2), (STAGE, 0, 0, 4), (STAGE, 1, 0, 3), (STAGE, 1, 3, 1), (NORMALIZE, 0, 0, 8)]
    assert [(s["src"], s["dst"]) for s in first] == [(IN, OUT)] * 3 + [(OUT, WS), (WS, OUT), (WS, OUT), (OUT, OUT)]


def test_the_argument_check_and_its_order(sim):
    p = C.c_void_p(0x1000)
    zero = (C.c_uint64 * 4)(0, 0, 0, 0)
    five = (C.c_uint64 * 4)(5, 0, 0, 0)
    ok = lambda *a: sim.hsg_check(a[0], a[1], C.c_int(a[2]), C.c_size_t(a[3]), a[4])
    assert ok(p, p, 0, 1, None) == 0 and ok(p, p, 22, 1 << 18, five) == 0
    for bad in ((p, p, -1, 1, None), (p, p, 23, 1, None), (None, p, 3, 1, None), (p, None, 3, 1, None), (p, p, 22, (1 << 18) + 1, None), (p, p, 0, (1 << 40) + 1, None),
                (p, p, 3, 1, zero)):
        assert ok(*bad) == -2, bad
