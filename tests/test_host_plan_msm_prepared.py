"""The host arithmetic of the multi-scalar multiplication against prepared bases (bn_amd/csrc/host_plan.hpp: msm_prepared_plan,
msm_prepared_tail_scalars, bn_msm_prepared_window_bits and the two argument checks), compiled with g++ and replayed on the CPU."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import bn_model as M
import hostsim_msm_prepared_lib as L

R = M.R_ORD
SIZES = (0, 1, 16, 17, 1 << 20)
WIDTHS = (3, 8, 13, 16)
BAD_ARG = -2
DUMMY = C.c_void_p(0x1000)


def _from_mont(row):
    v = sum(int(x) << (64 * i) for i, x in enumerate(row))
    return v * pow(1 << 256, -1, R) % R


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_workspace_offsets_and_level_slots(n, c):
    """every offset is 256-byte aligned, the regions lie in order without overlap inside `bytes`, and no level has fewer slots than the
    entries that can reach it: level 0 reads at most W * chunk entries (every digit non-zero), level l + 1 the two slots of every lane
    of level l - taken through msm_level_len, the function the kernels themselves use"""
    lib = L.lib()
    piece = lib.hsp_piece()
    for V in (96, 192):
        chunk = max(1, n)                                              # the host unit plans for max(1, min(n, msm_chunk)) terms
        p = L.plan(c, chunk, V, piece)
        W, K = L.windows(c), 1 << (c - 1)
        assert (p["W"], p["K"], p["G"], p["groups"], p["count"]) == (W, K, min(16, K), K // min(16, K), K // min(16, K))
        assert p["n0max"] == W * chunk
        regions = [(p["o_counts"], K * 4), (p["o_tiles"], 1024 * 4), (p["o_n0"], 4), (p["o_idx"], p["n0max"] * 4), (p["o_keys"], p["n0max"] * 4), (p["o_buckets"], K * V)]
        for slots, o_pts, o_keys in p["levels"]:
            regions += [(o_pts, slots * V), (o_keys, slots * 4)]
        regions.append((p["o_terms"], 2 * p["count"] * V))
        at = 0
        for off, size in regions:
            assert off % 256 == 0 and off >= at, (off, at)
            at = off + size
        assert at <= p["bytes"]
        # the true entry counts: every count from none to all of the W * n digits non-zero goes through the same levels
        for n0 in {0, 1, W * n // 2, W * n}:
            for level, (slots, _, _) in enumerate(p["levels"]):
                N = lib.hsp_level_len(n0, level)
                lanes = (N + piece - 1) // piece
                assert slots >= 2 * lanes, (n0, level)
                assert N <= (p["n0max"] if level == 0 else p["levels"][level - 1][0]), (n0, level)
        last = lib.hsp_level_len(W * n, len(p["levels"]) - 1)
        assert last <= piece                                           # the last planned level is one lane: nothing is left over


@pytest.mark.parametrize("c", range(3, 17))
def test_tail_scalars_are_base_plus_one_and_one(c):
    K = 1 << (c - 1)
    G = min(16, K)
    groups = K // G
    s = L.tail_scalars(c)
    assert s.shape == (2 * groups, 4)
    assert [_from_mont(r) for r in s[:groups]] == [q * G + 1 for q in range(groups)]
    assert [_from_mont(r) for r in s[groups:]] == [1] * groups
    # which is what the reduction's terms need: bucket b weighs b + 1 = (base + 1) + (b - base)
    for q in range(groups):
        for b in range(q * G, (q + 1) * G):
            assert b + 1 == (q * G + 1) * 1 + (b - q * G)


def recorded_width_table():
    """{(group, log2 n): width} of the "# width table" line of profiles/r29_msm_prepared.txt - what tools/time_msm_prepared.py --widths found
    fastest (the smallest median) at every size it swept"""
    text = (pathlib.Path(__file__).resolve().parents[1] / "profiles" / "r29_msm_prepared.txt").read_text()
    line = re.search(r"^# width table[^:]*: (.*)$", text, re.M).group(1)
    table = {(int(g), int(lg)): int(c) for g, lg, c in re.findall(r"G(\d) 2\^(\d+): (\d+)", line)}
    assert set(table) == {(1, 16), (1, 18), (1, 20), (1, 22), (2, 15), (2, 18), (2, 20)}, table
    return table


def test_default_width_is_total_and_is_the_recorded_table():
    """the rule was fixed before the sweep: the default width of a size is the one with the smallest median; a size that was not measured
    takes the width of the nearest measured one.  The function is one function of n for both groups, so the groups must agree where both
    were measured - they do - and it is total on 0 .. 2^26"""
    lib = L.lib()
    table = recorded_width_table()
    for (g, lg), c in table.items():
        assert lib.hsp_window_bits(1 << lg) == c, (g, lg)
    measured = sorted({lg for _, lg in table})
    sizes = sorted(set([0, 1, 2, 3, 1000] + [1 << e for e in range(27)] + [(1 << e) - 1 for e in range(1, 27)] + [(1 << e) + 1 for e in range(26)]))
    assert sizes[-1] == 1 << 26
    for n in sizes:
        c = lib.hsp_window_bits(n)
        assert 3 <= c <= 16
        lg = max(n, 1).bit_length() - 1
        nearest = min(measured, key=lambda m: (abs(m - lg), m))
        assert c in {w for (_, m), w in table.items() if m == nearest}, n
    assert lib.hsp_window_bits((1 << 64) - 1) in set(table.values())


def test_prepare_check():
    lib = L.lib()
    ok = lambda *a: lib.hsp_prepare_check(*a)
    assert ok(DUMMY, 5, 0, DUMMY) == 0 and ok(None, 0, 0, DUMMY) == 0 and ok(DUMMY, 5, 3, DUMMY) == 0 and ok(DUMMY, 5, 16, DUMMY) == 0
    assert ok(None, 5, 0, DUMMY) == BAD_ARG and ok(DUMMY, 5, 0, None) == BAD_ARG and ok(None, 0, 0, None) == BAD_ARG
    for bits in (-1, 1, 2, 17, 255):
        assert ok(DUMMY, 5, bits, DUMMY) == BAD_ARG, bits
    # a table index w * count + i leaves bit 31 to the sign: W * count < 2^31
    for c in (3, 13, 16):
        W = L.windows(c)
        edge = ((1 << 31) + W - 1) // W                               # the smallest count with W * count >= 2^31
        assert W * (edge - 1) < 1 << 31 <= W * edge
        assert ok(DUMMY, edge - 1, c, DUMMY) == 0 and ok(DUMMY, edge, c, DUMMY) == BAD_ARG
    assert ok(DUMMY, (1 << 40) + 1, 0, DUMMY) == BAD_ARG


def test_prepared_check():
    lib = L.lib()
    ck = lambda *a: lib.hsp_prepared_check(*a)
    assert ck(1, 1, 1, 10, 0, DUMMY, 10, DUMMY) == 0 and ck(1, 2, 2, 10, 3, DUMMY, 7, DUMMY) == 0
    assert ck(1, 1, 1, 10, 10, None, 0, DUMMY) == 0 and ck(1, 1, 1, 0, 0, None, 0, DUMMY) == 0          # n == 0; a handle of zero points
    assert ck(0, 0, 1, 0, 0, None, 0, DUMMY) == BAD_ARG                                                  # no handle
    assert ck(1, 2, 1, 10, 0, DUMMY, 1, DUMMY) == BAD_ARG and ck(1, 1, 2, 10, 0, DUMMY, 1, DUMMY) == BAD_ARG      # the other group
    assert ck(1, 1, 1, 10, 0, None, 1, DUMMY) == BAD_ARG and ck(1, 1, 1, 10, 0, DUMMY, 1, None) == BAD_ARG
    assert ck(1, 1, 1, 10, 3, DUMMY, 8, DUMMY) == BAD_ARG and ck(1, 1, 1, 10, 11, None, 0, DUMMY) == BAD_ARG
    assert ck(1, 1, 1, 10, (1 << 64) - 1, DUMMY, 2, DUMMY) == BAD_ARG                                    # first + n wraps around
