"""The bodies of the wide Poseidon kernels (bn_amd/csrc/poseidon_wide_ops.hpp) and the C++ table derivation (poseidon_wide_table.hpp) on the
CPU, built with -DBN_BOUNDS, against the integer model of tests/poseidon_wide_cases.py: every G of 4 / 8 / 16 at the widths on both sides of
every fr_dot chunk seam and every elements-per-lane seam, edge rows, n_outs and init, and chains whose neighbours run different numbers of
blocks.  A group is a loop over its lanes per phase; the exchange buffer is laid out like the workgroup's LDS."""
import numpy as np
import pytest

import fr_cases as FC
import hostsim_poseidon_wide_lib as H
import poseidon_wide_cases as WC

R = WC.R
LANES = (4, 8, 16)


@pytest.mark.parametrize("t", range(2, 18))
def test_the_cpp_table_is_the_python_derivation(t):
    from bn_amd import poseidon
    assert H.lib().hspw_rounds_partial(t) == poseidon.R_P[t] and H.lib().hspw_table_elems(t) == (8 + poseidon.R_P[t]) * t + t * t
    C, M = H.table(t)
    pC, pM = poseidon.constants(t)
    assert C == list(pC)
    assert M == [list(r) for r in pM]


def test_the_table_rejects_other_widths():
    buf = np.zeros(8, np.uint32)
    for t in (-1, 0, 1, 18):
        assert H.lib().hspw_table_elems(t) == 0 and H.lib().hspw_rounds_partial(t) == -1
        assert H.lib().hspw_table(t, buf.ctypes.data_as(H._U32P)) == -2
    assert H.lib().hspw_default_lanes() in LANES


@pytest.fixture(scope="module")
def seam_cases():
    """{t: (rows, init, {n_outs: expected with init, expected without})} - computed once"""
    out = {}
    for t in WC.SEAM_WIDTHS:
        rows = WC.ex_rows(t - 1, 6, 500 + t) + [[0] * (t - 1)]
        init = [R - 1, 0, 1] + WC.values(len(rows) - 3, 600 + t)
        full_i = [WC.permute([i] + r) for i, r in zip(init, rows)]
        full_0 = [WC.permute([0] + r) for r in rows]
        out[t] = (rows, init, full_i, full_0)
    return out


@pytest.mark.parametrize("G", LANES)
@pytest.mark.parametrize("t", WC.SEAM_WIDTHS)
def test_ex_at_the_seam_widths(seam_cases, G, t):
    rows, init, full_i, full_0 = seam_cases[t]
    if t == 17:
        assert full_0[0][0] == WC.KNOWN[16]
    for n_outs in sorted({1, 2, t}):
        got, launches = H.ex(G, rows, None, n_outs)
        assert launches == 1 and np.array_equal(got, FC.rows([v for s in full_0 for v in s[:n_outs]])), (G, t, n_outs)
        got, _ = H.ex(G, rows, init, n_outs)
        assert np.array_equal(got, FC.rows([v for s in full_i for v in s[:n_outs]])), (G, t, n_outs, "init")


@pytest.mark.parametrize("G", LANES)
def test_sub_launches_cover_every_row_once(G):
    rows = WC.ex_rows(7, 9, 77)
    want = FC.rows([WC.hash_ex(r)[0] for r in rows])
    for step, launches in ((1 << 22, 1), (4 * G, 3), (G, 9), (1, 9)):
        got, n = H.ex(G, rows, None, 1, step=step)
        assert n == launches and np.array_equal(got, want), (G, step)


@pytest.mark.parametrize("G", LANES)
@pytest.mark.parametrize("rate", [1, 2, 5, 15, 16])
def test_chains_whose_neighbours_run_different_block_counts(G, rate):
    lengths = WC.mixed_lengths(rate, 10, 900 + rate)
    assert set(WC.chain_lengths(rate)) <= set(lengths)
    recs, flat, off = WC.records(lengths, 901 + rate)
    want = FC.rows([WC.hash_chain(r, rate) for r in recs])
    got, launches = H.chain(G, flat, off, rate)
    assert launches == 1 and np.array_equal(got, want)
    got, launches = H.chain(G, flat, off, rate, step=3 * G)
    assert launches == 4 and np.array_equal(got, want)


def test_chain_edges():
    # only empty records, one record, and records of r - 1 (every word of the state and of the padding meets the largest element)
    for G in LANES:
        got, _ = H.chain(G, [], [0, 0, 0], 16)
        assert np.array_equal(got, FC.rows([WC.hash_chain([], 16)] * 2))
        got, _ = H.chain(G, [R - 1] * 33, [0, 33], 16)
        assert np.array_equal(got, FC.rows([WC.hash_chain([R - 1] * 33, 16)]))
        got, n = H.chain(G, [], [0], 16)
        assert got.shape == (0, 4) and n == 0


def test_the_checks_of_host_plan():
    l = H.lib()
    D, BAD = 0x100000, -2
    assert [l.hspw_ex_check(D, k, None, 1, D + (1 << 30), 1, 1) for k in (0, 1, 16, 17)] == [BAD, 0, 0, BAD]
    assert [l.hspw_ex_check(D, 3, None, k, D + (1 << 30), 1, 1) for k in (0, 1, 4, 5)] == [BAD, 0, 0, BAD]
    assert l.hspw_ex_check(D, 17, None, 1, D, 0, 1) == BAD and l.hspw_ex_check(None, 2, None, 1, None, 0, 1) == 0
    assert l.hspw_ex_check(None, 2, None, 1, D, 1, 1) == BAD and l.hspw_ex_check(D, 2, None, 1, None, 1, 1) == BAD
    assert l.hspw_ex_check(D, 16, None, 1, D + (1 << 50), (1 << 40) // 17, 0) == 0 and l.hspw_ex_check(D, 16, None, 1, D + (1 << 50), (1 << 40) // 17 + 1, 0) == BAD
    # overlap: out inside in, out inside init, and the device form does not look
    assert l.hspw_ex_check(D, 2, None, 1, D + 32, 4, 1) == BAD and l.hspw_ex_check(D, 2, None, 1, D + 8 * 32, 4, 1) == 0
    assert l.hspw_ex_check(D, 2, D + 4096, 1, D + 4096 + 96, 4, 1) == BAD and l.hspw_ex_check(D, 2, D + 4096, 1, D + 4096 + 128, 4, 1) == 0
    assert l.hspw_ex_check(D, 2, None, 1, D, 4, 0) == 0
    off = lambda *v: (H.C.c_size_t * len(v))(*v)
    assert [l.hspw_chain_check(D, off(0, 2), 1, r, D + 4096, 1) for r in (0, 1, 16, 17)] == [BAD, 0, 0, BAD]
    assert l.hspw_chain_check(D, off(1, 2), 1, 16, D + 4096, 1) == BAD and l.hspw_chain_check(D, off(0, 3, 2), 2, 16, D + 4096, 1) == BAD
    assert l.hspw_chain_check(None, off(0, 0), 1, 16, D, 1) == 0 and l.hspw_chain_check(None, off(0, 1), 1, 16, D, 1) == BAD
    assert l.hspw_chain_check(D, None, 1, 16, D + 4096, 1) == BAD and l.hspw_chain_check(D, off(0, 1), 1, 16, None, 1) == BAD
    assert l.hspw_chain_check(D, off(0, (1 << 40) + 1), 1, 16, D + (1 << 50), 0) == BAD and l.hspw_chain_check(D, off(0, 1 << 40), 1, 16, D + (1 << 50), 0) == 0
    assert l.hspw_chain_check(D, off(0, 4), 1, 16, D + 96, 1) == BAD and l.hspw_chain_check(D, off(0, 4), 1, 16, D + 128, 1) == 0
    assert l.hspw_chain_check(D, None, 0, 16, None, 1) == 0 and l.hspw_chain_check(D, None, 0, 17, None, 1) == BAD
