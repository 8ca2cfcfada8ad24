"""The bodies of bn254_fr_scan_batch (bn_amd/csrc/scan_ops.hpp) and its planner (host_plan.hpp bn_scan_plan) on the CPU:
tests/hostsim/hostsim_scan.cpp runs the kernels' own code over host arrays along the planner's own work list against Python integers
(tests/scan_cases.py over tests/fr_cases.py): every combination of the three flags, of the operands (a only, b only, both) and of init (given,
NULL) over the whole list of lengths, out aliasing an operand, and the seam between sub-launches.  The simulation also checks every piece
against the arrays before its lane runs, so a plan that reads or writes outside them fails here and never on a device."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as FC
import hostsim_scan_lib as HS
import scan_cases as SC

PIECES = (8, 16, 32, 64)
FANS = (2, 4, 16)
BAD_ARG = -2
OPERANDS = ("a", "b", "ab")


@pytest.fixture(scope="module")
def PF():
    sim = HS.lib()
    return int(sim.hss_shipped_piece()), int(sim.hss_shipped_fan())


@pytest.fixture(scope="module")
def every_length(PF):
    """(lens, offsets, a per term, a per segment, b, init) over the whole list of lengths, empty segments first, last and adjacent - computed
    once, never changed"""
    lens = [0] + SC.lengths(*PF) + [0, 0, 3, 0]
    n = sum(lens)
    return lens, SC.offsets_of(lens), SC.values(n, 1), SC.values(len(lens), 2), SC.values(n, 3), SC.values(len(lens), 4)


def _diff(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8]


def _case(case, which, with_init, flags):
    lens, offsets, a_term, a_seg, b, init = case
    a = None if "a" not in which else (a_seg if flags["a_per_segment"] else a_term)
    return a, (b if "b" in which else None), offsets, (init if with_init else None)


def test_the_shipped_choices_are_covered(PF):
    assert PF[0] in PIECES and PF[1] in FANS


@pytest.mark.parametrize("with_init", [True, False], ids=["init", "init_null"])
@pytest.mark.parametrize("which", OPERANDS)
@pytest.mark.parametrize("flags", SC.FLAG_SETS, ids=lambda f: "r%de%ds%d" % (f["reverse"], f["exclusive"], f["a_per_segment"]))
def test_every_flag_operand_and_init_over_the_lengths_list(PF, every_length, flags, which, with_init):
    a, b, offsets, init = _case(every_length, which, with_init, flags)
    want = FC.rows(SC.model(a, b, offsets, init, **flags))
    got, launches = HS.scan(a, b, offsets, init, *PF, **flags)
    assert np.array_equal(got, want), _diff(got, want)
    assert launches == SC.launches(every_length[0], *PF, 1 << 22)


@pytest.mark.parametrize("F", FANS)
@pytest.mark.parametrize("P", PIECES)
def test_other_piece_lengths_and_fans(P, F):
    lens = SC.lengths(P, F) + [0, 5]
    n = sum(lens)
    a, b, init, a_seg = SC.values(n, P), SC.values(n, F + 50), SC.values(len(lens), 7), SC.values(len(lens), 8)
    offsets = SC.offsets_of(lens)
    for flags in (SC.FLAG_SETS[0], SC.FLAG_SETS[-1]):                                           # no flag, all three
        aa = a_seg if flags["a_per_segment"] else a
        want = FC.rows(SC.model(aa, b, offsets, init, **flags))
        got, _ = HS.scan(aa, b, offsets, init, P, F, **flags)
        assert np.array_equal(got, want), (flags, _diff(got, want))


def test_the_bytes_do_not_depend_on_the_plan():
    lens = [0, 1, 5, 37, 300, 0, 64]
    n = sum(lens)
    a, b, init = SC.values(n, 11), SC.values(n, 12), SC.values(len(lens), 13)
    offsets = SC.offsets_of(lens)
    for flags in (dict(), dict(reverse=True, exclusive=True)):
        want = FC.rows(SC.model(a, b, offsets, init, **flags))
        for P in PIECES + (1, 3):
            for F in FANS + (3,):
                for step in (1 << 22, 7, 1):
                    got, _ = HS.scan(a, b, offsets, init, P, F, step, **flags)
                    assert np.array_equal(got, want), (P, F, step, flags)


@pytest.mark.parametrize("kind", ["ones", "minus_ones"])
def test_all_ones_and_all_minus_ones(PF, kind):
    P, F = PF
    lens = [P + 1, F * P + 1, 3]
    n = sum(lens)
    v, offsets = SC.values(n, 0, kind), SC.offsets_of(lens)
    for a, b in ((v, v), (v, None), (None, v)):
        for flags in (dict(), dict(reverse=True)):
            got, _ = HS.scan(a, b, offsets, None, P, F, **flags)
            assert np.array_equal(got, FC.rows(SC.model(a, b, offsets, None, **flags))), (kind, a is None, b is None, flags)
    if kind == "ones":                                                                          # prefix sums of ones count: 1, 2, 3, ..
        got, _ = HS.scan(None, v, offsets, None, P, F)
        assert np.array_equal(got, FC.rows([t + 1 for L in lens for t in range(L)]))


def test_a_zero_factor_resets_the_recurrence(PF):
    """a zero a[t] in the middle of a piece makes that piece's map constant: everything behind it forgets init and the terms in front"""
    P, F = PF
    L = F * P + 1
    a, b = SC.values(L, 21), SC.values(L, 22)
    a = [v or 1 for v in a]
    z = 5 * P + 3
    a[z] = 0
    got1, _ = HS.scan(a, b, [0, L], [123], P, F)
    b2 = list(b); b2[0] = (b2[0] + 1) % FC.R
    got2, _ = HS.scan(a, b2, [0, L], [456], P, F)
    assert np.array_equal(got1, FC.rows(SC.model(a, b, [0, L], [123])))
    assert np.array_equal(got1[z:], got2[z:]) and not np.array_equal(got1[z - 1], got2[z - 1])
    assert np.array_equal(got1[z], FC.rows([b[z]])[0])


@pytest.mark.parametrize("alias", ["a", "b"])
def test_out_may_be_an_operand(PF, every_length, alias):
    lens, offsets, a, _, b, init = every_length
    for flags in (dict(), dict(reverse=True), dict(exclusive=True), dict(reverse=True, exclusive=True)):
        want = FC.rows(SC.model(a, b, offsets, init, **flags))
        got, _ = HS.scan(a, b, offsets, init, *PF, alias=alias, **flags)
        assert np.array_equal(got, want), (alias, flags, _diff(got, want))
    if alias == "b":                                                                            # Horner in place: a per segment, out is b
        a_seg = every_length[3]
        flags = dict(reverse=True, a_per_segment=True)
        got, _ = HS.scan(a_seg, b, offsets, None, *PF, alias="b", **flags)
        assert np.array_equal(got, FC.rows(SC.model(a_seg, b, offsets, None, **flags)))


def test_sub_launches_cut_every_level(PF):
    P, F = PF
    lens = [P] * 25 + [20 * P]                                                                  # 25 + 20 = 45 pieces
    n = sum(lens)
    a, b, init = SC.values(n, 31), SC.values(n, 32), SC.values(len(lens), 33)
    offsets = SC.offsets_of(lens)
    for flags in (dict(), dict(reverse=True)):
        got, launches = HS.scan(a, b, offsets, init, P, F, step=20, **flags)
        assert launches == SC.launches(lens, P, F, 20)
        assert np.array_equal(got, FC.rows(SC.model(a, b, offsets, init, **flags)))
    if (P, F) == (16, 16):
        assert launches == (3, 1, 2, 3)


@pytest.mark.parametrize("m", [1, 255, 256, 257])
def test_segment_counts_around_a_workgroup(PF, m):
    P, F = PF
    cyc = [L for L in SC.lengths(P, F) if L <= F * P + 1]
    lens = [cyc[j % len(cyc)] for j in range(m)]
    n = sum(lens)
    a, b, init = SC.values(n, m), SC.values(n, m + 1), SC.values(m, m + 2)
    offsets = SC.offsets_of(lens)
    got, _ = HS.scan(a, b, offsets, init, P, F)
    assert np.array_equal(got, FC.rows(SC.model(a, b, offsets, init)))


def test_polynomial_division_and_powers_as_scans(PF):
    """the shapes bn_amd.poly uses: divide_linear is ONE reverse scan with a = z per segment and b = p, powers ONE exclusive scan with init one"""
    P, F = PF
    L = F * P + 1
    p, z = SC.values(L, 41), 0x1234567
    out = SC.model([z], p, [0, L], None, reverse=True, a_per_segment=True)
    got, _ = HS.scan([z], p, [0, L], None, P, F, reverse=True, a_per_segment=True)
    assert np.array_equal(got, FC.rows(out))
    y, q = out[0], out[1:]
    assert y == sum(c * pow(z, i, FC.R) for i, c in enumerate(p)) % FC.R
    back = [0] * L                                                                              # q * (X - z) + y == p
    for i, c in enumerate(q):
        back[i + 1] = (back[i + 1] + c) % FC.R
        back[i] = (back[i] - c * z) % FC.R
    back[0] = (back[0] + y) % FC.R
    assert back == [v % FC.R for v in p]
    got, _ = HS.scan([z], None, [0, L], [1], P, F, exclusive=True, a_per_segment=True)
    assert np.array_equal(got, FC.rows([pow(z, i, FC.R) for i in range(L)]))


def test_the_argument_checks():
    sim = HS.lib()
    D = C.c_void_p(0x1000)
    off = lambda *v: (C.c_size_t * len(v))(*v)
    ok = lambda *a: sim.hss_check(*a)
    assert ok(D, D, off(0, 1, 3), 2, 0, D) == 0 and ok(D, None, off(0, 1, 3), 2, 7, D) == 0 and ok(None, D, off(0, 1, 3), 2, 1, D) == 0
    assert ok(None, None, off(0, 1, 3), 2, 0, D) == BAD_ARG                                     # both operands NULL
    for flags in (8, 16, 1 << 31, 15):
        assert ok(D, D, off(0, 1, 3), 2, flags, D) == BAD_ARG                                   # an unknown flag bit
    assert ok(D, D, None, 2, 0, D) == BAD_ARG                                                   # offsets == NULL with m > 0
    assert ok(D, D, off(1, 1, 3), 2, 0, D) == BAD_ARG                                           # offsets[0] != 0
    assert ok(D, D, off(0, 4, 3), 2, 0, D) == BAD_ARG                                           # decreasing
    assert ok(D, D, off(0, (1 << 40) + 1), 1, 0, D) == BAD_ARG
    assert ok(D, D, off(0, 1, 3), 2, 0, None) == BAD_ARG                                        # a NULL out
    assert ok(D, D, off(0, 0, 0), 2, 0, D) == 0                                                 # only empty segments
