"""The bodies of bn254_g{1,2}_ntt_batch (bn_amd/csrc/group_ntt_ops.hpp: butterflies and passes; group_ops.hpp: the normalisation) on the CPU:
tests/hostsim/hostsim_group_ntt.cpp runs the kernels' own code over host arrays, G2 on simulated lane pairs, through the steps of the
shipped planner (host_plan.hpp bn_group_ntt_group), with the run-time enforcement of every limb / value bound on (-DBN_BOUNDS: a violated
bound aborts the process), against the O(n^2) sums of tests/group_ntt_cases.py.  Expected bytes are exact."""
import ctypes as C

import numpy as np
import pytest

import group_ntt_cases as GC

_U32P = C.POINTER(C.c_uint32)
SHIFTS = (None, 5)
BIG = 1 << 22


@pytest.fixture(scope="module")
def sim():
    return GC.hostsim()


def _ntt(lib, g, P, log_n, inverse, shift, cap=BIG, chain_cap=BIG, in_place=False):
    P = np.ascontiguousarray(P, np.uint64)
    out = P.copy() if in_place else np.full_like(P, 0x5a5a5a5a5a5a5a5a)
    src = out if in_place else P
    sh = GC.shift_row(shift)
    rc = lib.hsg_ntt(C.c_int(g), src.ctypes.data_as(_U32P), out.ctypes.data_as(_U32P), C.c_uint32(log_n), C.c_size_t(P.shape[0] >> log_n), C.c_int(1 if inverse else 0),
                     None if sh is None else sh.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.c_size_t(chain_cap))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("log_n", GC.LOGS)
@pytest.mark.parametrize("g", [1, 2])
def test_the_bodies_against_the_model(sim, g, log_n):
    n = 1 << log_n
    for name, P in GC.inputs(g, log_n, seed=10 * g + log_n).items():
        for inverse in (False, True):
            for shift in SHIFTS:
                want = GC.model(g, P, log_n, inverse, shift)
                got = _ntt(sim, g, P, log_n, inverse, shift)
                assert np.array_equal(got, want), (g, log_n, name, inverse, shift, np.nonzero((got != want).any(axis=1))[0])
                # the stage whose twiddles are all one runs no chain; a shift or an inverse is one pass of n chains more
                passes = n if log_n and (inverse or shift is not None) else 0
                assert sim.hsg_chains() == (n // 2 * (log_n - 1) if log_n else 0) + passes
        assert np.array_equal(_ntt(sim, g, P, log_n, True, 5, in_place=True), GC.model(g, P, log_n, True, 5)), ("in place", g, log_n, name)


@pytest.mark.parametrize("g", [1, 2])
def test_special_inputs_give_what_the_definition_says(sim, g):
    sets = GC.inputs(g, 3, seed=3)
    zero = GC.normalize(g, sets["all infinity"][:1])[0]
    out = _ntt(sim, g, sets["constant"], 3, False, None)
    eight = GC.model(g, sets["constant"][:1], 0)                                # [1] P ...
    mul = GC.oracle().g1_mul if g == 1 else GC.oracle().g2_mul
    eight = GC.normalize(g, [mul(eight[0], GC.FC.rows([8])[0])])[0]             # ... and [8] P
    assert np.array_equal(out[0], eight) and all(np.array_equal(r, zero) for r in out[1:])
    assert all(np.array_equal(r, zero) for r in _ntt(sim, g, sets["all infinity"], 3, False, 5))
    delta = np.concatenate([sets["random"][:1], sets["all infinity"][1:]])
    out = _ntt(sim, g, delta, 3, False, None)
    assert all(np.array_equal(r, GC.normalize(g, delta[:1])[0]) for r in out)


@pytest.mark.parametrize("g", [1, 2])
def test_groups_and_sub_launches_do_not_change_the_bytes(sim, g):
    """three transforms of 8 with a launch cap of 4 units (every transform a group of its own, every step several sub-launches), of 16 (two
    transforms per group, then one), chain launches capped below the others, in place and out of place"""
    P = GC.batch(g, 3, 3, seed=7)
    for inverse, shift in ((False, 5), (True, None)):
        want = GC.model(g, P, 3, inverse, shift)
        for cap, chain_cap in ((4, BIG), (16, BIG), (16, 3), (BIG, BIG)):
            for in_place in (False, True):
                assert np.array_equal(_ntt(sim, g, P, 3, inverse, shift, cap, chain_cap, in_place), want), (g, inverse, shift, cap, chain_cap, in_place)


@pytest.mark.parametrize("g", [1, 2])
def test_round_trip(sim, g):
    P = GC.batch(g, 2, 2, seed=1)
    for shift in SHIFTS:
        assert np.array_equal(_ntt(sim, g, _ntt(sim, g, P, 2, False, shift), 2, True, shift), GC.normalize(g, P))
