"""The passes of bn254_fr_mle_quotients (host_plan.hpp bn_mle_quotients_plan) on the CPU, through tests/hostsim/hostsim_mle_open.cpp: the levels,
lanes and scratch of every plan, and the index arithmetic of the passes replayed in Python - every record of the heap written exactly
once, and nothing read that was not written."""
import pytest

import hostsim_mle_open_lib as HO
import mle_open_cases as OC

RHOS = (1, 2, 3, 4)
NVS = range(14)


@pytest.mark.parametrize("rho", RHOS)
def test_the_passes_of_every_plan(rho):
    for nv in NVS:
        passes, slots = HO.plan(nv, rho)
        assert (passes, slots) == OC.plan(nv, rho), (nv, rho)
        levels = [p[0] for p in passes]
        assert sum(levels) == nv and len(passes) == -(-nv // rho)
        assert levels == [rho] * (nv // rho) + ([nv % rho] if nv % rho else [])                # the full passes come before the remainder
        length = 1 << nv
        for p, (lv, vars_, lanes, first, last) in enumerate(passes):
            assert 1 << vars_ == length and lanes == length >> lv                            # lanes per pass are L / 2^levels
            assert first == (p == 0) and last == (p == len(passes) - 1)
            length = lanes
        assert length == 1
        assert slots == ((1 << nv) >> levels[0] if passes else 0)


@pytest.mark.parametrize("rho", RHOS)
def test_replaying_the_index_arithmetic_writes_every_heap_record_once(rho):
    for nv in NVS:
        passes, slots = HO.plan(nv, rho)
        n = 1 << nv
        heap = [0] * n                                                                          # writes per record
        scratch = [None] * slots                                                                # the pass that wrote the record last
        for p, (lv, vars_, lanes, first, last) in enumerate(passes):
            reads, writes = [], []
            for i in range(lanes):
                for c in range(1 << lv):
                    at = i + c * lanes
                    assert at < 1 << vars_
                    if not first:
                        assert at < slots and scratch[at] == p - 1, (nv, rho, p, at)              # what the pass before left there
                    reads.append(at)
                for k in range(lv):
                    j = vars_ - 1 - k
                    for c in range(1 << (lv - 1 - k)):
                        at = (1 << j) + i + c * lanes
                        assert 1 <= at < n
                        heap[at] += 1
                if last:
                    assert i == 0
                    heap[0] += 1
                else:
                    assert i < slots
                    writes.append(i)
            assert sorted(reads) == list(range(1 << vars_))                                     # every record of the table is read by one lane
            for i in writes:
                scratch[i] = p
        if nv == 0:
            assert passes == [] and heap == [0]                                                 # the one record is copied
        else:
            assert heap == [1] * n, (nv, rho)
            assert passes[-1][4] == 1
