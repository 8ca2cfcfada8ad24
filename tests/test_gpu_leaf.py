"""The GPU's inline-asm field leaves DIRECTLY, at the operand bounds they state: every leaf of bn_amd/csrc/fe_asm.hpp (fe_mul, fe_sqr, fe_mul2,
fe_mul2s, fe_mul6, fe_mul5, fe_wmul2, fe_wmul2s, the four fe_wred specialisations) and every asm chain of the fused reductions (BN_LC_CHAIN in
fe.hpp) on raw limbs - tests/leafprobe/bn254_leafprobe.hip, one case per lane, one launch per leaf - in both build contexts: forced inline
(BN_INLINE_ALL, the pairing kernels' form) and as real functions.  The whole-kernel parity tests feed canonical records and cannot put a limb at
lb (2^29 - 1), a value at vb q or a signed difference at its extremes; here the cases of tests/leaf_cases.py do (hot limbs, ceilings, degenerate,
random), and the result must equal the bounds-checked C++ twin (tests/hostsim/hostsim_leaf.cpp) LIMB FOR LIMB - fe.hpp's promise - and satisfy the
integer model.  The expected values come from the CPU; tests/test_hostsim_leaf.py proves the cases to be inside every contract."""
import numpy as np
import pytest

import hostsim_leaf_lib as H
import leaf_cases as L

pytestmark = pytest.mark.gpu
NAMES = [l[0] for l in L.LEAVES]
_twin = {}


def twin(name):
    """(operands, flags, the twin's result) of every case of a leaf, computed once for both contexts"""
    if name not in _twin:
        ops, bounds, flags = L.pack(name)
        want = H.run(L.LEAF_ID[name], ops, bounds, flags, L.LEAVES[L.LEAF_ID[name]][2])
        for a in (ops, flags, want):
            a.setflags(write=False)
        _twin[name] = (ops, flags, want)
    return _twin[name]


@pytest.mark.parametrize("ctx", ["inl", "fn"])
def test_the_probe_holds_the_same_list(ctx):
    import leafprobe
    assert leafprobe.leaf_table(ctx) == H.leaf_table() == [(name, kinds, outw) for name, kinds, outw, _ in L.LEAVES]


@pytest.mark.parametrize("ctx", ["inl", "fn"])
@pytest.mark.parametrize("name", NAMES)
def test_leaf_equals_its_twin_limb_for_limb(name, ctx):
    import leafprobe
    ops, flags, want = twin(name)
    n, outw = want.shape
    assert n % 64 != 0 and n > 64                      # several blocks and a ragged last wave
    got, ops_after, flags_after = leafprobe.run(ctx, L.LEAF_ID[name], ops, flags, outw)
    cs = L.cases(name)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s [%s]: %d of %d cases differ from the twin, first: %s" % (
        name, ctx, bad.size, n, ["%s: got %s want %s" % (cs[i][0], [hex(int(x)) for x in got[i]], [hex(int(x)) for x in want[i]]) for i in bad[:3]])
    count, first = L.failures(name, got)
    assert count == 0, "%s [%s]: %d of %d cases fail the integer model, first: %s" % (name, ctx, count, n, first)
    assert np.array_equal(ops_after, ops) and np.array_equal(flags_after, flags), "the kernel wrote its operands"
