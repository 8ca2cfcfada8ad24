"""Point validation and the endomorphism subgroup test of G2 under the bounds-enforcing host simulation (tests/hostsim/hostsim_subgroup.cpp: the
bodies of bn_amd/csrc/subgroup_ops.hpp compiled with g++ -DBN_BOUNDS, so every lazy-limb bound of the new chain is checked on the CPU): every case
of subgroup_cases.py against the integer model, whose membership is [r]P == 0 alone; the endomorphism test against the r - 1 chain of io_wire.hpp;
and the G2 decoders, which call the test behind BN254_G2_SUBGROUP_ENDO, on the records of compress_cases.py - statuses and bytes as before."""
import numpy as np
import pytest

import bn_model as M
import compress_cases as CC
import hash_g2_cases as HC
import hostsim_subgroup_lib as H
import subgroup_cases as S


def test_bounds_are_enforced_and_the_decoders_take_the_shipped_test():
    assert H.lib().hss_bounds_enabled() == 1
    src = (H.CSRC / "io_wire.hpp").read_text()
    shipped = int(src.split("#define BN254_G2_SUBGROUP_ENDO ")[1].split()[0])
    assert H.decoders_use_endo() == bool(shipped)


@pytest.mark.parametrize("g", (1, 2))
def test_every_case_has_the_models_status(g):
    cases = S.g1_cases() if g == 1 else S.g2_cases()
    got = H.validate(g, np.stack([r for _, r, _ in cases]))
    for (name, _, want), st in zip(cases, got):
        assert st == want, (name, st, want)


@pytest.mark.parametrize("g", (1, 2))
def test_a_batch_is_its_records_one_by_one(g):
    rows, want = (S.g1_batch if g == 1 else S.g2_batch)(len(S.g2_cases()) + 5, 7)
    assert np.array_equal(H.validate(g, rows), want)
    assert H.validate(g, rows[:0]).shape == (0,)


def _affine_xy(p):
    a = HC.aff(p)
    return np.array([l for c in a for h in c for l in M.to_mont_limbs(h)], np.uint64)


def test_the_endomorphism_test_agrees_with_the_chain_on_every_point_of_the_twist():
    seen = set()
    for name, row, st in S.g2_cases():
        if st not in (S.OK, S.E_SUBGROUP):
            continue
        member = st == S.OK
        assert H.endo(row) == member, name
        p = S.g2_point(row)
        if p[2] == HC.ZERO:                                    # the chain takes an affine point: infinity has none
            continue
        xy = _affine_xy(p)
        assert H.chain(xy) == member, name
        assert H.decoder_test(xy) == member, name
        seen.add(member)
    assert seen == {True, False}


def _wire(x, y):
    return b"\x04" + b"".join((c[1] * M.Q + c[0]).to_bytes(64, "big") for c in (x, y))


def test_the_wire_decoder_reports_what_it_did():
    """tag 4 records: accepted points of compress_cases, a point outside the subgroup, a point off the curve"""
    for pt in CC.multiples(2)[:6]:
        st, out = H.g2_decode(_wire(*pt))
        assert st == 0 and np.array_equal(out, CC.words(2, pt))
    x, y = CC.g2_outside_subgroup()
    for yy in (y, M.f2_neg(y)):
        st, out = H.g2_decode(_wire(x, yy))
        assert st == 5 and np.array_equal(out, CC.words(2, None))
    gx, gy = CC.multiples(2)[0]
    st, out = H.g2_decode(_wire(gx, M.f2_add(gy, (1, 0))))
    assert st == 4 and np.array_equal(out, CC.words(2, None))
    for l, p in S._small_order_points():                       # small order: partial sums of the chain pass through infinity
        st, out = H.g2_decode(_wire(*HC.aff(p)))
        assert st == 5, l
    st, out = H.g2_decode(b"\x00" * 129)
    assert st == 0 and np.array_equal(out, CC.words(2, None))


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_decompression_is_unchanged_on_the_existing_cases(fmt):
    code = CC.FORMATS[fmt]
    seen = set()
    for name, b, want, pt in CC.records(2, code):
        for form in (0, 1):
            st, out = H.g2_decompress(b, code, form)
            assert st == want, (name, form, st, want)
            assert np.array_equal(out, CC.words(2, pt)), (name, form)
        seen.add(want)
    assert seen >= {0, 1, 3, 4, 5}
