"""The bodies of bn_amd/csrc/fr_sqrt_ops.hpp and the packing bodies of babyjub_ops.hpp on the CPU (tests/hostsim/hostsim_bjj_pack.cpp, g++
-DBN_BOUNDS) against the integer model of tests/bjj_pack_cases.py, byte for byte: both forms of the square root on every case, the ratio,
packing, unpacking and the packed verifier with every status in its precedence."""
import numpy as np
import pytest

import babyjub_cases as BC
import bjj_pack_cases as PK
import fr_cases as FC
import hostsim_bjj_pack_lib as H

R = PK.R


@pytest.mark.parametrize("form", [0, 1])
def test_sqrt_on_every_case_and_across_a_seam(form):
    vals = list(PK.sqrt_values())
    want, want_ok = PK.model_sqrt(vals)
    got, ok, launches = H.sqrt(FC.rows(vals), form)
    assert np.array_equal(got, want) and ok.tolist() == want_ok.tolist() and launches == 1
    assert set(want_ok.tolist()) == {0, 1}
    got, ok, launches = H.sqrt(FC.rows(vals), form, step=7, in_place=True)
    assert np.array_equal(got, want) and ok.tolist() == want_ok.tolist() and launches == -(-len(vals) // 7)
    got, ok, _ = H.sqrt(FC.rows(vals), form, with_ok=False)
    assert np.array_equal(got, want) and ok is None


@pytest.mark.parametrize("form", [0, 1])
def test_sqrt_ratio_takes_no_inversion_and_agrees_with_the_quotient(form):
    rng = np.random.default_rng(2603)
    us = list(PK.sqrt_values()[:40]) + [FC.rand(rng) for _ in range(24)]
    vs = [FC.rand(rng) or 1 for _ in us]
    vs[0], vs[1], vs[2] = 1, R - 1, 5
    want, want_ok = PK.model_sqrt([u * BC.inv(v) % R for u, v in zip(us, vs)])
    got, ok = H.sqrt_ratio(FC.rows(us), FC.rows(vs), form)
    assert np.array_equal(got, want) and ok.tolist() == want_ok.tolist()
    assert set(want_ok.tolist()) == {0, 1}


def test_pack_gives_the_models_bytes():
    pts = [p for _, p, st in PK.unpack_records() if st == 0] + [p for _, p in BC.edge_points()]
    want = PK.byte_rows([PK.pack(p) for p in pts])
    got, launches = H.pack(BC.point_rows(pts))
    assert np.array_equal(got, want) and launches == 1
    got, launches = H.pack(BC.point_rows(pts), step=5)
    assert np.array_equal(got, want) and launches == -(-len(pts) // 5)
    H.pack(BC.point_rows(BC.RAW_OUT_OF_RANGE))                                        # words not below r: some bytes, no abort


@pytest.mark.parametrize("form", [0, 1])
def test_unpack_gives_the_models_points_and_statuses(form):
    recs = PK.unpack_records()
    B = PK.byte_rows([b for b, _, _ in recs])
    want, want_st = BC.point_rows([p for _, p, _ in recs]), [st for _, _, st in recs]
    got, st, launches = H.unpack(B, form)
    assert st.tolist() == want_st and np.array_equal(got, want) and launches == 1
    assert set(want_st) == {0, 1, 3, 4}
    got, st, launches = H.unpack(B, form, step=9)
    assert st.tolist() == want_st and np.array_equal(got, want) and launches == -(-len(recs) // 9)
    ok = [i for i, s in enumerate(want_st) if s == 0]
    assert np.array_equal(H.pack(got[ok])[0], B[ok])                                  # pack(unpack(b)) == b for accepted b


@pytest.mark.parametrize("form", [0, 1])
def test_verify_packed_with_every_status_in_its_precedence(form):
    rows = PK.packed_signature_rows()
    want = [r[4] for r in rows]
    assert set(want) == {0, 1, 3, 4, 6}
    got, launches = H.verify_packed(*PK.signature_arrays(rows), form)
    assert got.tolist() == want and launches == 1
    got, launches = H.verify_packed(*PK.signature_arrays(rows), form, step=5)
    assert got.tolist() == want and launches == -(-len(rows) // 5)


def test_the_library_ships_one_of_the_two_forms():
    assert H.lib().hsp_shipped_form() in (0, 1)
