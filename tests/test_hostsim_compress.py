"""The device bodies of the compressed encodings on the CPU (tests/hostsim/hostsim_compress.cpp: sqrt_ops.hpp and io_compress.hpp compiled with
g++ -DBN_BOUNDS, so the lazy-limb bounds are enforced through both exponentiation chains) against the integer model of compress_cases.py."""
import random

import numpy as np
import pytest

import bn_model as M
import compress_cases as CC
import hostsim_compress_lib as HS

Q = M.Q
FORMS = [0, 1]


def _fq_samples():
    rng = random.Random(20)
    xs = [0, 1, 4, 3, Q - 1, Q - 4]
    res = [pow(rng.randrange(1, Q), 2, Q) for _ in range(16)]
    non = [-r % Q for r in res]                                  # -1 is a non-residue
    return xs + res + non


@pytest.mark.parametrize("form", FORMS)
def test_fe_sqrt_cand(form):
    e = (Q - 3) // 4
    seen = set()
    for a in _fq_samples():
        t, y, chi = HS.fe_sqrt_cand(a, form)
        assert t == pow(a, e, Q) and y == t * a % Q and chi == t * t * a % Q == pow(a, (Q - 1) // 2, Q), a
        assert y * y % Q == chi * a % Q
        assert chi == (0 if a == 0 else 1 if CC.fq_is_square(a) else Q - 1)
        seen.add(chi)
    assert seen == {0, 1, Q - 1}


def _f2_samples():
    rng = random.Random(21)
    fixed = [(4, 0), (3, 0), (Q - 4, 0), (0, 5), (0, 0), (1, 0), (Q - 1, 0), (0, 1)]
    squares = [M.f2_sqr((rng.randrange(Q), rng.randrange(Q))) for _ in range(64)]
    anything = [(rng.randrange(Q), rng.randrange(Q)) for _ in range(64)]
    return fixed, squares, anything


@pytest.mark.parametrize("form", FORMS)
def test_f2_sqrt(form):
    fixed, squares, anything = _f2_samples()
    for a in fixed + squares:
        root, sq = HS.f2_sqrt(a, form)
        assert CC.f2_is_square(a), a                              # every element of Fq is a square in Fq2; (0, 5) and (0, 1) have square norms
        assert sq and M.f2_sqr(root) == (a[0] % Q, a[1] % Q), a
    non = 0
    for a in anything:
        root, sq = HS.f2_sqrt(a, form)
        assert sq == CC.f2_is_square(a), a                        # the Legendre symbol of the norm
        if sq:
            assert M.f2_sqr(root) == a
        non += not sq
    assert 16 <= non <= 48, non                                   # about half


def test_sign_rule():
    rng = random.Random(22)
    for y in [1, 2, (Q - 1) // 2, (Q + 1) // 2, Q - 1, Q - 2] + [rng.randrange(1, Q) for _ in range(16)]:
        assert HS.fe_sign(y) == CC.fq_sign(y) == 1 - CC.fq_sign(-y % Q), y
        assert HS.f2_sign((y, 0)) == CC.fq_sign(y) and HS.f2_sign((5, y)) == HS.f2_sign((Q - 5, y)) == CC.fq_sign(y)
    assert CC.compress(1, (1, 2), CC.ARK).hex() == "01" + "00" * 31
    assert CC.compress(1, (1, 2), CC.GNARK).hex() == "80" + "00" * 30 + "01"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
@pytest.mark.parametrize("g", [1, 2])
def test_records_against_the_model(g, fmt, form):
    f = CC.FORMATS[fmt]
    seen = set()
    for name, b, st, pt in CC.records(g, f):
        got_st, got = HS.decompress(g, b, f, form)
        assert got_st == st, (name, got_st, st)
        assert np.array_equal(got, CC.words(g, pt)), name
        seen.add(st)
        if st == CC.OK:                                           # compress(decompress(b)) == b, from the normalised and from a raw Jacobian image
            assert HS.compress(g, got, f) == b, name
            if pt is not None:
                o = M.FQ_OPS if g == 1 else M.FQ2_OPS
                jac = M.g_double(o, M.g_double(o, (pt[0], pt[1], o.one)))
                assert HS.compress(g, CC.jacobian_words(g, jac), f) == CC.compress(g, CC.affine(g, jac), f), name
    assert seen == ({0, 1, 3, 4} if g == 1 else {0, 1, 3, 4, 5})


def test_case_lists_hold_what_they_promise():
    for g in (1, 2):
        for f in (CC.ARK, CC.GNARK):
            recs = {r[0]: r for r in CC.records(g, f)}
            assert recs["infinity"][2] == 0 and recs["infinity"][3] is None
            assert recs["flags=sign0"][2] == recs["flags=sign1"][2] == 0 and recs["flags=sign0"][3] != recs["flags=sign1"][3]
            assert recs["flags=inf"][2] == recs["flags=bad"][2] == recs["infinity+stray"][2] == 3
            assert recs["bad+range"][2] == recs["bad+nopoint"][2] == 3 and recs["range+nopoint"][2] == 1
            assert all(r[2] == 1 for n, r in recs.items() if n.startswith("range["))
            assert all(r[2] == 4 for n, r in recs.items() if n.startswith("nopoint"))
            signs = {(CC.fq_sign(r[3][1]) if g == 1 else CC.f2_sign(r[3][1])) for r in recs.values() if r[3] is not None}
            assert signs == {0, 1}
    assert all(r[2] == 5 for r in CC.records(2, CC.ARK) if r[0].startswith("outside"))
    gen = CC.records(1, CC.ARK)[0]
    assert gen[3] == (1, 2) and gen[1].hex() == "01" + "00" * 31 and CC.records(1, CC.GNARK)[0][1].hex() == "80" + "00" * 30 + "01"
