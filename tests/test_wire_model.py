"""The wire format without a GPU: the integer model of wire_cases.py against the project's oracle and against the device bodies of
bn_amd/csrc/io_wire.hpp compiled with g++ (tests/hostsim/hostsim.cpp with -DBN_BOUNDS, and hostsim_subgroup.cpp), on every case of the lists -
records that fail several checks at once, the 512-bit extremes of the Fq2 split, Fr at its limits, Jacobian inputs of the encoders - and the
model of the byte stream against expectations written out by hand.  Every comparison is of exact bytes; no case is skipped."""
import ctypes as C

import numpy as np
import pytest

import hostsim_lib
import hostsim_subgroup_lib as HS
import wire_cases as W
from conftest import canon_infinity

_U8P, _U32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def hs():
    return hostsim_lib.HostSim(bounds=True)


def _dec(lib, fn, rec, words):
    """a decoder body on one record -> (status, words); the output starts as a pattern the body has to overwrite"""
    b = np.frombuffer(bytes(rec), np.uint8).copy()
    out = np.full(words, 0x5a5a5a5a5a5a5a5a, np.uint64)
    rc = getattr(lib, fn)(b.ctypes.data_as(_U8P), out.ctypes.data_as(_U32P))
    assert bytes(b) == bytes(rec)
    return rc, out


def _enc(lib, fn, row, size):
    p = np.ascontiguousarray(row, np.uint64).copy()
    out = np.full(size, 0xa5, np.uint8)
    getattr(lib, fn)(p.ctypes.data_as(_U32P), out.ctypes.data_as(_U8P))
    assert np.array_equal(p, row)
    return out


def test_the_lists_cover_what_they_claim():
    g1, g2, fr = W.g1_collision_cases(), W.g2_collision_cases(), W.fr_cases()
    assert len(g1) == 5 * (3 * 3 + 1) and len(g2) >= 5 * 16 + 2 * 7 + 2
    assert {c.status for c in g1} == {0, 1, 3, 4} and {c.status for c in g2} == {0, 2, 3, 4, 5}
    assert [st for _, _, st, _ in fr] == [0, 0, 0, 1, 1, 1, 1, 0]
    assert {c.status for c in g1 + g2} | {st for _, _, st, _ in fr} == {0, 1, 2, 3, 4, 5}
    for g in (1, 2):
        cases = W.collision_cases(g)
        assert len({c.name for c in cases}) == len(cases)
        for pair, found in W.separating_cases(g).items():                # every adjacent pair of the priority list: a record that fails exactly these two
            assert found, (g, pair)
            assert all(c.status == dict(W.PRIORITY[g])[pair[0]] for c in found)
        for c in cases:                                                   # tag 0 wins over everything; a record that fails nothing is accepted
            assert (c.status == 0) == (c.rec[0] == 0 or not c.failed), c.name
            assert (c.point is None) == (c.status != 0 or c.rec[0] == 0), c.name
        assert any(c.rec[0] == 0 and any(c.rec[1:]) for c in cases)       # infinity with padding that is not zero
    every = {c.name: c for c in g2}
    assert {c.failed for c in g2} >= {frozenset(s) for s in (["tag", "range", "curve", "subgroup"], ["subgroup"], ["curve"], ["range"], ["tag"])}
    assert every["tag4/x/y/off/inside"].failed == {"curve"} and every["tag4/x/y/on/outside"].status == 5
    assert W.in_subgroup(2, W.GEN[2]) and W.on_curve(2, W.GEN[2]) and W.on_curve(1, W.GEN[1]) and W.in_subgroup(1, W.GEN[1])
    x, y = W.g2_full_order_point()
    assert W.on_curve(2, (x, y)) and not W.in_subgroup(2, (x, y))


@pytest.mark.parametrize("g", [1, 2])
def test_decoders_model_against_oracle(oracle, g):
    dec = oracle.g1_decode if g == 1 else oracle.g2_decode
    for c in W.collision_cases(g):
        rc, out = dec(np.frombuffer(c.rec, np.uint8))
        assert rc == c.status, (c.name, rc, c.status)
        if rc == 0:
            assert canon_infinity(out).tobytes() == W.words(g, c.point).tobytes(), c.name


def test_fr_model_against_oracle(oracle):
    for name, rec, st, v in W.fr_cases():
        rc, out = oracle.fr_decode(np.frombuffer(rec, np.uint8))
        assert rc == st, name
        if st == 0:
            assert out.tobytes() == W.fr_words(v).tobytes() and bytes(oracle.fr_encode(out)) == rec == W.fr_encode(v), name


@pytest.mark.parametrize("g", [1, 2])
def test_encoders_model_against_oracle(oracle, g):
    enc, norm = (oracle.g1_encode, oracle.g1_normalize) if g == 1 else (oracle.g2_encode, oracle.g2_normalize)
    P, recs, normal = W.encode_batch(g, 24)
    assert (P[:, 2 * W.WORDS[g] // 3:] != normal[:, 2 * W.WORDS[g] // 3:]).any(axis=1).sum() >= 8           # Jacobian inputs with z != 1
    for i in range(P.shape[0]):
        assert bytes(enc(P[i])) == recs[i].tobytes(), i
        assert canon_infinity(norm(P[i])).tobytes() == normal[i].tobytes(), i
        st, pt = W.decode(g, recs[i])                                     # decode(encode(P)) == normalize(P) inside the model
        assert st == 0 and W.words(g, pt).tobytes() == normal[i].tobytes()


@pytest.mark.parametrize("g, fn", [(1, "hs_g1_decode"), (2, "hs_g2_decode"), (2, "hss_g2_decode")])
def test_decoder_bodies_under_gxx_against_model(hs, g, fn):
    """status AND output words: a rejected record is G::zero() = (0, 1, 0), tag 0 is infinity whatever its padding"""
    lib = HS.lib() if fn.startswith("hss") else hs.lib
    for c in W.collision_cases(g):
        rc, out = _dec(lib, fn, c.rec, W.WORDS[g])
        assert rc == c.status, (c.name, rc, c.status)
        assert out.tobytes() == W.words(g, c.point).tobytes(), c.name
    for p in W.valid_points(g):
        rc, out = _dec(lib, fn, W.encode(g, p), W.WORDS[g])
        assert rc == 0 and out.tobytes() == W.words(g, p).tobytes()


def test_fr_bodies_under_gxx_against_model(hs):
    for name, rec, st, v in W.fr_cases():
        rc, out = _dec(hs.lib, "hs_fr_decode", rec, 4)
        assert rc == st and out.tobytes() == W.fr_words(v).tobytes(), name            # a rejected record is Fr::zero()
        if st == 0:
            assert _enc(hs.lib, "hs_fr_encode", W.fr_words(v), 32).tobytes() == rec, name
    b, st, k = W.fr_batch(40)
    for i in range(40):
        rc, out = _dec(hs.lib, "hs_fr_decode", b[i], 4)
        assert rc == st[i] and out.tobytes() == k[i].tobytes(), i


@pytest.mark.parametrize("g, fn", [(1, "hs_g1_encode"), (2, "hs_g2_encode")])
def test_encoder_bodies_under_gxx_against_model(hs, g, fn):
    P, recs, _ = W.encode_batch(g, 24)
    for i in range(P.shape[0]):
        assert _enc(hs.lib, fn, P[i], W.RS[g]).tobytes() == recs[i].tobytes(), i


@pytest.mark.parametrize("g", [1, 2])
def test_the_stream_model_on_cases_written_out_by_hand(g):
    rs = W.RS[g]
    cases = {c.name: c for c in W.stream_cases(g)}
    assert len(cases) == len(W.stream_cases(g))
    want = {"empty": ((0, [], 0),) * 2, "lone 00": ((1, [0], 1),) * 2, "lone 04": ((0, [], 0),) * 2, "lone 09": ((1, [3], 1),) * 2,
            "one record cut at 1": ((0, [], 0),) * 2, f"one record cut at {rs - 1}": ((0, [], 0),) * 2,
            "second record cut at 33": ((1, [0], rs),) * 2, "00 00 04..": ((3, [0, 0, 0], rs + 2),) * 2, "00 00 04.. cut": ((2, [0, 0], 2),) * 2,
            "bad tag in the middle": ((5, [0, 3, 0, 0, 0], 3 * rs + 2), (2, [0, 3], rs + 1)),
            "off the curve in the middle": ((6, [0, 0, 4, 0, 3, 0], 4 * rs + 2), (3, [0, 0, 4], 2 * rs + 1)),
            "max_points=0 of 8": ((0, [], 0),) * 2, "max_points=3 of 8": ((3, [0, 0, 0], 2 * rs + 1),) * 2,
            "max_points=4 of 8": ((4, [0, 0, 0, 3], 2 * rs + 2),) * 2,
            "max_points=5 of 8": ((5, [0, 0, 0, 3, 0], 3 * rs + 2), (4, [0, 0, 0, 3], 2 * rs + 2)),
            "max_points=7 of 8": ((7, [0, 0, 0, 3, 0, 0, 4], 4 * rs + 3), (4, [0, 0, 0, 3], 2 * rs + 2)),
            "max_points=8 of 8": ((8, [0, 0, 0, 3, 0, 0, 4, 0], 5 * rs + 3), (4, [0, 0, 0, 3], 2 * rs + 2)),
            "max_points=9 of 8": ((8, [0, 0, 0, 3, 0, 0, 4, 0], 5 * rs + 3), (4, [0, 0, 0, 3], 2 * rs + 2)),
            "max_points=8 and a cut tail": ((8, [0, 0, 0, 3, 0, 0, 4, 0], 5 * rs + 3), (4, [0, 0, 0, 3], 2 * rs + 2))}
    for name, (default, stop) in want.items():
        assert cases[name].default[:3] == default and cases[name].stop[:3] == stop, name
    cuts = [c for c in cases.values() if "cut at" in c.name]
    assert len(cuts) == (2 * (rs - 1) if g == 1 else 14)
    for c in cuts:                                                        # a cut record is never consumed, in neither mode
        whole = rs if c.name.startswith("second") else 0
        assert c.default[:3] == c.stop[:3] == (whole // rs, [0] * (whole // rs), whole), c.name
    pts = list(W.valid_points(g)[:5]) + [None, None]
    data = W.stream_encode(g, [None] + pts)
    assert len(data) == 5 * rs + 3 and W.stream_decode(g, data) == (8, [0] * 8, len(data), [None] + pts)
