"""The device bodies of hash-to-curve for G2 on the CPU (tests/hostsim/hostsim_hash_g2.cpp: hash_g2_ops.hpp compiled with g++ -DBN_BOUNDS, so
the lazy-limb bounds are enforced through the field reduction, the five chains of the map, the double-and-add chain of [u]P, psi and its powers,
the four additions and the normalisation) against the integer model of hash_g2_cases.py, SHA-256 included.  Neither side is checked against
gnark-crypto or any other library."""
import random

import numpy as np

import bn_model as M
import hash_g2_cases as HC
import hostsim_hash_g2_lib as HS
from hash_cases import expand_message_xmd

Q = M.Q


def test_field_elements_from_96_bytes_and_sgn0():
    rng = random.Random(40)
    halves = [0, 1, 2, Q - 1, Q, Q + 1, 2 * Q, 6 * Q - 1, (1 << 256) - 1, 1 << 256, (1 << 256) + Q, 1 << 383, (1 << 384) - 1]
    pairs = [u for _, u in HC.u_cases()] + [(a, b) for a in halves for b in halves[:6]] + [(rng.getrandbits(384), rng.getrandbits(384)) for _ in range(60)]
    for c0, c1 in pairs:
        assert HS.field(c0, c1) == ((c0 % Q, c1 % Q), HC.sgn0((c0, c1))), (hex(c0), hex(c1))
    assert {HS.field(0, 3)[1], HS.field(Q, 2 * Q + 1)[1], HS.field(1, 0)[1]} == {1} and HS.field(2, 1)[1] == 0 and HS.field(0, 2)[1] == 0


def test_inv0_and_is_square_through_the_norm():
    rng = random.Random(41)
    assert HS.inv0((0, 0)) == ((0, 0), True)
    seen = set()
    for a in [(1, 0), (0, 1), (Q - 1, 0), (0, Q - 1), (2, 0), (9, 1)] + [(rng.randrange(Q), rng.randrange(Q)) for _ in range(24)]:
        inv, sq = HS.inv0(a)
        assert M.f2_mul(inv, a) == (1, 0) and sq == HC.is_square(a), a
        seen.add(sq)
    assert seen == {True, False}


def test_map_to_curve_cases_and_random_inputs():
    cases = HC.u_cases()
    got = HS.map_to_curve(HC.u_bytes([u for _, u in cases]))
    for (name, u), row in zip(cases, got):
        assert np.array_equal(row, HC.words(HC.map_to_curve(u))), name
    rng = random.Random(42)
    us = [(rng.getrandbits(384), rng.getrandbits(384)) for _ in range(60)]
    got = HS.map_to_curve(HC.u_bytes(us))
    branches = set()
    for u, row in zip(us, got):
        pt, br, _ = HC.map_branch(u)
        assert np.array_equal(row, HC.words(pt)), u
        branches.add(br)
    assert branches == {1, 2, 3}


def test_psi_and_its_powers_on_jacobian_coordinates():
    for _, pt, _ in HC.clear_cases()[:3] + HC.clear_cases()[8:10] + HC.clear_cases()[-4:-3]:
        want = pt
        for j in (1, 2, 3):
            want = HC.psi(want)
            got = HS.psi(j, HC.jac_words(pt))
            assert HC.affine_of(got) == HC.aff(want), j
            assert M.from_mont_limbs(got[16:20]) == want[2][0] and M.from_mont_limbs(got[20:24]) == want[2][1]      # Z itself: conj^j


def test_clear_cofactor_on_mapped_points_g2_points_and_infinity():
    pts, want = HC.clear_batch(len(HC.clear_cases()))
    got = HS.clear_cofactor(pts)
    for (name, _, _), g, w in zip(HC.clear_cases(), got, want):
        assert np.array_equal(g, w), name
    assert np.array_equal(HS.clear_cofactor(pts, in_place=True), want)
    zero = HC.words(None)
    assert all(np.array_equal(g, zero) for (n, _, c), g in zip(HC.clear_cases(), got) if c is None) and sum(c is None for _, _, c in HC.clear_cases()) == 3
    # on G2 the clearing is the scalar k; off it, the result has order r
    rng = random.Random(43)
    ks = [rng.randrange(1, M.R_ORD) for _ in range(4)]
    qs = [M.g_mul(M.FQ2_OPS, M.G2_ONE, kk) for kk in ks]
    got = HS.clear_cofactor(np.stack([HC.jac_words(q) for q in qs]))
    for kk, row in zip(ks, got):
        assert np.array_equal(row, HC.words(HC.aff(M.g_mul(M.FQ2_OPS, M.G2_ONE, kk * HC.CLEAR_K % M.R_ORD)))), kk
    # one more mapped point, checked by the r-fold sum alone: outside G2 before, inside after
    p = HC.jac(HC.map_to_curve((11, 13)))
    assert HC.in_g2(HC.affine_of(HS.clear_cofactor(HC.jac_words(p))[0])) and not HC.in_g2(HC.aff(p))


def test_hash_to_curve_from_uniform_bytes():
    cases = HC.uniform_cases()
    got = HS.hash_uniform(np.stack([np.frombuffer(b, np.uint8) for _, b in cases]))
    for (name, b), row in zip(cases, got):
        assert np.array_equal(row, HC.words(HC.hash_uniform(b))), name
    rng = random.Random(44)
    rows = [rng.getrandbits(1536).to_bytes(192, "big") for _ in range(24)]
    got = HS.hash_uniform(np.stack([np.frombuffer(b, np.uint8) for b in rows]))
    for b, row in zip(rows, got):
        assert np.array_equal(row, HC.words(HC.hash_uniform(b))), b.hex()


def test_expand_message_xmd_to_192_bytes_at_every_seam():
    for dl in HC.DST_LENS:
        dst = HC.dst_of(dl)
        for ml in HC.msg_lens(dl) + [100, 191, 300]:
            msg = HC.messages(1, ml, dl)[0].tobytes()
            assert HS.expand(msg, dst) == expand_message_xmd(msg, dst, 192), (dl, ml)
    quux = b"QUUX-V01-CS02-with-expander-SHA256-128"
    for msg in (b"", b"abc", b"abcdef0123456789", b"q128_" + b"q" * 128, b"a512_" + b"a" * 512):
        assert HS.expand(msg, quux) == expand_message_xmd(msg, quux, 192)
    # RFC 9380 appendix K.1 lists the 128-byte expansions; 192 bytes has no vector there.  The first block of an expansion depends on the
    # length, so the 96-byte instance (pinned by the G1 tests) and this one share no prefix
    assert HS.expand(b"abc", quux)[:32] != expand_message_xmd(b"abc", quux, 96)[:32]
    rng = random.Random(46)
    for _ in range(100):
        msg = rng.randbytes(rng.randrange(0, 200)); dst = rng.randbytes(rng.randrange(1, 256))
        assert HS.expand(msg, dst) == expand_message_xmd(msg, dst, 192), (len(msg), len(dst))


def test_hash_to_curve_from_messages():
    for dst, msgs, uniform, points in HC.message_cases():
        got = HS.hash_msgs(msgs, dst)
        assert np.array_equal(got, points), (len(dst), msgs.shape)
        assert np.array_equal(got, HS.hash_uniform(uniform))
    bls = HS.hash_msgs(np.frombuffer(b"\x11" * 32, np.uint8).reshape(1, 32), HC.BLS_G2_DST)
    assert np.array_equal(bls[0], HC.words(HC.hash_to_curve(b"\x11" * 32, HC.BLS_G2_DST)))
