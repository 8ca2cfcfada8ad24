"""The device bodies of hash-to-curve for G1 on the CPU (tests/hostsim/hostsim_hash.cpp: hash_ops.hpp compiled with g++ -DBN_BOUNDS, so the
lazy-limb bounds are enforced through the field reduction, both forms of inv0, the four chains of the map, the addition and the normalisation)
against the integer model of hash_cases.py, SHA-256 included."""
import random

import numpy as np
import pytest

import bn_model as M
import hash_cases as HC
import hostsim_hash_lib as HS

Q = M.Q
FORMS = [0, 1]


def test_field_elements_from_48_bytes():
    rng = random.Random(30)
    vs = [u for _, u in HC.u_cases()] + [0, 1, Q - 1, Q, 2 * Q, 5 * Q, 6 * Q - 1, (1 << 256) - 1, 1 << 256, (1 << 256) + Q, 1 << 383, (1 << 384) - 1]
    vs += [rng.getrandbits(384) for _ in range(200)] + [rng.getrandbits(256) << 128 for _ in range(8)] + [((1 << 128) - 1) << 256 | rng.getrandbits(256) for _ in range(8)]
    for v in vs:
        assert HS.field(v) == v % Q, hex(v)


@pytest.mark.parametrize("form", FORMS)
def test_inv0(form):
    rng = random.Random(31)
    assert HS.inv0(0, form) == 0
    for a in [1, 2, Q - 1, Q - 2] + [rng.randrange(1, Q) for _ in range(24)]:
        assert HS.inv0(a, form) * a % Q == 1, a


@pytest.mark.parametrize("form", FORMS)
def test_map_to_curve_cases_and_random_inputs(form):
    cases = HC.u_cases()
    got = HS.map_to_curve(HC.u_bytes([u for _, u in cases]), form)
    for (name, u), row in zip(cases, got):
        assert np.array_equal(row, HC.words(HC.map_to_curve(u))), name
    rng = random.Random(32 + form)
    us = [rng.getrandbits(384) for _ in range(300)]
    got = HS.map_to_curve(HC.u_bytes(us), form)
    branches = set()
    for u, row in zip(us, got):
        pt, br, _ = HC.map_branch(u)
        assert np.array_equal(row, HC.words(pt)), hex(u)
        branches.add(br)
    assert branches == {1, 2, 3}


@pytest.mark.parametrize("form", FORMS)
def test_hash_to_curve_from_uniform_bytes(form):
    cases = HC.uniform_cases()
    got = HS.hash_uniform(np.stack([np.frombuffer(b, np.uint8) for _, b in cases]), form)
    for (name, b), row in zip(cases, got):
        assert np.array_equal(row, HC.words(HC.hash_uniform(b))), name
    rng = random.Random(34 + form)
    rows = [rng.getrandbits(768).to_bytes(96, "big") for _ in range(200)]
    got = HS.hash_uniform(np.stack([np.frombuffer(b, np.uint8) for b in rows]), form)
    for b, row in zip(rows, got):
        assert np.array_equal(row, HC.words(HC.hash_uniform(b))), b.hex()


def test_expand_message_xmd_at_every_seam():
    for dl in HC.DST_LENS:
        dst = HC.dst_of(dl)
        for ml in HC.msg_lens(dl) + [100, 191, 300]:
            msg = HC.messages(1, ml, dl)[0].tobytes()
            assert HS.expand(msg, dst) == HC.expand_message_xmd(msg, dst, 96), (dl, ml)
    quux = b"QUUX-V01-CS02-with-expander-SHA256-128"
    for msg in (b"", b"abc", b"abcdef0123456789", b"q128_" + b"q" * 128, b"a512_" + b"a" * 512):
        assert HS.expand(msg, quux) == HC.expand_message_xmd(msg, quux, 96)
    rng = random.Random(36)
    for _ in range(200):
        msg = rng.randbytes(rng.randrange(0, 200)); dst = rng.randbytes(rng.randrange(1, 256))
        assert HS.expand(msg, dst) == HC.expand_message_xmd(msg, dst, 96), (len(msg), len(dst))


@pytest.mark.parametrize("form", FORMS)
def test_hash_to_curve_from_messages(form):
    for dst, msgs, uniform, points in HC.message_cases():
        got = HS.hash_msgs(msgs, dst, form)
        assert np.array_equal(got, points), (len(dst), msgs.shape)
        assert np.array_equal(got, HS.hash_uniform(uniform, form))
    rng = random.Random(38 + form)
    for _ in range(40):
        ml = rng.randrange(0, 120); dst = rng.randbytes(rng.randrange(1, 256))
        msgs = np.frombuffer(rng.randbytes(5 * ml), np.uint8).reshape(5, ml)
        want = np.stack([HC.words(HC.hash_to_curve(m.tobytes(), dst)) for m in msgs])
        assert np.array_equal(HS.hash_msgs(msgs, dst, form), want), (ml, len(dst))
    bls = HS.hash_msgs(np.frombuffer(b"\x11" * 32, np.uint8).reshape(1, 32), HC.BLS_DST, form)
    assert np.array_equal(bls[0], HC.words(HC.hash_to_curve(b"\x11" * 32, HC.BLS_DST)))
