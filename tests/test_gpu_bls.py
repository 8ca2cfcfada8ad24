"""bn_amd.bls on an MI355X (run with -m gpu): sign and verify, the three ways a check must fail, a batch with one spoiled entry, aggregates over
distinct messages and over one message."""
import numpy as np
import pytest

import hash_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def keys():
    from bn_amd import Fr, bls
    rng = np.random.default_rng(2220)
    sks = [Fr.random(rng) for _ in range(70)]
    return sks, bls.public_keys(sks)


def test_sign_then_verify_and_the_three_ways_to_fail(keys):
    from bn_amd import G1, bls
    sks, pks = keys
    msg = b"\x42" * 32
    sig = bls.sign(sks[0], msg)
    assert np.array_equal(sig.limbs, (G1(HC.words(HC.hash_to_curve(msg, bls.DST))) * sks[0]).limbs)       # H(m) * sk, H from the model
    assert bls.verify(pks[0], msg, sig) is True
    flipped = bytes([msg[0] ^ 1]) + msg[1:]
    assert bls.verify(pks[0], flipped, sig) is False
    assert bls.verify(pks[1], msg, sig) is False
    assert bls.verify(pks[0], msg, -sig) is False
    assert bls.verify(pks[0], msg, sig, dst=b"another tag") is False


def test_keygen():
    from bn_amd import G2, bls
    sk, pk = bls.keygen(np.random.default_rng(1))
    assert pk == G2.one() * sk


def test_verify_batch_reports_exactly_the_spoiled_entry(keys):
    from bn_amd import bls
    sks, pks = keys
    msgs = HC.messages(70, 32, seed=3)
    sigs = bls.sign_batch(sks, msgs)
    assert bls.verify_batch(pks, msgs, sigs).all()
    spoiled = list(sigs); spoiled[41] = sigs[40]
    ok = bls.verify_batch(pks, msgs, spoiled)
    assert ok.dtype == bool and np.flatnonzero(~ok).tolist() == [41]
    mixed = [bytes([i]) * (1 + i % 5) for i in range(8)]                          # mixed lengths: the hashlib route, same bytes
    ok = bls.verify_batch(pks[:8], mixed, bls.sign_batch(sks[:8], mixed))
    assert ok.all()


def test_aggregates(keys):
    from bn_amd import bls
    sks, pks = keys
    msgs = [bytes([i]) * 32 for i in range(9)]
    sigs = bls.sign_batch(sks[:9], msgs)
    agg = bls.aggregate(sigs)
    assert bls.verify_aggregate(pks[:9], msgs, agg) is True
    assert bls.verify_aggregate(pks[:9], msgs[1:] + msgs[:1], agg) is False
    assert bls.verify_aggregate(pks[:9], msgs, bls.aggregate(sigs[:8])) is False
    with pytest.raises(ValueError, match="distinct messages"):
        bls.verify_aggregate(pks[:9], msgs[:8] + msgs[:1], agg)
    one = b"one message for everybody"
    same = bls.aggregate(bls.sign_batch(sks[:9], [one] * 9))
    assert bls.fast_aggregate_verify(pks[:9], one, same) is True
    assert bls.fast_aggregate_verify(pks[:8], one, same) is False
    assert bls.fast_aggregate_verify(pks[:9], b"another", same) is False
