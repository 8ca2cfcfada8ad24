"""bn_amd.bls_minpk on an MI355X (run with -m gpu): keys in G1, signatures in G2 - sign and verify, the ways a check must fail, a batch with one
spoiled entry, aggregates over distinct messages and over one message."""
import numpy as np
import pytest

import hash_g2_cases as HC

pytestmark = pytest.mark.gpu
N = 8


@pytest.fixture(scope="module")
def keys():
    from bn_amd import Fr, bls_minpk
    rng = np.random.default_rng(2320)
    sks = [Fr.random(rng) for _ in range(N)]
    return sks, bls_minpk.public_keys(sks)


def test_sign_then_verify_and_the_ways_to_fail(keys):
    from bn_amd import G1, G2, bls_minpk as bls
    sks, pks = keys
    assert pks[0] == G1.one() * sks[0]
    msg = b"\x42" * 32
    sig = bls.sign(sks[0], msg)
    assert np.array_equal(sig.limbs, (G2(HC.words(HC.hash_to_curve(msg, bls.DST))) * sks[0]).limbs)       # H(m) * sk, H from the model
    assert bls.verify(pks[0], msg, sig) is True
    flipped = bytes([msg[0] ^ 1]) + msg[1:]
    assert bls.verify(pks[0], flipped, sig) is False                             # a flipped message bit
    assert bls.verify(pks[1], msg, sig) is False                                 # another key
    flipped_key = G1(pks[0].limbs.copy()); flipped_key.limbs[4] ^= np.uint64(1)  # a flipped bit of the key's y: not even on the curve
    assert bls.verify(flipped_key, msg, sig) is False
    assert bls.verify(pks[0], msg, -sig) is False
    assert bls.verify(pks[0], msg, sig, dst=b"another tag") is False


def test_keygen():
    from bn_amd import G1, bls_minpk as bls
    sk, pk = bls.keygen(np.random.default_rng(1))
    assert pk == G1.one() * sk


def test_verify_batch_reports_exactly_the_spoiled_entry(keys):
    from bn_amd import bls_minpk as bls
    sks, pks = keys
    msgs = HC.messages(N, 32, seed=3)
    sigs = bls.sign_batch(sks, msgs)
    assert bls.verify_batch(pks, msgs, sigs).all()
    spoiled = list(sigs); spoiled[5] = sigs[4]
    ok = bls.verify_batch(pks, msgs, spoiled)
    assert ok.dtype == bool and np.flatnonzero(~ok).tolist() == [5]
    bad = msgs.copy(); bad[2, 7] ^= 0x10
    assert np.flatnonzero(~bls.verify_batch(pks, bad, sigs)).tolist() == [2]
    mixed = [bytes([i]) * (1 + i % 5) for i in range(N)]                          # mixed lengths: the hashlib route, same bytes
    assert bls.verify_batch(pks, mixed, bls.sign_batch(sks, mixed)).all()


def test_aggregates(keys):
    from bn_amd import bls_minpk as bls
    sks, pks = keys
    msgs = [bytes([i]) * 32 for i in range(N)]
    sigs = bls.sign_batch(sks, msgs)
    agg = bls.aggregate(sigs)
    assert bls.verify_aggregate(pks, msgs, agg) is True
    assert bls.verify_aggregate(pks, msgs[1:] + msgs[:1], agg) is False
    assert bls.verify_aggregate(pks, msgs, bls.aggregate(sigs[:N - 1])) is False
    with pytest.raises(ValueError, match="distinct messages"):
        bls.verify_aggregate(pks, msgs[:N - 1] + msgs[:1], agg)
    one = b"one message for everybody"
    same = bls.aggregate(bls.sign_batch(sks, [one] * N))
    assert bls.fast_aggregate_verify(pks, one, same) is True
    assert bls.fast_aggregate_verify(pks[:N - 1], one, same) is False
    assert bls.fast_aggregate_verify(pks, b"another", same) is False
