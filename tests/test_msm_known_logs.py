"""The expectation of the large MSM tests (tests/msm_known_logs.py) checked against the oracle on the CPU: a wrong expectation must not pass
for a kernel bug."""
import numpy as np
import pytest

import bn_model as M
import edge_inputs as E
import msm_known_logs as KL
from bn_oracle import FR
from test_gpu_msm_bucket import _want

R = M.R_ORD


@pytest.mark.parametrize("g", [1, 2])
def test_known_logs_against_the_oracle_fold(oracle, g):
    """n = 50 with every special term (a chunk of 32: the seam pair is in), a second call from the second start: [sum a_i k_i] G is the
    oracle's g*_mul_batch, g*_add in index order, g*_normalize over points the oracle makes itself"""
    n, chunk = 50, 32
    logs = KL.Logs(np.random.default_rng(3100 + g), n, starts=(0, 10), seams=(chunk,))
    a = logs.ints
    assert a[1] == 0 and a[11] == 0 and a[2] == a[3] and a[4] + a[5] == R and a[31] + a[32] == R
    one, mul = (oracle.g1_one, oracle.g1_mul_batch) if g == 1 else (oracle.g2_one, oracle.g2_mul_batch)
    P = mul(np.tile(one(), (n, 1)), E.fr(oracle, a))
    w = P.shape[1] // 3
    assert not P[1, 2 * w:].any() and P[0, 2 * w:].any()
    for lo, m, ch in ((0, n, chunk), (10, 22, chunk), (0, 32, chunk)):
        k, special = KL.draw_scalars(np.random.default_rng(3110 + g + lo + m), logs, lo, m, ch)
        ks = KL.to_ints(k)
        assert (ks[0], ks[6], ks[7], ks[-3], ks[-2], ks[-1]) == (R - 1, 0, 1, 1, 0, R - 1) and ks[4] == ks[5]
        assert {0, m - 1} <= set(special) and ((m <= ch) or ({ch - 1, ch} <= set(special) and ks[ch - 1] == ks[ch]))
        got = KL.expected(oracle, g, KL.host_sum(logs, lo, k))
        assert np.array_equal(got, _want(oracle, g, P[lo:lo + m], E.fr(oracle, ks))), (lo, m)
        assert got[2 * w:].any()                                        # a finite point


def test_wire_bytes_are_the_oracles_fr_encoding(oracle):
    """the records handed to fr_decode_batch: words -> 32 big-endian bytes, equal to the oracle's encoding of the value and decoded by it to
    the value's Montgomery row; to_words / to_ints are inverse to each other"""
    rng = np.random.default_rng(3120)
    vals = [0, 1, R - 1, 1 << 252, (1 << 253) - 1] + KL.to_ints(KL.draw(rng, 8))
    words = KL.to_words(vals)
    assert KL.to_ints(words) == vals and max(vals[5:]) < 1 << 253 and min(vals[5:]) > 1 << 200
    b = KL.wire(words)
    assert b.shape == (len(vals), 32) and b.dtype == np.uint8
    for i, v in enumerate(vals):
        row = oracle.fp_from_int(FR, v)
        assert bytes(b[i]) == v.to_bytes(32, "big") == bytes(oracle.fr_encode(row))
        rc, back = oracle.fr_decode(b[i])
        assert rc == 0 and np.array_equal(back, row)
