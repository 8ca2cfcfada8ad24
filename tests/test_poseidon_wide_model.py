"""The wide Poseidon instance (t = 2 .. 17) in host integers, without a GPU: bn_amd.poseidon against the independent model of
tests/poseidon_wide_cases.py - constants, the validity of the Cauchy draw, the sixteen known answers (rows 6 and 16 are circomlibjs's published
values, rows 1 and 2 the answers the repository pinned before, every other row this project's own regression anchor), PoseidonEx and the
framing of the chain."""
import pytest

import poseidon_cases as PC
import poseidon_wide_cases as WC

R = WC.R


@pytest.mark.parametrize("t", range(2, 18))
def test_package_and_model_agree_on_the_constants_and_the_first_cauchy_draw_is_valid(t):
    from bn_amd import poseidon
    assert poseidon.R_F == WC.FULL and poseidon.R_P[t] == WC.PARTIAL[t]
    C, M = poseidon.constants(t)
    mC, mM, xs, ys = WC.constants(t)
    assert len(C) == (8 + WC.PARTIAL[t]) * t and list(C) == mC
    assert [list(r) for r in M] == mM
    assert all(c < R for c in C)
    assert len(set(xs + ys)) == 2 * t, "the matrix draws are not distinct"
    assert all((x + y) % R for x in xs for y in ys), "a sum of the matrix draws is zero"
    assert all(M[i][j] * (xs[i] + ys[j]) % R == 1 for i in range(t) for j in range(t))


def test_the_partial_round_counts_are_circomlibs_list():
    from bn_amd import poseidon
    assert [poseidon.R_P[t] for t in range(2, 18)] == [56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68]
    assert sorted(poseidon.R_P) == list(range(2, 18))
    assert {t: WC.PARTIAL[t] for t in PC.PARTIAL} == PC.PARTIAL                                  # the narrow widths did not move


@pytest.mark.parametrize("n", range(1, 17))
def test_the_sixteen_answers_come_out_of_both(n):
    from bn_amd import poseidon
    x = list(range(1, n + 1))
    assert WC.permute([0] + x)[0] == WC.KNOWN[n]
    assert poseidon.permute_host([0] + x)[0] == WC.KNOWN[n]
    assert poseidon.hash_ex_host(x) == [WC.KNOWN[n]]


def test_the_anchors_are_what_the_older_tests_pin():
    assert set(WC.EXTERNAL) == {6, 16} and set(WC.PINNED_BEFORE) == {1, 2}
    for n in (1, 2, 3, 4):
        assert WC.KNOWN[n] == PC.KNOWN_HASH[tuple(range(1, n + 1))]


def test_hash_ex_is_the_hash_and_the_permutation():
    from bn_amd import poseidon
    for n in range(1, 5):
        for x in WC.ex_rows(n, 5, 100 + n):
            assert poseidon.hash_ex_host(x) == [poseidon.hash_host(x)] == [PC.hash_(x)]
    for n in (1, 5, 16):
        x = WC.values(n, 7)
        init = WC.values(1, 8)[0]
        full = poseidon.hash_ex_host(x, init=init, n_outs=n + 1)
        assert full == poseidon.permute_host([init] + x) == WC.permute([init] + x)
        assert poseidon.hash_ex_host(x, init=init, n_outs=2) == full[:2] == WC.hash_ex(x, init, 2)
        assert poseidon.hash_ex_host(x, init=init) != poseidon.hash_ex_host(x)


@pytest.mark.parametrize("rate", [1, 2, 5, 16])
def test_the_framing_of_the_chain(rate):
    from bn_amd import poseidon
    for L in WC.chain_lengths(rate):
        v = WC.values(L, 40 + L)
        want = WC.hash_chain(v, rate)
        assert poseidon.hash_chain_host(v, rate) == want
        assert poseidon.chain_blocks(L, rate) == WC.blocks(L, rate) == max(1, -(-L // rate))
        # by hand: the length, then block after block through element 0
        c, padded = L, v + [0] * (WC.blocks(L, rate) * rate - L)
        for at in range(0, len(padded), rate):
            c = WC.permute([c] + padded[at:at + rate])[0]
        assert c == want
        assert poseidon.hash_chain_host(v + [0], rate) != want, "a trailing zero must change the digest: the length is absorbed"
    assert poseidon.hash_chain_host([], rate) == WC.permute([0] * (rate + 1))[0]                 # an empty record: one block of zeros under c = 0
    one = WC.values(1, 3)
    assert poseidon.hash_chain_host(one, rate) == WC.hash_ex(one + [0] * (rate - 1), init=1)[0]


def test_the_public_hash_did_not_grow():
    from bn_amd import poseidon
    assert poseidon.ARITY_MAX == 4 and poseidon.EX_INPUTS_MAX == 16
    with pytest.raises(ValueError, match="1 .. 4 inputs, not 5"):
        poseidon.hash_host([1, 2, 3, 4, 5])
    with pytest.raises(ValueError, match="1 .. 16 inputs, not 17"):
        poseidon.hash_ex_host([1] * 17)
    with pytest.raises(ValueError, match="1 .. 16 inputs, not 0"):
        poseidon.hash_ex_host([])
    with pytest.raises(ValueError, match="n_outs = 4: 1 .. 3 for 2 inputs"):
        poseidon.hash_ex_host([1, 2], n_outs=4)
    with pytest.raises(ValueError, match="n_outs = 0"):
        poseidon.hash_ex_host([1, 2], n_outs=0)
    for rate in (0, 17):
        with pytest.raises(ValueError, match="rate = %d: 1 .. 16" % rate):
            poseidon.hash_chain_host([1], rate)
    with pytest.raises(ValueError, match="t = 18: 2 .. 17 are defined"):
        poseidon.constants(18)
    with pytest.raises(ValueError, match="t = 1: 2 .. 17 are defined"):
        poseidon.constants(1)
