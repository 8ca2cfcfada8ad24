"""The bodies of bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch and bn254_fr_merkle_tree (bn_amd/csrc/poseidon_ops.hpp) and the levels of a
tree (host_plan.hpp bn_merkle_plan) on the CPU: tests/hostsim/hostsim_poseidon.cpp runs the kernels' own code over host arrays, in the
bound-enforcing build, against the integer model of tests/poseidon_cases.py - byte for byte.  Both variants of the matrix row run: the plain one
and the product-sum fr_dot of fr.hpp, whose bounds (a violated one aborts) are also driven to their edge: every operand r - 1, five pairs."""
import numpy as np
import pytest

import fr_cases as FC
import hostsim_poseidon_lib as HP
import poseidon_cases as PC

R = FC.R
VARIANTS = [False, True]


def _same(got, want):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), np.nonzero((got != want).any(axis=1))[0][:8]


@pytest.fixture(scope="module")
def want_states():
    """per width: the states (edge inputs in every position, then random ones: 64 random states) and the model's permutations - computed once"""
    out = {}
    for t in (2, 3, 4, 5):
        states = PC.states(t, 4 + 4 * t + 64, 100 + t)
        out[t] = (states, [PC.permute(s) for s in states])
    return out


@pytest.mark.parametrize("fused", VARIANTS)
@pytest.mark.parametrize("t", [2, 3, 4, 5])
def test_permute_equals_the_model_out_of_place_and_in_place(want_states, t, fused):
    states, want = want_states[t]
    got, launches = HP.permute(states, fused=fused)
    _same(got, PC.rows(want))
    assert launches == 1
    got, launches = HP.permute(states, step=7, in_place=True, fused=fused)
    _same(got, PC.rows(want))
    assert launches == -(-len(states) // 7)


@pytest.mark.parametrize("fused", VARIANTS)
@pytest.mark.parametrize("arity", [1, 2, 3, 4])
def test_hash_equals_the_model_and_the_known_answer(arity, fused):
    inputs = PC.hash_inputs(arity, 1 + 4 + 4 * arity + 8, 200 + arity)
    want = [PC.hash_(x) for x in inputs]
    assert want[0] == PC.KNOWN_HASH[tuple(range(1, arity + 1))]
    got, launches = HP.hash_(inputs, step=5, fused=fused)
    _same(got, FC.rows(want))
    assert launches == -(-len(inputs) // 5)


@pytest.mark.parametrize("fused", VARIANTS)
def test_the_known_hashes_of_arity_two(fused):
    inputs = [[0, 0], [R - 1, R - 1], [1, 2]]
    _same(HP.hash_(inputs, fused=fused)[0], FC.rows([PC.KNOWN_HASH[tuple(x)] for x in inputs]))
    _same(HP.permute([[0, 1, 2]], fused=fused)[0][1:2], FC.rows([PC.KNOWN_PERMUTE_012_1]))


@pytest.mark.parametrize("fused", VARIANTS)
@pytest.mark.parametrize("log_n, step", [(0, 1 << 22), (1, 1 << 22), (3, 1 << 22), (6, 1 << 22), (6, 5)])
def test_trees(log_n, step, fused):
    leaves = list(range(8)) if log_n == 3 else (PC.EDGE + PC.values(1 << log_n, 300 + log_n))[:1 << log_n]
    want = PC.tree(leaves)
    got, launches = HP.merkle(leaves, step=step, fused=fused)
    _same(got, FC.rows(want))
    assert launches == sum(-(-(1 << l) // step) for l in range(log_n))
    if log_n == 3:
        assert want[-1] == PC.KNOWN_ROOT_8


def test_the_product_sum_holds_its_bounds_at_the_edge():
    """every operand r - 1 and T = 5: the largest sum of products there is, 5 (r - 1)^2; then every T with edge and random operands"""
    for T in (1, 2, 3, 4, 5):
        a, b = [R - 1] * T, [R - 1] * T
        assert HP.dot(a, b).tobytes() == FC.rows([T % R]).tobytes()                  # (r - 1)^2 = 1 mod r
    top = (R - 1) * pow(FC.MONT, -1, R) % R                                           # the value whose Montgomery IMAGE is r - 1: the largest words
    assert FC.rows([top])[0].tolist() == [(R - 1) >> (64 * j) & (2**64 - 1) for j in range(4)]
    for T in (1, 2, 3, 4, 5):
        assert HP.dot([top] * T, [top] * T).tobytes() == FC.rows([T * top * top % R]).tobytes()
    rng = np.random.default_rng(9)
    for T in (1, 2, 3, 4, 5):
        for _ in range(40):
            a = [PC.EDGE[int(rng.integers(4))] if rng.integers(3) == 0 else FC.rand(rng) for _ in range(T)]
            b = [PC.EDGE[int(rng.integers(4))] if rng.integers(3) == 0 else FC.rand(rng) for _ in range(T)]
            assert HP.dot(a, b).tobytes() == FC.rows([sum(x * y for x, y in zip(a, b)) % R]).tobytes()
