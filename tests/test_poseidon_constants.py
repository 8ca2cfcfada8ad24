"""The constants of Poseidon over Fr without a GPU: the Grain derivation of bn_amd/poseidon.py (the single source; the header
bn_amd/csrc/poseidon_constants.hpp is generated from it) against the independent integer model of tests/poseidon_cases.py at all four widths,
both against the known answers - circomlib's published hashes among them -, the first-attempt matrix draw, and the committed header."""
import pathlib
import subprocess
import sys

import pytest

import poseidon_cases as PC

ROOT = pathlib.Path(__file__).resolve().parents[1]
R = PC.R
WIDTHS = [2, 3, 4, 5]


@pytest.mark.parametrize("t", WIDTHS)
def test_the_package_and_the_model_derive_the_same_constants(t):
    from bn_amd import poseidon
    C, M = poseidon.constants(t)
    mC, mM, xs, ys = PC.constants(t)
    assert poseidon.R_F == PC.FULL and poseidon.R_P[t] == PC.PARTIAL[t]
    assert list(C) == mC and len(C) == (8 + PC.PARTIAL[t]) * t and all(0 <= c < R for c in C)
    assert [list(row) for row in M] == mM
    for i in range(t):
        for j in range(t):
            assert M[i][j] * (xs[i] + ys[j]) % R == 1


@pytest.mark.parametrize("t", WIDTHS)
def test_the_first_matrix_draw_is_distinct_and_has_no_zero_sum(t):
    _, _, xs, ys = PC.constants(t)
    assert len(set(xs + ys)) == 2 * t
    assert all((x + y) % R for x in xs for y in ys)


def test_the_known_constants():
    from bn_amd import poseidon
    for C, M in (poseidon.constants(3), PC.constants(3)[:2]):
        assert (C[0], C[194], M[0][0], M[2][2]) == (PC.KNOWN_T3["C0"], PC.KNOWN_T3["C194"], PC.KNOWN_T3["M00"], PC.KNOWN_T3["M22"])
    for t, (index, head, tail) in PC.KNOWN_LAST.items():
        for C in (poseidon.constants(t)[0], PC.constants(t)[0]):
            assert len(C) == index + 1
            digits = "%064x" % C[index]
            assert digits.startswith(head) and digits.endswith(tail), (t, digits)


def test_the_known_hashes_permutation_and_root():
    from bn_amd import poseidon
    for inputs, want in PC.KNOWN_HASH.items():
        assert PC.hash_(inputs) == want and poseidon.hash_host(inputs) == want, inputs
    assert PC.permute([0, 1, 2])[1] == PC.KNOWN_PERMUTE_012_1 == poseidon.permute_host([0, 1, 2])[1]
    assert PC.tree(list(range(8)))[-1] == PC.KNOWN_ROOT_8
    level = list(range(8))
    while len(level) > 1:
        level = [poseidon.hash_host(level[i:i + 2]) for i in range(0, len(level), 2)]
    assert level == [PC.KNOWN_ROOT_8]


@pytest.mark.parametrize("t", WIDTHS)
def test_the_two_permutations_agree_on_the_edge_inputs(t):
    from bn_amd import poseidon
    for s in PC.states(t, 4 + 4 * t + 4, 900 + t):
        assert poseidon.permute_host(s) == PC.permute(s)


def test_the_committed_header_is_current():
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_poseidon_constants.py"), "--check"], capture_output=True, text=True)
    assert p.returncode == 0 and "up to date" in p.stdout, p.stdout + p.stderr
    other = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_poseidon_constants.py"), "--check", str(ROOT / "README.md")], capture_output=True, text=True)
    assert other.returncode == 1 and "stale" in other.stdout                                    # the check does tell a difference, and writes nothing
