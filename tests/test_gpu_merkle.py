"""bn_amd.merkle on an MI355X (run with -m gpu): a tree over 2^8 leaves, openings, verify in host integers and verify_batch on the GPU, against
the integer model of tests/poseidon_cases.py."""
import pytest

import poseidon_cases as PC

pytestmark = pytest.mark.gpu
INDICES = [0, 1, 127, 255]


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def built(eng):
    from bn_amd import Fr, merkle
    vals = (PC.EDGE + PC.values(256, 81))[:256]
    tree = merkle.Tree([Fr(v) for v in vals], engine=eng)
    return vals, PC.tree(vals), tree


def test_the_tree_is_the_models(built):
    vals, nodes, tree = built
    assert tree.depth == 8 and [x.v for x in tree.nodes] == nodes and tree.root.v == nodes[-1]


@pytest.mark.parametrize("i", INDICES)
def test_open_and_verify(built, i):
    from bn_amd import Fr, merkle
    vals, nodes, tree = built
    path = tree.open(i)
    assert [x.v for x in path] == PC.path(vals, nodes, i)
    assert merkle.verify(tree.root, Fr(vals[i]), i, path)
    assert not merkle.verify(tree.root, Fr(vals[i]), i ^ 1, path) and not merkle.verify(tree.root, Fr(vals[i] + 1), i, path)


def test_verify_batch_accepts_the_openings_and_reports_each_spoiled_one(built, eng):
    from bn_amd import Fr, merkle
    vals, nodes, tree = built
    leaves = [Fr(vals[i]) for i in INDICES]
    paths = [tree.open(i) for i in INDICES]
    assert merkle.verify_batch(tree.root, leaves, INDICES, paths, engine=eng) == [True] * 4
    flipped = [list(p) for p in paths]
    flipped[1][3] = flipped[1][3] + Fr.one()                                                     # a sibling of opening 1
    assert merkle.verify_batch(tree.root, leaves, INDICES, flipped, engine=eng) == [True, False, True, True]
    assert merkle.verify_batch(tree.root, leaves, [0, 1, 126, 255], paths, engine=eng) == [True, True, False, True]          # a wrong index
    wrong = list(leaves); wrong[3] = wrong[3] + Fr.one()
    assert merkle.verify_batch(tree.root, wrong, INDICES, paths, engine=eng) == [True, True, True, False]                   # a wrong leaf
    assert merkle.verify_batch(tree.root, [leaves[0]], [256], [paths[0]], engine=eng) == [False]                            # outside the tree
