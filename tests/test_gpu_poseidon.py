"""Poseidon hashes and Merkle trees over Fr on an MI355X (run with -m gpu): bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch,
bn254_fr_merkle_tree, their _dev entry points and the Python faces.  The model is Python integers (tests/poseidon_cases.py, written
independently of bn_amd/poseidon.py): the expected bytes are the limbs of v * 2^256 mod r - byte equality, no tolerance.  The sizes are the
seams of a wave (63, 64, 65) and of a block (257), one lane, and a seam between two sub-launches reached through the library's internal
hook, as the other Fr families reach theirs."""
import ctypes as C
import threading

import numpy as np
import pytest

import fr_cases as FC
import poseidon_cases as PC

pytestmark = pytest.mark.gpu
R = FC.R
SIZES = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_poseidon_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def hashes():
    """per arity: 257 input rows (the known-answer input first, the edge inputs in every position, random rows) and the model's hashes -
    computed once, never changed; a size takes the first n rows"""
    out = {}
    for arity in (1, 2, 3, 4):
        inputs = PC.hash_inputs(arity, max(SIZES), 500 + arity)
        out[arity] = (inputs, [PC.hash_(x) for x in inputs])
    return out


@pytest.fixture(scope="module")
def permutations():
    out = {}
    for t in (2, 3, 4, 5):
        states = PC.states(t, 65, 600 + t)
        out[t] = (states, [PC.permute(s) for s in states])
    return out


@pytest.fixture(scope="module")
def trees():
    """leaves and the model's nodes per log_n; 3 is the tree over 0 .. 7 of the known root"""
    out = {}
    for log_n in (0, 1, 2, 3, 9, 11):
        leaves = list(range(8)) if log_n == 3 else (PC.EDGE + PC.values(1 << log_n, 700 + log_n))[:1 << log_n]
        out[log_n] = (leaves, PC.tree(leaves))
    return out


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    assert got.tobytes() == want.tobytes(), np.nonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))[0][:8]


def _limbs(rows_of_ints):
    return PC.rows(rows_of_ints).reshape(len(rows_of_ints), -1, 4)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1).copy()).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("arity", [1, 2, 3, 4])
def test_hashes_against_the_model(eng, hashes, arity, n):
    inputs, want = hashes[arity]
    assert want[0] == PC.KNOWN_HASH[tuple(range(1, arity + 1))]
    X = _limbs(inputs[:n])
    _same(eng.fr_poseidon_batch(X), FC.rows(want[:n]))
    assert X.tobytes() == _limbs(inputs[:n]).tobytes()


def test_the_known_answers_of_arity_two(eng):
    inputs = [[0, 0], [R - 1, R - 1], [1, 2]]
    _same(eng.fr_poseidon_batch(_limbs(inputs)), FC.rows([PC.KNOWN_HASH[tuple(x)] for x in inputs]))
    _same(eng.fr_poseidon_permute_batch(_limbs([[0, 1, 2]]))[0, 1:2], FC.rows([PC.KNOWN_PERMUTE_012_1]))


@pytest.mark.parametrize("t", [2, 3, 4, 5])
def test_permute_out_of_place_and_in_place(eng, permutations, t):
    import torch
    states, want = permutations[t]
    W = PC.rows(want)
    _same(eng.fr_poseidon_permute_batch(_limbs(states)).reshape(-1, 4), W)
    stream = torch.cuda.Stream()
    d_in, d_io = _dev(_limbs(states)), _dev(_limbs(states))
    out = torch.zeros(len(states) * t * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        eng.fr_poseidon_permute_batch_dev(d_in.data_ptr(), t, out.data_ptr(), len(states), stream=stream.cuda_stream)
        eng.fr_poseidon_permute_batch_dev(d_io.data_ptr(), t, d_io.data_ptr(), len(states), stream=stream.cuda_stream)
    stream.synchronize()
    _same(_host(out), W)
    _same(_host(d_io), W)
    assert _host(d_in).tobytes() == PC.rows(states).tobytes()


@pytest.mark.parametrize("arity", [1, 2, 3, 4])
def test_the_dev_form_agrees_with_the_host_buffer_form(eng, hashes, arity):
    import torch
    inputs, want = hashes[arity]
    n = 65
    stream = torch.cuda.Stream()
    d_in = _dev(_limbs(inputs[:n]))
    out = torch.zeros(n * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        eng.fr_poseidon_batch_dev(d_in.data_ptr(), arity, out.data_ptr(), n, stream=stream.cuda_stream)
    stream.synchronize()
    _same(_host(out), eng.fr_poseidon_batch(_limbs(inputs[:n])))
    _same(_host(out), FC.rows(want[:n]))


def test_the_seam_between_sub_launches(eng, lib, hashes, trees):
    """257 hashes in sub-launches of 100, and a tree of 2^9 leaves in sub-launches of 100: the launches are those of the cut"""
    inputs, want = hashes[2]
    leaves, nodes = trees[9]
    eng.profile(True); eng.profile_reset()
    assert lib.bn254_fr_poseidon_set_launch_max(100) == 0
    try:
        got = eng.fr_poseidon_batch(_limbs(inputs))
        got_tree = eng.fr_merkle_tree(FC.rows(leaves))
        launches = tuple(eng.kernel_stats(s)[1] for s in ("fr_poseidon", "fr_merkle_level"))
    finally:
        assert lib.bn254_fr_poseidon_set_launch_max(0) == 0
        eng.profile(False)
    assert launches == (3, sum(-(-(1 << l) // 100) for l in range(9)))
    _same(got, FC.rows(want))
    _same(got_tree, FC.rows(nodes))


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 9, 11])
def test_every_node_of_a_tree(eng, trees, log_n):
    leaves, nodes = trees[log_n]
    got = eng.fr_merkle_tree(FC.rows(leaves))
    assert got.shape == ((1 << log_n) - 1, 4)
    if log_n:
        _same(got, FC.rows(nodes))
    if log_n == 3:
        assert nodes[-1] == PC.KNOWN_ROOT_8 and got[-1].tobytes() == FC.rows([PC.KNOWN_ROOT_8]).tobytes()


def test_the_tree_dev_form_on_a_stream(eng, trees):
    import torch
    leaves, nodes = trees[9]
    stream = torch.cuda.Stream()
    d_leaves = _dev(FC.rows(leaves))
    out = torch.zeros(511 * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        eng.fr_merkle_tree_dev(d_leaves.data_ptr(), 9, out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _same(_host(out), FC.rows(nodes))
    assert _host(d_leaves).tobytes() == FC.rows(leaves).tobytes()


def test_two_host_threads_alternate_hashes_and_trees_on_one_context(eng, hashes, trees):
    """the host-buffer forms hold the context's mutex for the whole call: two threads that alternate the two calls on ONE context, out of step
    with each other, get the bytes a single thread gets"""
    inputs, want = hashes[2]
    leaves, nodes = trees[9]
    X, L = _limbs(inputs), FC.rows(leaves)
    W, T = FC.rows(want), FC.rows(nodes)
    bad, go = [], threading.Barrier(2)

    def work(me):
        try:
            go.wait(timeout=30)
            for k in range(6):
                if (k + me) % 2:
                    if eng.fr_poseidon_batch(X).tobytes() != W.tobytes(): bad.append((me, k, "hash"))
                else:
                    if eng.fr_merkle_tree(L).tobytes() != T.tobytes(): bad.append((me, k, "tree"))
        except Exception as e:                                                                  # a thread must not die silently
            bad.append((me, repr(e)))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts: t.start()
    for t in ts: t.join(timeout=120)
    assert not any(t.is_alive() for t in ts) and bad == []
    assert X.tobytes() == _limbs(inputs).tobytes() and L.tobytes() == FC.rows(leaves).tobytes()


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr, poseidon
    assert bn_amd.fr_poseidon_batch([[Fr(1), Fr(2)], [Fr(0), Fr(0)]]) == [Fr(PC.KNOWN_HASH[(1, 2)]), Fr(PC.KNOWN_HASH[(0, 0)])]
    assert bn_amd.fr_poseidon_permute_batch([[Fr(0), Fr(1), Fr(2)]])[0] == [Fr(v) for v in PC.permute([0, 1, 2])]
    assert bn_amd.fr_merkle_tree([Fr(i) for i in range(8)])[-1] == Fr(PC.KNOWN_ROOT_8) and bn_amd.fr_merkle_tree([Fr(3)]) == []
    for k in (1, 2, 3, 4):
        assert poseidon.hash([Fr(i) for i in range(1, k + 1)]) == Fr(PC.KNOWN_HASH[tuple(range(1, k + 1))]) == Fr(poseidon.hash_host(range(1, k + 1)))
