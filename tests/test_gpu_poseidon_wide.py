"""Wide Poseidon over Fr on an MI355X (run with -m gpu): bn254_fr_poseidon_ex_batch, bn254_fr_poseidon_chain_batch, their _dev entry points and the
Python faces.  The model is Python integers (tests/poseidon_wide_cases.py, written independently of bn_amd/poseidon.py): the expected bytes
are the limbs of v * 2^256 mod r - byte equality, no tolerance.  The sizes are the seams, not the workload: a group, a wave and a workgroup
of the lanes-per-permutation the library ships (read from its hook), one row, and a seam between two sub-launches reached through the
library's internal hook, as the other Fr families reach theirs."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as FC
import poseidon_cases as PC
import poseidon_wide_cases as WC

pytestmark = pytest.mark.gpu
R = FC.R


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_poseidon_wide_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_fr_poseidon_wide_lanes.argtypes = []
    l.bn254_fr_poseidon_wide_block.argtypes = []
    return l


@pytest.fixture(scope="module")
def rows16():
    """257 rows of 16 inputs (the known-answer row first, the all-edge rows, every edge value in every position, random rows), one init per
    row and the model's whole permutations with and without it - computed once, never changed; a size takes the first n rows"""
    rows = WC.ex_rows(16, 257, 1600, edges=True)
    init = [R - 1, 1, 0] + WC.values(254, 1601)
    return rows, init, [WC.permute([0] + r) for r in rows], [WC.permute([i] + r) for i, r in zip(init, rows)]


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    assert got.tobytes() == want.tobytes(), np.nonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))[0][:8]


def _limbs(rows_of_ints):
    return WC.rows(rows_of_ints).reshape(len(rows_of_ints), -1, 4)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1).copy()).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("n_inputs", range(1, 17))
def test_ex_at_every_width_against_the_model(eng, n_inputs):
    rows = WC.ex_rows(n_inputs, 65, 1000 + n_inputs)
    want = [WC.hash_ex(r)[0] for r in rows]
    assert want[0] == WC.KNOWN[n_inputs]                  # rows 6 and 16: circomlibjs's values; 1 and 2: pinned before; the others this project's own
    X = _limbs(rows)
    _same(eng.fr_poseidon_ex_batch(X).reshape(-1, 4), FC.rows(want))
    assert X.tobytes() == _limbs(rows).tobytes()


def test_ex_at_the_seams_of_a_group_a_wave_and_a_workgroup(eng, lib, rows16):
    rows, _, full, _ = rows16
    G, block = lib.bn254_fr_poseidon_wide_lanes(), lib.bn254_fr_poseidon_wide_block()
    assert G in (4, 8, 16) and block % 64 == 0
    sizes = sorted({1, 64 // G - 1, 64 // G, 64 // G + 1, block // G - 1, block // G + 1, 257})
    assert all(0 < n <= 257 for n in sizes)
    want = FC.rows([s[0] for s in full])
    for n in sizes:
        _same(eng.fr_poseidon_ex_batch(_limbs(rows[:n])).reshape(-1, 4), want[:n])


@pytest.mark.parametrize("n_outs", [1, 2, 17])
def test_n_outs_and_init_with_edge_elements_in_every_position(eng, rows16, n_outs):
    rows, init, full_0, full_i = rows16
    n = 3 + 3 * 16 + 1 + 12                               # the known-answer row, the all-edge rows, every edge in every position, random rows
    X = _limbs(rows[:n])
    _same(eng.fr_poseidon_ex_batch(X, None, n_outs).reshape(-1, 4), FC.rows([v for s in full_0[:n] for v in s[:n_outs]]))
    _same(eng.fr_poseidon_ex_batch(X, FC.rows(init[:n]), n_outs).reshape(-1, 4), FC.rows([v for s in full_i[:n] for v in s[:n_outs]]))


@pytest.mark.parametrize("n_inputs", [1, 2, 3, 4])
def test_ex_is_byte_equal_to_the_one_lane_kernels(eng, n_inputs):
    """the same inputs through the existing kernels: the hash, and the permutation with element 0 as init and every output"""
    t = n_inputs + 1
    states = PC.states(t, 65, 1100 + t)
    S = PC.rows(states).reshape(65, t, 4)
    inputs = np.ascontiguousarray(S[:, 1:])
    _same(eng.fr_poseidon_ex_batch(inputs).reshape(-1, 4), eng.fr_poseidon_batch(inputs))
    _same(eng.fr_poseidon_ex_batch(inputs, np.ascontiguousarray(S[:, 0]), t), eng.fr_poseidon_permute_batch(S))


@pytest.fixture(scope="module")
def chains():
    """per rate: 300 records of lengths 0 .. 3 rate + 2, shuffled so that the groups of one wave run different numbers of blocks, and the model's digests"""
    out = {}
    for rate in (1, 2, 15, 16):
        lengths = WC.mixed_lengths(rate, 300, 1200 + rate)
        recs, flat, off = WC.records(lengths, 1300 + rate)
        out[rate] = (flat, off, [WC.hash_chain(r, rate) for r in recs])
    return out


@pytest.mark.parametrize("rate", [1, 2, 15, 16])
def test_chains_of_mixed_lengths(eng, chains, rate):
    flat, off, want = chains[rate]
    lengths = np.diff(off.astype(np.int64))
    blocks = np.maximum(1, -(-lengths // rate))
    assert len(set(blocks[:8].tolist())) > 1 and set(WC.chain_lengths(rate)) <= set(lengths.tolist())
    X = FC.rows(flat)
    _same(eng.fr_poseidon_chain_batch(X, off, rate), FC.rows(want))
    assert X.tobytes() == FC.rows(flat).tobytes()


def test_one_chain_and_only_empty_ones(eng, chains):
    flat, off, want = chains[16]
    a, b = int(off[5]), int(off[6])
    _same(eng.fr_poseidon_chain_batch(FC.rows(flat[a:b]) if b > a else np.zeros((0, 4), np.uint64), [0, b - a], 16), FC.rows(want[5:6]))
    _same(eng.fr_poseidon_chain_batch(np.zeros((0, 4), np.uint64), [0, 0, 0], 16), FC.rows([WC.hash_chain([], 16)] * 2))


def test_the_chain_dev_form_agrees_with_the_host_buffer_form(eng, chains):
    import torch
    flat, off, want = chains[15]
    stream = torch.cuda.Stream()
    d_in = _dev(FC.rows(flat))
    out = torch.zeros(300 * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        eng.fr_poseidon_chain_batch_dev(d_in.data_ptr(), off, 15, out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _same(_host(out), eng.fr_poseidon_chain_batch(FC.rows(flat), off, 15))
    _same(_host(out), FC.rows(want))
    assert _host(d_in).tobytes() == FC.rows(flat).tobytes()


def test_the_seam_between_sub_launches(eng, lib, rows16, chains):
    """65 rows and 300 records in sub-launches of 100 LANES: the launches are those of the cut"""
    rows, init, _, full_i = rows16
    flat, off, want = chains[2]
    G = lib.bn254_fr_poseidon_wide_lanes()
    per = max(1, 100 // G)
    eng.profile(True); eng.profile_reset()
    assert lib.bn254_fr_poseidon_wide_set_launch_max(100) == 0
    try:
        got = eng.fr_poseidon_ex_batch(_limbs(rows[:65]), FC.rows(init[:65]), 2)
        got_chain = eng.fr_poseidon_chain_batch(FC.rows(flat), off, 2)
        launches = tuple(eng.kernel_stats(s)[1] for s in ("fr_poseidon_ex", "fr_poseidon_chain"))
    finally:
        assert lib.bn254_fr_poseidon_wide_set_launch_max(0) == 0
        eng.profile(False)
    assert launches == (-(-65 // per), -(-300 // per))
    _same(got.reshape(-1, 4), FC.rows([v for s in full_i[:65] for v in s[:2]]))
    _same(got_chain, FC.rows(want))


def test_two_widths_first_used_from_dev_calls_on_two_streams():
    """a fresh context whose first use of two widths are _dev calls, one after the other on two streams: each call finds the table it needs in
    place (the upload is a blocking copy made before the launch is enqueued)"""
    import bn_amd
    import torch
    e = bn_amd.Engine(0)
    cases = []
    for n_inputs, seed in ((9, 1400), (13, 1401)):                                              # no other test of this module uses these on this context
        rows = WC.ex_rows(n_inputs, 20, seed)
        cases.append((n_inputs, rows, _dev(_limbs(rows)), torch.zeros(20 * 4, dtype=torch.int64, device="cuda:0"), torch.cuda.Stream()))
    torch.cuda.synchronize()
    for n_inputs, _, d_in, out, stream in cases:
        with torch.cuda.stream(stream):
            e.fr_poseidon_ex_batch_dev(d_in.data_ptr(), n_inputs, None, 1, out.data_ptr(), 20, stream=stream.cuda_stream)
    for n_inputs, rows, _, out, stream in cases:
        stream.synchronize()
        _same(_host(out), FC.rows([WC.hash_ex(r)[0] for r in rows]))


def test_the_python_face_and_a_tree_from_records(eng):
    import bn_amd
    from bn_amd import Fr, merkle, poseidon
    assert bn_amd.fr_poseidon_ex_batch([[Fr(i) for i in range(1, 7)]]) == [[Fr(WC.KNOWN[6])]]
    assert poseidon.hash_ex([Fr(i) for i in range(1, 17)]) == [Fr(WC.KNOWN[16])]
    x = WC.values(5, 1500)
    assert poseidon.hash_ex([Fr(v) for v in x], init=Fr(7), n_outs=6) == [Fr(v) for v in WC.permute([7] + x)]
    lengths = [0, 1, 15, 16, 17, 50, 3, 33]
    recs, _, _ = WC.records(lengths, 1501)
    rows = [[Fr(v) for v in r] for r in recs]
    leaves = [WC.hash_chain(r, 16) for r in recs]
    assert bn_amd.fr_poseidon_chain_batch(rows) == [Fr(v) for v in leaves]
    assert poseidon.hash_chain(rows[5]) == Fr(leaves[5]) == Fr(poseidon.hash_chain_host(recs[5]))
    tree = merkle.Tree.from_records(rows, rate=16, engine=eng)
    assert [n.v for n in tree.nodes] == PC.tree(leaves) and [l.v for l in tree.leaves] == leaves
    assert merkle.verify(tree.root, tree.leaves[4], 4, tree.open(4))
