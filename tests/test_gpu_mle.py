"""Multilinear tables and sumcheck rounds over Fr on an MI355X (run with -m gpu): bn254_fr_mle_eq, bn254_fr_mle_fold, bn254_fr_sumcheck_round, their
_dev entry points, the Python faces and bn_amd.mle.  The model is Python integers (tests/mle_cases.py over tests/fr_cases.py): the expected
bytes are the limbs of v * 2^256 mod r, and they do not depend on how the plan deals the indices out.  The shapes are the smallest that reach
every seam of the plan for the shipped piece length P and fan F, read from the library's internal hooks: around one lane, one sum lane per
t, a second and a third sum level, two sub-launches of a level."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as FC
import mle_cases as MC

pytestmark = pytest.mark.gpu
R = FC.R
GROUP_SETS = MC.group_sets()


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_sumcheck_piece.argtypes = []; l.bn254_fr_sumcheck_piece.restype = C.c_uint
    l.bn254_fr_sumcheck_fan.argtypes = []; l.bn254_fr_sumcheck_fan.restype = C.c_uint
    l.bn254_fr_mle_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def PF(lib):
    return int(lib.bn254_fr_sumcheck_piece()), int(lib.bn254_fr_sumcheck_fan())


@pytest.fixture(scope="module")
def tables(PF):
    """per group set, rows of integers for the largest half length - computed once, never changed; a shape takes its first h and its last h rows"""
    P, F = PF
    most = max(MC.round_shapes(P, F))
    return {name: MC.rows_of(2 * most, k, 7 + i) for i, (name, k, degree, groups) in enumerate(GROUP_SETS)}


def _rows_for(rows, h):
    return rows[:h] + rows[len(rows) - h:]


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    assert got.tobytes() == want.tobytes(), np.nonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))[0][:8]


def _limb_groups(groups):
    return [(FC.rows([c])[0], m) for c, m in groups]


@pytest.mark.parametrize("which", range(9), ids=["1", "2", "P-1", "P", "P+1", "2P", "FP", "FP+1", "FFP+1"])
@pytest.mark.parametrize("name, k, degree, groups", GROUP_SETS, ids=[g[0] for g in GROUP_SETS])
def test_the_round_over_every_shape_and_group_set(eng, PF, tables, name, k, degree, groups, which):
    h = MC.round_shapes(*PF)[which]
    rows = _rows_for(tables[name], h)
    want = MC.round_sums(rows, groups, degree)
    got = eng.fr_sumcheck_round(MC.limbs(rows), _limb_groups(groups), degree)
    _same(got, FC.rows(want))
    assert (want[0] + want[1]) % R == sum(MC.expression(r, groups) for r in rows) % R          # out[0] + out[1] is the sum over all n
    if name.startswith("degree 1"):
        assert want == [sum(r[0] for r in rows[:h]) % R, sum(r[0] for r in rows[h:]) % R]       # the two half sums


def test_the_limits_sixteen_tables_and_sixteen_groups(eng, PF):
    P, F = PF
    rng = np.random.default_rng(3)
    rows = MC.rows_of(2 * (P + 1), 16, 21)
    groups = [(FC.rand(rng), [c, (c * 5 + 3) % 16, 15 - c][:1 + c % 3]) for c in range(16)]
    _same(eng.fr_sumcheck_round(MC.limbs(rows), _limb_groups(groups)), FC.rows(MC.round_sums(rows, groups, 3)))


def test_the_seam_between_sub_launches_of_a_round(eng, lib, PF, tables):
    """25 lanes in sub-launches of 20: the launches of the two round scopes are those of the model"""
    P, F = PF
    name, k, degree, groups = GROUP_SETS[0]
    rows = _rows_for(tables[name], 25 * P)
    eng.profile(True); eng.profile_reset()
    assert lib.bn254_fr_mle_set_launch_max(20) == 0
    try:
        got = eng.fr_sumcheck_round(MC.limbs(rows), _limb_groups(groups), degree)
        launches = tuple(eng.kernel_stats(s)[1] for s in ("fr_sumcheck_round", "fr_sumcheck_sum"))
    finally:
        assert lib.bn254_fr_mle_set_launch_max(0) == 0
        eng.profile(False)
    assert launches == MC.launches(25 * P, degree, P, F, 20)
    _same(got, FC.rows(MC.round_sums(rows, groups, degree)))


@pytest.mark.parametrize("length", [2, 4, 254, 256, 258, 2 * 8193])
def test_fold_against_the_model(eng, length):
    t = MC.values(length, 31)
    T = FC.rows(t)
    rng = np.random.default_rng(length)
    for r in (0, 1, R - 1, FC.rand(rng)):
        _same(eng.fr_mle_fold(T, FC.rows([r])[0]), FC.rows(MC.fold(t, r)))
    assert T.tobytes() == FC.rows(t).tobytes()


def test_fold_in_place_on_a_stream_leaves_the_upper_half(eng):
    """device-resident records on a stream that is not the default one; out is in, then out is another buffer; r is overwritten as soon as
    the call has returned"""
    import torch
    length = 2 * 8193
    t = MC.values(length, 32)
    T = FC.rows(t)
    stream = torch.cuda.Stream()
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")
    d_in, d_in2 = dev(T), dev(T)
    out = torch.zeros(length // 2 * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    r = [FC.rows([v])[0].copy() for v in (R - 2, 12345)]
    with torch.cuda.stream(stream):
        eng.fr_mle_fold_dev(d_in.data_ptr(), length, r[0], d_in.data_ptr(), stream=stream.cuda_stream)
        r[0][:] = 0
        eng.fr_mle_fold_dev(d_in2.data_ptr(), length, r[1], out.data_ptr(), stream=stream.cuda_stream)
        r[1][:] = 0
    stream.synchronize()
    host = lambda x: x.cpu().numpy().view(np.uint64).reshape(-1, 4)
    _same(host(d_in)[:length // 2], FC.rows(MC.fold(t, R - 2)))
    _same(host(d_in)[length // 2:], T[length // 2:])
    _same(host(out), FC.rows(MC.fold(t, 12345)))
    assert host(d_in2).tobytes() == T.tobytes()


def test_one_fold_of_six_records_is_three_folds(eng):
    rows = MC.rows_of(2, 3, 33)
    got = eng.fr_mle_fold(MC.limbs(rows), FC.rows([77])[0])
    assert got.shape == (1, 3, 4)
    for j in range(3):
        _same(got[:, j], eng.fr_mle_fold(FC.rows([rows[0][j], rows[1][j]]), FC.rows([77])[0]))
        _same(got[:, j], FC.rows(MC.fold([rows[0][j], rows[1][j]], 77)))


@pytest.mark.parametrize("nv", [0, 1, 2, 7, 13])
def test_eq_against_the_model(eng, lib, nv):
    rng = np.random.default_rng(40 + nv)
    z = [(R - 1) if j % 3 == 1 else FC.rand(rng) for j in range(nv)]
    want = MC.eq_table(z)
    assert sum(want) % R == 1                                                                   # the table sums to one
    _same(eng.fr_mle_eq(FC.rows(z)), FC.rows(want))
    bits = [(j * 5 + 1) % 3 % 2 for j in range(nv)]                                             # a point of the hypercube: the indicator of its index
    ind = [0] * (1 << nv); ind[sum(b << j for j, b in enumerate(bits))] = 1
    _same(eng.fr_mle_eq(FC.rows(bits)), FC.rows(ind))
    if nv == 13:                                                                                # 32 sub-launches of 256 lanes
        eng.profile(True); eng.profile_reset()
        assert lib.bn254_fr_mle_set_launch_max(256) == 0
        try:
            got = eng.fr_mle_eq(FC.rows(z))
            launches = eng.kernel_stats("fr_mle_eq")[1]
        finally:
            assert lib.bn254_fr_mle_set_launch_max(0) == 0
            eng.profile(False)
        assert launches == 32
        _same(got, FC.rows(want))


def test_eq_dev_on_a_stream(eng):
    import torch
    z = MC.values(9, 44)
    stream = torch.cuda.Stream()
    d_z = torch.from_numpy(FC.rows(z).view(np.int64).copy()).to("cuda:0")
    out = torch.zeros(512 * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        eng.fr_mle_eq_dev(d_z.data_ptr(), 9, out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _same(out.cpu().numpy().view(np.uint64).reshape(-1, 4), FC.rows(MC.eq_table(z)))


def test_the_round_dev_form_on_a_stream(eng, PF, tables):
    import torch
    P, F = PF
    name, k, degree, groups = GROUP_SETS[1]
    h = F * P + 1
    rows = _rows_for(tables[name], h)
    stream = torch.cuda.Stream()
    d_t = torch.from_numpy(MC.limbs(rows).view(np.int64).copy()).to("cuda:0")
    out = torch.zeros((degree + 1) * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        assert eng.fr_sumcheck_round_dev(d_t.data_ptr(), 2 * h, k, _limb_groups(groups), out.data_ptr(), stream=stream.cuda_stream) == degree
    stream.synchronize()
    _same(out.cpu().numpy().view(np.uint64).reshape(-1, 4), FC.rows(MC.round_sums(rows, groups, degree)))


def test_evaluate_is_nv_folds_and_the_model(eng):
    from bn_amd import Fr, mle
    t = MC.values(1 << 9, 51)
    point = MC.values(9, 52)
    y = mle.evaluate(FC.rows(t), [Fr(p) for p in point], engine=eng)
    assert y == Fr(MC.evaluate(t, point))
    cur = FC.rows(t)
    for r in point[::-1]:
        cur = mle.fold(cur, Fr(r), limbs=True, engine=eng)
    assert cur.shape == (1, 4) and Fr.from_limbs(cur[0]) == y


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr
    z = [Fr(v) for v in MC.values(3, 53)]
    assert bn_amd.fr_mle_eq(z) == [Fr(v) for v in MC.eq_table([x.v for x in z])] and bn_amd.fr_mle_eq([]) == [Fr.one()]
    a = [Fr(v) for v in MC.values(6, 54)]
    assert bn_amd.fr_mle_fold(a, z[0]) == [Fr(v) for v in MC.fold([x.v for x in a], z[0].v)]
    cols = [[Fr(v) for v in MC.values(6, 55 + j)] for j in range(2)]
    groups = [(Fr(3), [0, 1]), (Fr(R - 1), [1])]
    rows = [[c[i].v for c in cols] for i in range(6)]
    assert bn_amd.fr_sumcheck_round(cols, groups) == [Fr(v) for v in MC.round_sums(rows, [(3, [0, 1]), (R - 1, [1])], 2)]
