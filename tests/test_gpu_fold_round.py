"""The fused fold-then-round call on an MI355X (run with -m gpu): bn254_fr_sumcheck_fold_round, its _dev entry point, the Python faces and
bn_amd.sumcheck.prove_resident.  The model is Python integers (tests/fold_round_cases.py: MC.fold, then MC.round_sums), and every result is
also compared in bytes with fr_mle_fold followed by fr_sumcheck_round on the same engine.  The shapes are the smallest that reach every seam
of the plan for the shipped piece length P and fan F: around one lane, one sum lane per t, a second and a third sum level, two sub-launches
of a level - with the piece forced to the shipped value, and with nothing forced (the adaptive choice, 4 at these sizes)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import fold_round_cases as FR
import fr_cases as FC
import mle_cases as MC

pytestmark = pytest.mark.gpu
R = FC.R
SETS = FR.group_sets()


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_sumcheck_fold_piece.argtypes = []; l.bn254_fr_sumcheck_fold_piece.restype = C.c_uint
    l.bn254_fr_sumcheck_fold_set_piece.argtypes = [C.c_uint]
    l.bn254_fr_sumcheck_fan.argtypes = []; l.bn254_fr_sumcheck_fan.restype = C.c_uint
    l.bn254_fr_mle_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def PF(lib):
    return int(lib.bn254_fr_sumcheck_fold_piece()), int(lib.bn254_fr_sumcheck_fan())


@pytest.fixture(scope="module")
def tables(PF):
    """per group set, rows of integers for the largest h2 - computed once, never changed; a shape takes its first 2 h2 and its last 2 h2 rows"""
    most = max(MC.round_shapes(*PF))
    return {name: MC.rows_of(4 * most, k, 17 + i) for i, (name, k, degree, groups) in enumerate(SETS)}


@pytest.fixture(scope="module")
def model():
    """(group set, h2, r) -> (folded limbs, sums limbs), computed once per key and shared by the forced and the adaptive run"""
    return {}


def _want(model, tables, name, groups, degree, h2, r):
    if (name, h2, r) not in model:
        folded, sums = FR.fold_round(FR.rows_for(tables[name], h2), r, groups, degree)
        model[name, h2, r] = (MC.limbs(folded), FC.rows(sums))
    return model[name, h2, r]


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    assert got.tobytes() == want.tobytes(), np.nonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))[0][:8]


def _limb_groups(groups):
    return [(FC.rows([c])[0], m) for c, m in groups]


def _fr(v):
    return FC.rows([v])[0]


class _Piece:
    """the piece forced for a block, restored at its end"""
    def __init__(self, lib, P): self.lib, self.P = lib, P

    def __enter__(self): assert self.lib.bn254_fr_sumcheck_fold_set_piece(self.P) == 0

    def __exit__(self, *exc): assert self.lib.bn254_fr_sumcheck_fold_set_piece(0) == 0


@pytest.mark.parametrize("forced", [True, False], ids=["shipped piece", "adaptive piece"])
@pytest.mark.parametrize("which", range(9), ids=["1", "2", "P-1", "P", "P+1", "2P", "FP", "FP+1", "FFP+1"])
@pytest.mark.parametrize("name, k, degree, groups", SETS, ids=[g[0] for g in SETS])
def test_fold_round_over_every_shape_and_group_set(eng, lib, PF, tables, model, name, k, degree, groups, which, forced):
    h2 = MC.round_shapes(*PF)[which]
    r = FR.challenges(h2)[3]
    rows = FR.rows_for(tables[name], h2)
    T = MC.limbs(rows)
    before = T.copy()
    folded_w, out_w = _want(model, tables, name, groups, degree, h2, r)
    lg = _limb_groups(groups)
    with _Piece(lib, PF[0] if forced else 0):
        folded, out = eng.fr_sumcheck_fold_round(T, _fr(r), lg, degree)
    _same(folded, folded_w); _same(out, out_w)
    assert T.tobytes() == before.tobytes()
    two = eng.fr_mle_fold(T, _fr(r))                                                            # the two calls it replaces, same engine
    _same(folded, two); _same(out, eng.fr_sumcheck_round(two, lg, degree))


@pytest.mark.parametrize("r", [0, 1])
def test_the_challenges_zero_and_one_keep_the_lower_and_the_upper_half(eng, PF, tables, r):
    name, k, degree, groups = SETS[0]
    h2 = PF[0] + 1
    rows = FR.rows_for(tables[name], h2)
    T = MC.limbs(rows)
    folded, out = eng.fr_sumcheck_fold_round(T, _fr(r), _limb_groups(groups), degree)
    _same(folded, T[2 * h2 * r:2 * h2 * (r + 1)])
    _same(out, FC.rows(MC.round_sums(rows[2 * h2 * r:2 * h2 * (r + 1)], groups, degree)))


def test_the_limits_sixteen_tables_and_sixteen_groups_and_degree_one(eng, PF):
    P, F = PF
    rng = np.random.default_rng(3)
    rows = MC.rows_of(4 * (P + 1), 16, 21)
    groups = [(FC.rand(rng), [c, (c * 5 + 3) % 16, 15 - c][:1 + c % 3]) for c in range(16)]
    r = FC.rand(rng)
    folded_w, sums = FR.fold_round(rows, r, groups, 3)
    folded, out = eng.fr_sumcheck_fold_round(MC.limbs(rows), _fr(r), _limb_groups(groups))
    _same(folded, MC.limbs(folded_w)); _same(out, FC.rows(sums))
    rows = MC.rows_of(4 * (2 * P + 3), 1, 22)                                                   # degree 1 with one table
    folded_w, sums = FR.fold_round(rows, r, [(1, [0])], 1)
    folded, out = eng.fr_sumcheck_fold_round(MC.limbs(rows), _fr(r), [(_fr(1), [0])], 1)
    _same(folded, MC.limbs(folded_w)); _same(out, FC.rows(sums))
    half = len(rows) // 4
    assert sums == [sum(x[0] for x in folded_w[:half]) % R, sum(x[0] for x in folded_w[half:]) % R]


def test_the_seam_between_sub_launches(eng, lib, PF, tables):
    """25 lanes in sub-launches of 20: the launches of the two scopes are those of the model"""
    P, F = PF
    name, k, degree, groups = SETS[0]
    rows = FR.rows_for(tables[name], 25 * P)
    r = FR.challenges(25)[3]
    eng.profile(True); eng.profile_reset()
    assert lib.bn254_fr_mle_set_launch_max(20) == 0
    try:
        with _Piece(lib, P):
            folded, out = eng.fr_sumcheck_fold_round(MC.limbs(rows), _fr(r), _limb_groups(groups), degree)
        launches = tuple(eng.kernel_stats(s)[1] for s in ("fr_sumcheck_fold_round", "fr_sumcheck_sum"))
    finally:
        assert lib.bn254_fr_mle_set_launch_max(0) == 0
        eng.profile(False)
    assert launches == FR.launches(25 * P, degree, P, F, 20)
    folded_w, sums = FR.fold_round(rows, r, groups, degree)
    _same(folded, MC.limbs(folded_w)); _same(out, FC.rows(sums))


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")


def _host(x):
    return x.cpu().numpy().view(np.uint64).reshape(-1, 4)


def test_the_dev_form_in_place_on_a_stream_twice_in_a_row(eng, PF, tables):
    """in place on a stream that is not the default one; the second call folds what the first one left, with no host synchronisation between
    them; r is overwritten as soon as a call has returned"""
    import torch
    P, F = PF
    name, k, degree, groups = SETS[1]
    h2 = 2 * (F * P + 1)                                                                        # n = 8 (F P + 1): the second call has n / 2
    rows = FR.rows_for(tables[name], h2)
    T = MC.limbs(rows)
    n = len(rows)
    lg = _limb_groups(groups)
    stream = torch.cuda.Stream()
    d_t = _dev(T)
    outs = torch.zeros(2 * (degree + 1) * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    r = [_fr(v).copy() for v in (R - 2, 12345)]
    with torch.cuda.stream(stream):
        assert eng.fr_sumcheck_fold_round_dev(d_t.data_ptr(), n, k, r[0], lg, d_t.data_ptr(), outs.data_ptr(), stream=stream.cuda_stream) == degree
        r[0][:] = 0
        eng.fr_sumcheck_fold_round_dev(d_t.data_ptr(), n // 2, k, r[1], lg, d_t.data_ptr(), outs.data_ptr() + 32 * (degree + 1), degree, stream.cuda_stream)
        r[1][:] = 0
    stream.synchronize()
    f1, s1 = FR.fold_round(rows, R - 2, groups, degree)
    f2, s2 = FR.fold_round(f1, 12345, groups, degree)
    got = _host(d_t).reshape(n, k, 4)
    _same(got[:n // 4], MC.limbs(f2))
    _same(got[n // 4:n // 2], MC.limbs(f1)[n // 4:])                                            # the upper half of the first result, left by the second call
    _same(got[n // 2:], T[n // 2:])                                                             # the upper half of the input, left by the first
    _same(_host(outs), FC.rows(s1 + s2))


def test_the_scratch_is_ordered_between_the_fused_call_and_the_round_on_two_streams(eng, PF, tables):
    """fr_sumcheck_fold_round_dev on one stream and fr_sumcheck_round_dev on another, back to back on one context: both put their partial
    sums into the same context-owned scratch, and each must give the bytes it gives alone"""
    import torch
    P, F = PF
    name, k, degree, groups = SETS[0]
    lg = _limb_groups(groups)
    h2 = F * F * P + 1
    rows = FR.rows_for(tables[name], h2)
    other = rows[::-1][:2 * (F * F * P + 1)]
    r = FR.challenges(9)[3]
    d_a, d_b = _dev(MC.limbs(rows)), _dev(MC.limbs(other))
    folded = torch.zeros(len(rows) // 2 * k * 4, dtype=torch.int64, device="cuda:0")
    out_a = torch.zeros(6 * (degree + 1) * 4, dtype=torch.int64, device="cuda:0")
    out_b = torch.zeros(6 * (degree + 1) * 4, dtype=torch.int64, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in range(6):
        eng.fr_sumcheck_fold_round_dev(d_a.data_ptr(), len(rows), k, _fr(r), lg, folded.data_ptr(), out_a.data_ptr() + 32 * (degree + 1) * rep, degree, s1.cuda_stream)
        eng.fr_sumcheck_round_dev(d_b.data_ptr(), len(other), k, lg, out_b.data_ptr() + 32 * (degree + 1) * rep, degree, s2.cuda_stream)
    torch.cuda.synchronize()
    folded_w, sums = FR.fold_round(rows, r, groups, degree)
    _same(_host(folded).reshape(-1, k, 4), MC.limbs(folded_w))
    _same(_host(out_a), FC.rows(sums * 6))
    _same(_host(out_b), FC.rows(MC.round_sums(other, groups, degree) * 6))


def test_the_host_form_in_place_leaves_the_upper_half(eng, PF, tables):
    """the C entry point on host buffers with folded == tables: the lower half is the fold, rows [n/2, n) are left as they were"""
    from bn_amd import _native
    name, k, degree, groups = SETS[0]
    h2 = PF[1] * PF[0] + 1
    rows = FR.rows_for(tables[name], h2)
    T = MC.limbs(rows)
    before = T.copy()
    n = len(rows)
    r = FR.challenges(11)[3]
    off = np.concatenate([[0], np.cumsum([len(m) for _, m in groups])]).astype(np.uint64)
    members = np.array([j for _, m in groups for j in m], np.uint64)
    coeff = FC.rows([c for c, _ in groups])
    out = np.zeros((degree + 1, 4), np.uint64)
    p = lambda a: a.ctypes.data
    _native.check(_native.lib().bn254_fr_sumcheck_fold_round(eng._h, p(T), n, k, p(_fr(r)), p(off), p(members), p(coeff), len(groups), degree, p(T), p(out)))
    folded_w, sums = FR.fold_round(rows, r, groups, degree)
    _same(T[:n // 2], MC.limbs(folded_w)); _same(T[n // 2:], before[n // 2:]); _same(out, FC.rows(sums))


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr
    cols = [[Fr(v) for v in MC.values(12, 55 + j)] for j in range(2)]
    groups = [(Fr(3), [0, 1]), (Fr(R - 1), [1])]
    rows = [[c[i].v for c in cols] for i in range(12)]
    folded, out = bn_amd.fr_sumcheck_fold_round(cols, Fr(77), groups)
    folded_w, sums = FR.fold_round(rows, 77, [(3, [0, 1]), (R - 1, [1])], 2)
    _same(folded, MC.limbs(folded_w))
    assert out == [Fr(v) for v in sums]


# ---------------------------------------------------------------------------------------------------------------- prove_resident
PROOF_SETS = [s for s in SETS if s[0] in ("degree 3, four groups", "degree 4, a table twice")]


@pytest.fixture(scope="module")
def proofs(eng):
    """(group set, nv) -> (rows of integers, groups as Fr, proof and point of prove, of prove_resident) - proved once, never changed"""
    from bn_amd import Fr, sumcheck
    out = {}
    for name, k, degree, groups in PROOF_SETS:
        for nv in (1, 2, 5, 13):
            rows = MC.rows_of(1 << nv, k, 80 + nv)
            gs = [(Fr(c), m) for c, m in groups]
            T = MC.limbs(rows)
            out[name, nv] = (rows, gs, sumcheck.prove(T, gs, engine=eng), sumcheck.prove_resident(T, gs, engine=eng))
    return out


@pytest.mark.parametrize("nv", [1, 2, 5, 13])
@pytest.mark.parametrize("name, k, degree, groups", PROOF_SETS, ids=[g[0] for g in PROOF_SETS])
def test_prove_resident_gives_the_proof_of_prove_and_of_the_model(eng, proofs, name, k, degree, groups, nv):
    from bn_amd import Fr, mle, sumcheck
    rows, gs, (proof, point), (rproof, rpoint) = proofs[name, nv]
    assert rproof == proof and rpoint == point                                                  # claim, rounds, finals and point
    # the model prover over the transcript restated with hashlib
    h = lambda b: hashlib.sha256(b).digest()
    be = lambda xs: b"".join(int(x).to_bytes(32, "big") for x in xs)
    state = [h(b"bn_amd.sumcheck")]
    state[0] = h(state[0] + be([nv, k, degree, len(groups)]))
    for c, m in groups:
        state[0] = h(state[0] + be([c, len(m)] + m))
    claim = sum(MC.expression(r, groups) for r in rows) % R
    state[0] = h(state[0] + be([claim]))

    def challenge(s, g):
        state[0] = h(state[0] + be(g))
        r = int.from_bytes(h(state[0] + b"\x00") + h(state[0] + b"\x01"), "big") % R
        state[0] = h(state[0] + b"\x02")
        return r
    mclaim, mrounds, mfinals, mpoint = MC.prove(rows, groups, challenge)
    assert mclaim == claim == rproof.claim.v
    assert [[x.v for x in g] for g in rproof.rounds] == mrounds and [x.v for x in rproof.finals] == mfinals and [p.v for p in rpoint] == mpoint
    ok, vpoint = sumcheck.verify(rproof, nv, gs)
    assert ok and vpoint == rpoint
    T = MC.limbs(rows)
    assert rproof.finals == [mle.evaluate(T[:, j], rpoint, engine=eng) for j in range(k)]


def test_prove_resident_with_the_two_calls_gives_the_same_proof(eng, proofs):
    """the loop prove_resident falls back to when the fusion does not pay: fr_mle_fold_dev in place, then fr_sumcheck_round_dev"""
    from bn_amd import sumcheck
    name = PROOF_SETS[0][0]
    for nv in (2, 13):
        rows, gs, _, (rproof, rpoint) = proofs[name, nv]
        for fused in (True, False):
            assert sumcheck._prove_resident(MC.limbs(rows), gs, None, eng, fused) == (rproof, rpoint)
