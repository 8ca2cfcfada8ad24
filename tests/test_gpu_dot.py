"""Sparse linear maps over Fr on an MI355X (run with -m gpu): bn254_fr_dot_batch, its _dev entry point, the Python faces, and the Groth16
prover built on them (bn_amd.groth16.witness_map / setup / prove) end to end against the verifier.  The model is Python integers
(tests/dot_cases.py over tests/fr_cases.py): the expected bytes are the limbs of v * 2^256 mod r, and they do not depend on how the plan cuts
a segment.  The shapes are the smallest that reach every seam of the plan for the shipped piece length P and fan F, read from the library's
internal hooks: around one piece, one fold lane, a second and a third fold level, two workgroups of pieces, two sub-launches of a level."""
import ctypes as C

import numpy as np
import pytest

import dot_cases as DC
import fr_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_dot_piece.argtypes = []; l.bn254_fr_dot_piece.restype = C.c_uint
    l.bn254_fr_dot_fan.argtypes = []; l.bn254_fr_dot_fan.restype = C.c_uint
    l.bn254_fr_dot_set_launch_max.argtypes = [C.c_size_t]
    return l


@pytest.fixture(scope="module")
def PF(lib):
    return int(lib.bn254_fr_dot_piece()), int(lib.bn254_fr_dot_fan())


@pytest.fixture(scope="module")
def every_length(PF):
    """one call over the whole length list, gathered: (coeff, xval, x, index, offsets, expected rows) - computed once, never changed"""
    lens = DC.lengths(*PF)
    coeff, xval = DC.terms(sum(lens), seed=1)
    x, index = DC.gathered(xval, seed=2)
    offsets = DC.offsets_of(lens)
    return coeff, xval, x, index, offsets, FC.rows(DC.model(coeff, x, offsets, index))


def _diff(got, want):
    return np.nonzero((got != want).any(axis=1))[0][:8]


def test_every_length_against_the_model(eng, every_length):
    coeff, xval, x, index, offsets, want = every_length
    got = eng.fr_dot_batch(FC.rows(coeff), FC.rows(x), offsets, index)
    assert got.shape == want.shape and got.dtype == np.uint64
    assert got.tobytes() == want.tobytes(), _diff(got, want)
    assert not got[0].any()                                                     # the empty segment is Fr::zero()
    got = eng.fr_dot_batch(FC.rows(coeff), FC.rows(xval), offsets)              # index == NULL: x[t], the same sums
    assert got.tobytes() == want.tobytes(), _diff(got, want)


def test_257_segments_that_cycle_through_the_lengths(eng, PF):
    """two workgroups of pieces that write out directly, folded segments among them; empty segments first, last and adjacent"""
    P, F = PF
    cyc = [L for L in DC.lengths(P, F) if L <= F * P + 1]
    lens = [0, 0] + [cyc[j % len(cyc)] for j in range(254)] + [0]
    assert len(lens) == 257
    coeff, xval = DC.terms(sum(lens), seed=3)
    x, index = DC.gathered(xval, seed=4)
    offsets = DC.offsets_of(lens)
    got = eng.fr_dot_batch(FC.rows(coeff), FC.rows(x), offsets, index)
    want = FC.rows(DC.model(coeff, x, offsets, index))
    assert got.tobytes() == want.tobytes(), _diff(got, want)


def test_one_segment_of_three_fold_levels_alone(eng, every_length, PF):
    P, F = PF
    coeff, xval, x, index, offsets, want = every_length
    L = F * F * P + 1
    assert int(offsets[-1] - offsets[-2]) == L and DC.plan_levels(L, P, F) == 3
    lo = int(offsets[-2])
    got = eng.fr_dot_batch(FC.rows(coeff[lo:]), FC.rows(xval[lo:]), [0, L])
    assert got.tobytes() == want[-1:].tobytes()


def test_repeated_and_reversed_indices_and_a_vector_of_one(eng, PF):
    P, F = PF
    lens = [3, P + 1, F * P + 1]
    n = sum(lens)
    coeff, _ = DC.terms(n, seed=11)
    x = FC.values(5, seed=12)
    offsets = DC.offsets_of(lens)
    for index in ([4] * n, [t % 5 for t in range(n)], [4 - t % 5 for t in range(n)]):
        got = eng.fr_dot_batch(FC.rows(coeff), FC.rows(x), offsets, index)
        assert got.tobytes() == FC.rows(DC.model(coeff, x, offsets, index)).tobytes()
    got = eng.fr_dot_batch(FC.rows(coeff), FC.rows([FC.R - 1]), offsets, [0] * n)                  # nx = 1
    assert got.tobytes() == FC.rows(DC.model(coeff, [FC.R - 1], offsets, [0] * n)).tobytes()


def test_the_seam_between_sub_launches(eng, lib, PF):
    """45 pieces in sub-launches of 20: three launches of the product level, one per fold level (20 partial sums, then the rest)"""
    P, F = PF
    lens = [P] * 25 + [20 * P]
    coeff, xval = DC.terms(sum(lens), seed=9)
    offsets = DC.offsets_of(lens)
    eng.profile(True); eng.profile_reset()
    assert lib.bn254_fr_dot_set_launch_max(20) == 0
    try:
        got = eng.fr_dot_batch(FC.rows(coeff), FC.rows(xval), offsets)
        launches = {s: eng.kernel_stats(s)[1] for s in ("fr_dot", "fr_dot_fold")}
    finally:
        assert lib.bn254_fr_dot_set_launch_max(0) == 0
        eng.profile(False)
    assert launches == {"fr_dot": 3, "fr_dot_fold": DC.plan_levels(20 * P, P, F)}
    assert got.tobytes() == FC.rows(DC.model(coeff, xval, offsets)).tobytes()


def test_kernel_stats_show_both_scopes(eng, PF):
    P, F = PF
    coeff, xval = DC.terms(2 * P + 3, seed=5)
    eng.profile(True); eng.profile_reset()
    try:
        eng.fr_dot_batch(FC.rows(coeff), FC.rows(xval), [0, 2 * P + 3])
        stats = {s: eng.kernel_stats(s) for s in ("fr_dot", "fr_dot_fold")}
    finally:
        eng.profile(False)
    for s, (ms, launches) in stats.items():
        assert launches >= 1 and ms > 0, (s, ms, launches)


def test_the_dev_form_on_a_stream_with_its_offsets_freed(eng, every_length):
    """device-resident operands on a stream that is not the default one; the host offsets are overwritten as soon as the call has returned
    (the launches were planned from them); index both NULL and given.  (0.01 s once torch is warm; whichever test of a run uses torch first
    pays the ~11 s of its start-up.)"""
    import torch
    coeff, xval, x, index, offsets, want = every_length
    m = len(offsets) - 1
    stream = torch.cuda.Stream()
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")
    dc, dx, dxv, di = dev(FC.rows(coeff)), dev(FC.rows(x)), dev(FC.rows(xval)), dev(np.array(index, np.uint64))
    o1 = torch.zeros(m * 4, dtype=torch.int64, device="cuda:0"); o2 = torch.zeros_like(o1)
    torch.cuda.synchronize()
    off1, off2 = offsets.copy(), offsets.copy()
    with torch.cuda.stream(stream):
        eng.fr_dot_batch_dev(dc.data_ptr(), di.data_ptr(), dx.data_ptr(), len(x), off1, m, o1.data_ptr(), stream.cuda_stream)
        off1[:] = 1 << 63
        eng.fr_dot_batch_dev(dc.data_ptr(), None, dxv.data_ptr(), len(xval), off2, m, o2.data_ptr(), stream.cuda_stream)
        off2[:] = 1 << 63
    stream.synchronize()
    for what, t in (("index", o1), ("index == NULL", o2)):
        assert t.cpu().numpy().view(np.uint64).reshape(m, 4).tobytes() == want.tobytes(), what


def test_the_python_face(eng):
    import bn_amd
    from bn_amd import Fr
    rng = np.random.default_rng(5)
    coeff = [Fr.random(rng) for _ in range(7)]
    x = [Fr.random(rng) for _ in range(4)] + [Fr.zero()]
    index = [4, 0, 0, 3, 2, 1, 3]
    offsets = [0, 0, 3, 7, 7]
    want = [Fr(sum(coeff[t].v * x[index[t]].v for t in range(offsets[j], offsets[j + 1]))) for j in range(4)]
    assert bn_amd.fr_dot_batch(coeff, x, offsets, index) == want and want[0] == Fr.zero()
    assert bn_amd.fr_dot_batch(np.stack([c.limbs for c in coeff]), np.stack([v.limbs for v in x]), np.array(offsets), np.array(index)) == want      # arrays
    assert bn_amd.fr_dot_batch(coeff[:5], x, [0, 5]) == [Fr(sum(c.v * v.v for c, v in zip(coeff, x)))]
    assert bn_amd.fr_dot_batch([], [], [0]) == [] and bn_amd.fr_dot_batch([], [], [0, 0]) == [Fr.zero()]


# ---- Groth16 end to end: a generated system of 40 constraints (domain 64) whose rows run through every length of the list
def _draws(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(64), "little") % FC.R for _ in range(count)]


@pytest.fixture(scope="module", params=[1, 3])
def proved(request, PF):
    """(l, system as integer lists, R1CS, z rows, trapdoor, pk, vk, proof, (r, s)) - one setup and one proof per l, shared by the tests"""
    import bn_amd
    from bn_amd import groth16
    l = request.param
    _, nv, a, b, c, z = DC.r1cs(40, l, DC.lengths(*PF), seed=70 + l)
    mat = lambda m: (np.array(m[0], np.uint64), np.array(m[1], np.uint64), FC.rows(m[2]))
    system = groth16.R1CS(l, nv, mat(a), mat(b), mat(c))
    Z = FC.rows(z)
    trap = _draws(500 + l, 5)
    assert all(trap) and pow(trap[4], 64, FC.R) != 1                            # then setup keeps the first five draws
    pk, vk = groth16.setup(system, np.random.default_rng(500 + l))
    proof = groth16.prove(pk, system, Z, np.random.default_rng(600 + l))
    return l, (nv, a, b, c, z), system, Z, trap, pk, vk, proof, _draws(600 + l, 2)


def test_witness_map_equals_the_integer_products_row_by_row(proved):
    from bn_amd import groth16
    l, (nv, a, b, c, z), system, Z, *_ = proved
    ev = groth16.witness_map(system, Z)
    rows = len(a[0]) - 1
    for got, m in zip(ev, (a, b, c)):
        assert got.shape == (64, 4) and not got[rows:].any()
        assert got[:rows].tobytes() == FC.rows(DC.model(m[2], z, m[0], m[1])).tobytes()
    az, bz, cz = (DC.model(m[2], z, m[0], m[1]) for m in (a, b, c))
    assert [p * q % FC.R for p, q in zip(az, bz)] == cz


def test_a_proof_from_a_real_constraint_system_verifies(proved):
    from bn_amd import Fr, groth16
    l, (nv, a, b, c, z), system, Z, trap, pk, vk, proof, _ = proved
    public = [Fr(v) for v in z[1:l + 1]]
    assert len(vk.ic) == l + 1 and pk.a_query.shape == (nv, 12) and pk.b_g2_query.shape == (nv, 24) and pk.l_query.shape == (nv - l - 1, 12) and pk.h_query.shape == (63, 12)
    assert groth16.verify_batch(vk, [proof], [public]).tolist() == [True]
    assert groth16.verify_aggregate(vk, [proof], [public]) is True
    wrong = list(public); wrong[0] = wrong[0] + Fr.one()
    assert groth16.verify_batch(vk, [proof], [wrong]).tolist() == [False]       # a wrong public input


def test_setup_and_the_transposed_product_without_the_verifier(proved):
    """with the trapdoor known: A == (alpha + sum z_i u_i(tau) + r delta) G1, u_i(tau) from Lagrange's formula in Python integers"""
    from bn_amd import Fr, G1
    l, (nv, a, b, c, z), system, Z, trap, pk, vk, proof, (r, s) = proved
    alpha, beta, gamma, delta, tau = trap
    u = DC.column_values(a, nv, DC.lagrange_at(tau, 6))
    want = (alpha + sum(zi * ui for zi, ui in zip(z, u)) + r * delta) % FC.R
    assert proof[0] == G1.one() * Fr(want)
    assert vk.alpha_g1 == G1.one() * Fr(alpha) and pk.delta_g1 == G1.one() * Fr(delta)


def test_an_assignment_that_does_not_satisfy_the_system_is_rejected(proved):
    from bn_amd import Fr, groth16
    l, (nv, a, b, c, z), system, Z, trap, pk, vk, proof, _ = proved
    bad = list(z); bad[l + 2] = (bad[l + 2] + 1) % FC.R                         # one private entry changed: the constraints that use it fail
    used = set(a[1]) | set(b[1])
    assert l + 2 in used
    forged = groth16.prove(pk, system, FC.rows(bad), np.random.default_rng(1))
    assert groth16.verify_batch(vk, [forged], [[Fr(v) for v in z[1:l + 1]]]).tolist() == [False]


def test_the_rng_makes_a_proof_reproducible(proved):
    from bn_amd import Fr, groth16
    l, (nv, a, b, c, z), system, Z, trap, pk, vk, proof, _ = proved
    again = groth16.prove(pk, system, Z, np.random.default_rng(600 + l))
    other = groth16.prove(pk, system, Z, np.random.default_rng(601 + l))
    assert again == proof and other[0] != proof[0]
    public = [Fr(v) for v in z[1:l + 1]]
    assert groth16.verify_batch(vk, [proof, other], [public, public]).tolist() == [True, True]
