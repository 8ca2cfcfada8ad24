"""The quotients of a multilinear opening (bn254_fr_mle_quotients and its _dev twin), bn_amd.mle.quotients and bn_amd.mkzg, without a GPU: the
two declarations in every layer that mirrors the C header, the argument checks that answer before any device is touched, the profiling
scope, the Python surface and its errors, the test hooks, mle.quotients and mkzg's call sequence over a stand-in engine, and the register
budget of the device code - the kernels are further template instances of an existing kernel name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import fr_cases as FC
import mle_open_cases as OC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, FR_IN, FR_OUT, INT, D_IN, D_OUT = ("void", MUT), ("fr", CONST), ("fr", MUT), ("int", ()), ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_fr_mle_quotients": [CTX, FR_IN, INT, FR_IN, FR_OUT],
    "bn254_fr_mle_quotients_dev": [CTX, D_IN, INT, FR_IN, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPE = "fr_mle_quotients"
HOOKS = ("bn254_fr_mle_quotients_levels", "bn254_fr_mle_quotients_set_levels")
BAD_ARG = -2
R = FC.R


def test_header_declares_the_two_entry_points_and_documents_them():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
        assert decls[name]["params"][-1][0] == ("stream" if name.endswith("_dev") else "out")
    hdr = B.HEADER.read_text()
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for name in NAMES:
        assert name in semantics and name in threading, name
    assert "bn254_fr_mle_quotients serialises on the context" in threading
    own = " ".join(hdr[hdr.index("The quotients of a multilinear opening"):hdr.index("int bn254_fr_mle_quotients(")].split())
    for word in ("bit j of i", "MOST significant", "canonical", "q_j[i] = t[i + half] - t[i]", "t[i] = t[i] + z[j] * q_j[i]", "out[0] = f(z)", "out[2^j + i] = q_j[i]",
                 "nv == 0 copies", "HOST", "never written", "must NOT overlap", "aliasing is not supported", "BN254_E_BAD_ARG", "No LDS, no atomics", "Threading"):
        assert word in own, word
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook


def test_the_scope_name_is_documented_and_used():
    hdr = B.HEADER.read_text()
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    names = re.findall(r'"(\w+)"', block)
    assert names.count(SCOPE) == 1 and len(names) == len(set(names))
    unit = (ROOT / "bn_amd" / "csrc" / "bn254_mle.hip").read_text() + (ROOT / "bn_amd" / "csrc" / "mle_ops.hpp").read_text()
    assert '"%s"' % SCOPE in unit and "BnScope sc(c, s, FR_MLE_QUOT_SCOPE)" in unit


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    for name in NAMES:
        assert len(_native.SIGNATURES[name]) == len(EXPECTED[name]), name
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    assert "pub fn fr_mle_quotients(a: &[Fr], z: &[Fr]) -> Result<Vec<Fr>, GpuError>" in txt
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    assert "std::vector<Fr> fr_mle_quotients(" in hpp and "bn254_fr_mle_quotients(" in hpp
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        assert "bn254_fr_mle_quotients" in text and "mkzg" in text, doc
    assert (ROOT / "tools" / "time_mle_open.py").exists()
    assert "mkzg" in inspect.getdoc(__import__("bn_amd").sumcheck)


def test_python_surface():
    import bn_amd
    from bn_amd import engine, mkzg, mle
    assert list(inspect.signature(bn_amd.fr_mle_quotients).parameters) == ["a", "z", "engine"]
    E = engine.Engine
    assert list(inspect.signature(E.fr_mle_quotients).parameters) == ["self", "a", "z"]
    assert list(inspect.signature(E.fr_mle_quotients_dev).parameters) == ["self", "d_a", "z", "d_out", "stream"]
    assert list(inspect.signature(mle.quotients).parameters)[:2] == ["table", "point"]
    assert mkzg.SRS._fields == ("nv", "g1_levels", "g2_one", "tau_g2")
    assert list(inspect.signature(mkzg.setup).parameters)[:2] == ["nv", "rng"]
    assert list(inspect.signature(mkzg.commit).parameters)[:2] == ["srs", "table"]
    assert list(inspect.signature(mkzg.open).parameters)[:3] == ["srs", "table", "point"]
    assert list(inspect.signature(mkzg.verify_batch).parameters)[:5] == ["srs", "cs", "points", "ys", "proofs"]
    assert list(inspect.signature(mkzg.verify).parameters)[:5] == ["srs", "c", "point", "y", "proofs"]
    assert "TESTS AND DEVELOPMENT ONLY" in inspect.getdoc(mkzg.setup) and "_draw(rng)" in inspect.getsource(mkzg.setup)
    src = inspect.getsource(mkzg.setup)
    assert src.count("fr_mle_eq(") == 1 and src.count("g1_mul_base_batch(") == 1 and src.count("g2_mul_base_batch(") == 1
    src = inspect.getsource(mkzg.open)
    assert src.count("fr_mle_quotients(") == 1 and src.count("g1_msm_batch(") == 1
    src = inspect.getsource(mkzg.verify_batch)
    assert src.count("g1_msm_batch(") == 1 and src.count("g1_add_batch(") == 1 and src.count("pairing_check_batch(") == 1 and "e.g2_" not in src                # nothing is computed in G2
    for word in ("Not built", "random linear combination", "Zeromorph", "bucket-method"):
        assert word in inspect.getdoc(mkzg), word


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def _srs(nv):
    """a reference string of the right shapes and no content: the errors below are answered before it is read"""
    from bn_amd import G2, mkzg
    return mkzg.SRS(nv, np.zeros((2 << nv, 12), np.uint64), G2.one(), [G2.one()] * nv)


def test_bad_arguments_raise_before_any_device_call_and_name_the_operand():
    import bn_amd
    from bn_amd import G1, mkzg, mle
    one, g = bn_amd.Fr.one(), G1.one()
    nd = NoDevice()
    with pytest.raises(ValueError, match="^a holds 3 values but z has 2 variables"):
        bn_amd.fr_mle_quotients([one] * 3, [one] * 2, engine=nd)
    with pytest.raises(ValueError, match="^a holds 0 values but z has 0 variables"):
        bn_amd.fr_mle_quotients([], [], engine=nd)
    with pytest.raises(ValueError, match="^z holds 31 variables"):
        bn_amd.fr_mle_quotients([one] * 2, [one] * 31, engine=nd)
    with pytest.raises(ValueError, match="^a holds 4 values but z has 1 variables"):
        mle.quotients([one] * 4, [one], engine=nd)
    srs = _srs(2)
    with pytest.raises(ValueError, match="^the table holds 3 values: a multilinear polynomial has a power of two"):
        mkzg.commit(srs, [one] * 3, engine=nd)
    with pytest.raises(ValueError, match="^the table holds 0 values"):
        mkzg.commit(srs, [], engine=nd)
    with pytest.raises(ValueError, match="^the table holds 8 values but the reference string is for 2 variables"):
        mkzg.commit(srs, [one] * 8, engine=nd)
    with pytest.raises(ValueError, match="^the table holds 8 values but the reference string"):
        mkzg.open(srs, [one] * 8, [one] * 3, engine=nd)
    with pytest.raises(ValueError, match="^a holds 4 values but z has 1 variables"):
        mkzg.open(srs, [one] * 4, [one], engine=nd)
    with pytest.raises(ValueError, match="^2 commitments, 1 points, 2 values and 2 lists of proofs"):
        mkzg.verify_batch(srs, [g, g], [[one]], [one, one], [[g], [g]], engine=nd)
    with pytest.raises(ValueError, match="^1 commitments, 1 points, 0 values"):
        mkzg.verify_batch(srs, [g], [[one]], [], [[g]], engine=nd)
    with pytest.raises(ValueError, match="^opening 1: the point has 2 variables but 1 proofs"):
        mkzg.verify_batch(srs, [g, g], [[one], [one, one]], [one, one], [[g], [g]], engine=nd)
    with pytest.raises(ValueError, match="^opening 0: the point has 3 variables but the reference string is for 2"):
        mkzg.verify_batch(srs, [g], [[one] * 3], [one], [[g] * 3], engine=nd)
    with pytest.raises(ValueError, match="nv >= 0"):
        mkzg.setup(-1, np.random.default_rng(0), engine=nd)
    assert mkzg.verify_batch(srs, [], [], [], [], engine=nd).shape == (0,)


class Model:
    """a stand-in engine that answers the field call from the integer model, the group calls with zeros, and records what was asked"""
    def __init__(self): self.calls = []

    def fr_mle_quotients(self, a, z):
        from bn_amd import Fr
        ints = lambda x: [Fr.from_limbs(r).v for r in np.asarray(x, np.uint64).reshape(-1, 4)]
        self.calls.append(("fr_mle_quotients", len(a)))
        return FC.rows(OC.quotients(ints(a), ints(z)))

    def g1_msm(self, p, k):
        self.calls.append(("g1_msm", p.shape[0], k.shape[0]))
        return np.zeros(12, np.uint64)

    def g1_msm_batch(self, p, k, offsets):
        self.calls.append(("g1_msm_batch", p.shape[0], k.shape[0], [int(o) for o in offsets]))
        self.last = (p, k)
        return np.zeros((len(offsets) - 1, 12), np.uint64)


def test_mle_quotients_over_a_stand_in_engine_that_answers_from_the_model():
    from bn_amd import Fr, mle
    m = Model()
    table, z = OC.values(16, 61), OC.point(4, 62)
    y, qs = mle.quotients([Fr(v) for v in table], [Fr(v) for v in z], engine=m)
    assert m.calls == [("fr_mle_quotients", 16)]
    want_y, want_qs = OC.split(OC.quotients(table, z))
    assert y == Fr(want_y) and [[q.v for q in qj] for qj in qs] == want_qs and [len(q) for q in qs] == [1, 2, 4, 8]
    y, qs = mle.quotients(FC.rows(table), [Fr(v) for v in z], limbs=True, engine=m)
    assert y == Fr(want_y) and [q.shape for q in qs] == [(1, 4), (2, 4), (4, 4), (8, 4)] and qs[3].tobytes() == FC.rows(want_qs[3]).tobytes()
    assert mle.quotients([Fr(9)], [], engine=m) == (Fr(9), [])


def test_mkzg_open_hands_the_heap_to_one_segmented_sum_without_a_copy():
    """segment j of the one g1_msm_batch is records [2^j, 2^(j+1)) of the quotients against the same rows of the reference string, both as
    views; commit takes level m"""
    from bn_amd import Fr, mkzg
    srs = _srs(4)
    srs.g1_levels[:, 0] = np.arange(32)                                                        # row numbers, to recognise the slices
    m = Model()
    table, z = OC.values(8, 63), OC.point(3, 64)
    y, proofs = mkzg.open(srs, FC.rows(table), [Fr(v) for v in z], engine=m)
    assert [c[0] for c in m.calls] == ["fr_mle_quotients", "g1_msm_batch"] and m.calls[1][1:] == (7, 7, [0, 1, 3, 7])
    p, k = m.last
    assert np.shares_memory(p, srs.g1_levels) and list(p[:, 0]) == list(range(1, 8)) and k.base is not None
    assert k.tobytes() == FC.rows(OC.quotients(table, z)[1:]).tobytes()
    assert y == Fr(OC.evaluate(table, z)) and len(proofs) == 3
    m = Model()
    assert mkzg.open(srs, [Fr(5)], [], engine=m) == (Fr(5), []) and [c[0] for c in m.calls] == ["fr_mle_quotients"]
    m = Model()
    mkzg.commit(srs, FC.rows(table), engine=m)
    assert m.calls == [("g1_msm", 8, 8)]


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_mle_quotients_levels.argtypes = []; l.bn254_fr_mle_quotients_levels.restype = C.c_uint
    l.bn254_fr_mle_quotients_set_levels.argtypes = [C.c_uint]
    return l


BUF = (C.c_uint64 * 64)()        # 16 records; never dereferenced: every case below is answered before the data is read
BASE = C.addressof(BUF)
DUMMY, FAR = C.c_void_p(0x1000), C.c_void_p(0x1000000)


@pytest.mark.parametrize("case, a, nv, z, out", [
    ("nv below zero", DUMMY, -1, DUMMY, FAR),
    ("nv above the limit", DUMMY, 31, DUMMY, FAR),
    ("a NULL a", None, 3, DUMMY, FAR),
    ("a NULL a without variables", None, 0, None, FAR),
    ("a NULL out", DUMMY, 3, DUMMY, None),
    ("a NULL z with variables", DUMMY, 1, None, FAR),
    ("out is a", C.c_void_p(BASE), 2, DUMMY, C.c_void_p(BASE)),
    ("out is a without variables", C.c_void_p(BASE), 0, None, C.c_void_p(BASE)),
    ("out starts inside a", C.c_void_p(BASE), 2, DUMMY, C.c_void_p(BASE + 96)),
    ("a starts inside out", C.c_void_p(BASE + 32), 2, DUMMY, C.c_void_p(BASE)),
    ("out starts in the last bytes of a", C.c_void_p(BASE), 3, DUMMY, C.c_void_p(BASE + 255)),
])
def test_argument_errors_answer_without_a_device(lib, case, a, nv, z, out):
    assert [lib.bn254_fr_mle_quotients(None, a, nv, z, out), lib.bn254_fr_mle_quotients_dev(None, a, nv, z, out, None)] == [BAD_ARG] * 2, case


def test_the_check_accepts_neighbouring_buffers():
    """the same check through the host simulation, which has no device to fall back on: buffers that touch but do not overlap pass"""
    import hostsim_mle_open_lib as HO
    chk = HO.lib().hso_check
    assert chk(BASE, 2, 0x1000, BASE + 128) == 0 and chk(BASE + 128, 2, 0x1000, BASE) == 0 and chk(BASE, 0, None, BASE + 32) == 0
    assert chk(BASE, 2, 0x1000, BASE + 127) == BAD_ARG and chk(BASE + 127, 2, 0x1000, BASE) == BAD_ARG and chk(BASE, 30, 0x1000, BASE + (32 << 30) - 1) == BAD_ARG
    assert chk(BASE, 30, 0x1000, BASE + (32 << 30)) == 0


def test_the_hooks_check_their_bounds(lib):
    rho = lib.bn254_fr_mle_quotients_levels()
    assert rho in (1, 2, 3, 4)
    try:
        assert lib.bn254_fr_mle_quotients_set_levels(5) == BAD_ARG
        for v in (1, 2, 3, 4):
            assert lib.bn254_fr_mle_quotients_set_levels(v) == 0
    finally:
        assert lib.bn254_fr_mle_quotients_set_levels(0) == 0
    assert lib.bn254_fr_mle_quotients_levels() == rho


def test_the_kernels_are_instances_of_fr_decode_k_and_spill_nothing():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    import lane_shell
    lane_shell.unit_source("bn254_mle.hip")  # the unit adds no kernel under any other name: the shell is lane_launch.hpp's
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    meta = kernel_meta.instances(so)
    mine = {int(m.group(1)): n for n in meta if kernel_meta.short_name(n) == "bn254_fr_decode_k" for m in [re.search(r"\d+FrMleQuotOpILi(\d+)E", n)] if m}
    assert sorted(mine) == [1, 2, 3, 4], mine                                                   # one instance per number of levels
    for rho, n in mine.items():
        assert meta[n]["spill"] == 0 and meta[n]["private"] == 0 and meta[n]["lds"] == 0, (rho, meta[n])
