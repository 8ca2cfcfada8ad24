"""Sparse linear maps over Fr (bn254_fr_dot_batch and its _dev twin) and the Groth16 prover on top of them, without a GPU: the two
declarations in every layer that mirrors the C header, the argument checks that answer before any device is touched, the placement of the
profiling scopes, the Python surface and its errors, the test hooks, and the register budget of the device code - the kernels are template
instances of an existing kernel name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import dot_cases as DC
import fr_cases as FC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST = ("const",)
MUT = ("mut",)
CTX, FR_IN, FR_OUT, N = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ())
D_IN, D_OUT, OFF, IDX = ("void", CONST), ("void", MUT), ("usize", CONST), ("u64", CONST)
EXPECTED = {
    "bn254_fr_dot_batch": [CTX, FR_IN, IDX, FR_IN, N, OFF, N, FR_OUT],
    "bn254_fr_dot_batch_dev": [CTX, D_IN, D_IN, D_IN, N, OFF, N, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("fr_dot", "fr_dot_fold")
OPS = ("FrDotOp", "FrDotFoldOp")
HOOKS = ("bn254_fr_dot_piece", "bn254_fr_dot_fan", "bn254_fr_dot_set_launch_max", "bn254_fr_dot_set_piece")
BAD_ARG = -2


def test_header_declares_the_two_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    for name in NAMES:
        assert name in semantics, name
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_fr_dot_batch serialises on the context" in threading and "bn254_fr_dot_batch_dev" in threading
    own = " ".join(hdr[hdr.index("Sparse linear maps over Fr"):hdr.index("int bn254_fr_dot_batch(")].split())
    for word in ("out[j] = sum over t in [offsets[j], offsets[j+1]) of coeff[t] * x[index[t]]", "index == NULL", "Fr::zero()", "canonical", "HOST", "may not overlap",
                 "BN254_E_BAD_ARG", "2^40", "never a wrong sum", "ceil(log16(ceil(L / 4)))", "Threading"):
        assert word in own, word
    dev = " ".join(hdr[hdr.index("/* bn254_fr_dot_batch on device-resident"):hdr.index("int bn254_fr_dot_batch_dev(")].split())
    for word in ("cannot be read on the host, so it is NOT checked", "outside the contract, but memory safe", "contributes zero", "may be freed on return"):
        assert word in dev, word


def test_no_new_type_and_no_new_option():
    hdr = B.HEADER.read_text()
    assert "uint32_t" not in B._strip_c_comments(hdr)
    assert "dot" not in "".join(re.findall(r"typedef[^;]*;", hdr))
    assert B.c_enum("BN254_OPT_")["COUNT_"] == 16
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook


def test_the_scope_names_sit_between_the_pinned_lines():
    hdr = B.HEADER.read_text()
    parent = re.search(r'/\* kernel: ("miller".*?"g2_eq"\.)\n', hdr)
    assert parent, "the first line of the block is the one the earlier tests pin"
    assert "fr_dot" not in parent.group(1)
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    lines = block.split("\n")
    mine = [i for i, l in enumerate(lines) if '"fr_dot"' in l]
    ntt = [i for i, l in enumerate(lines) if '"ntt"' in l]
    assert len(mine) == 1 and len(ntt) == 1 and 0 < mine[0] < ntt[0]
    assert re.findall(r'"(\w+)"', lines[mine[0]]) == list(SCOPES)                               # a line of their own
    names = re.findall(r'"(\w+)"', block)
    assert tuple(names[-2:]) == ("ntt", "ntt_table") and len(names) == len(set(names))
    for s in SCOPES:
        assert names.count(s) == 1
    src = (ROOT / "bn_amd" / "csrc" / "bn254_dot.hip").read_text()
    assert set(re.findall(r'"(fr_\w+)"', src)) == set(SCOPES)
    assert "dot" not in (ROOT / "bn_amd" / "csrc" / "bn254_fr.hip").read_text()


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    for name in NAMES:
        assert len(_native.SIGNATURES[name]) == len(EXPECTED[name]), name
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    assert "pub fn fr_dot(coeff: &[Fr], index: Option<&[u64]>, x: &[Fr], offsets: &[usize]) -> Result<Vec<Fr>, GpuError>" in txt
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<Fr> fr_dot(", "bn254_fr_dot_batch("):
        assert s in hpp, s
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "bn254_fr_dot_batch" in (ROOT / doc).read_text(), doc
    assert "bn254_dot.hip" in [s.name for s in _native.SOURCES]
    assert (ROOT / "bn_amd" / "csrc" / "dot_ops.hpp").exists()
    assert " bn254_dot" in (ROOT / "tools" / "build_variant.sh").read_text()


def test_python_surface():
    import bn_amd
    from bn_amd import engine, groth16
    assert list(inspect.signature(bn_amd.fr_dot_batch).parameters) == ["coeff", "x", "offsets", "index", "engine"]
    E = engine.Engine
    assert list(inspect.signature(E.fr_dot_batch).parameters) == ["self", "coeff", "x", "offsets", "index"]
    assert inspect.signature(E.fr_dot_batch).parameters["index"].default is None
    assert list(inspect.signature(E.fr_dot_batch_dev).parameters) == ["self", "d_coeff", "d_index", "d_x", "nx", "offsets", "m", "d_out", "stream"]
    assert groth16.R1CS._fields == ("num_public", "num_variables", "a", "b", "c")
    assert groth16.ProvingKey._fields == ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2", "a_query", "b_g1_query", "b_g2_query", "l_query", "h_query")
    assert groth16.VerifyingKey._fields == ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "ic")
    assert list(inspect.signature(groth16.witness_map).parameters) == ["r1cs", "z", "engine"]
    assert list(inspect.signature(groth16.setup).parameters) == ["r1cs", "rng", "engine"]
    assert list(inspect.signature(groth16.prove).parameters) == ["pk", "r1cs", "z", "rng", "engine"]
    assert inspect.getsource(groth16.witness_map).count("fr_dot_batch(") == 1
    src = inspect.getsource(groth16.setup)
    assert src.count("fr_dot_batch(") == 1 and src.count("fr_ntt_batch(") == 1 and "inverse=True" in src
    assert src.count("g1_mul_base_batch(") == 1 and src.count("g2_mul_base_batch(") == 1
    assert "tests and development" in groth16.setup.__doc__.lower() and "ceremony" in groth16.setup.__doc__
    src = inspect.getsource(groth16.prove)
    assert src.count("e.g1_msm(") == 4 and src.count("e.g2_msm(") == 1 and src.count("poly.quotient(") == 2      # one of them in the docstring
    assert "does not verify" in " ".join(groth16.prove.__doc__.split())


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def _system(l=2):
    from bn_amd import groth16
    l, nv, a, b, c, z = DC.r1cs(5, l, [0, 1, 3], seed=1)
    mat = lambda m: (np.array(m[0], np.uint64), np.array(m[1], np.uint64), FC.rows(m[2]))
    return groth16.R1CS(l, nv, mat(a), mat(b), mat(c)), FC.rows(z)


def test_bad_arguments_raise_before_any_device_call():
    import bn_amd
    from bn_amd import groth16
    Fr = bn_amd.Fr
    one = [Fr.one()]
    dot = lambda *a, **k: bn_amd.fr_dot_batch(*a, engine=NoDevice(), **k)
    for offsets in ([1, 3], [0, 2, 1, 3], [0, 2], [0, 4], []):
        with pytest.raises(ValueError, match="offsets"):
            dot(one * 3, one * 3, offsets)
    with pytest.raises(ValueError, match="one to one"):
        dot(one * 3, one * 4, [0, 3])
    for index in ([0, 1], [0, 1, 2, 0]):
        with pytest.raises(ValueError, match="index"):
            dot(one * 3, one * 4, [0, 3], index=index)
    for index in ([0, 1, 4], [0, -1, 2], [0, 1 << 40, 2]):
        with pytest.raises(ValueError, match="out of range"):
            dot(one * 3, one * 4, [0, 3], index=index)
    with pytest.raises(ValueError, match="out of range"):
        dot(np.zeros((3, 4), np.uint64), np.zeros((0, 4), np.uint64), [0, 3], index=np.zeros(3, np.uint64))
    system, z = _system()
    for f in (lambda zz: groth16.witness_map(system, zz, engine=NoDevice()), lambda zz: groth16.prove(None, system, zz, None, engine=NoDevice())):
        with pytest.raises(ValueError, match="variables"):
            f(z[:-1])
        with pytest.raises(ValueError, match="constant one"):
            f(np.concatenate([FC.rows([2]), z[1:]]))
    short = system._replace(b=(system.b[0][:-1], system.b[1][:int(system.b[0][-2])], system.b[2][:int(system.b[0][-2])]))
    with pytest.raises(ValueError, match="number of rows"):
        groth16.witness_map(short, z, engine=NoDevice())
    with pytest.raises(ValueError, match="CSR"):
        groth16.witness_map(system._replace(a=(system.a[0] + np.uint64(1), system.a[1], system.a[2])), z, engine=NoDevice())
    with pytest.raises(ValueError, match="column"):
        groth16.witness_map(system._replace(num_variables=system.num_variables - 1), z[:-1], engine=NoDevice())


def test_witness_map_stacks_the_three_matrices_into_one_call():
    """a stand-in engine that answers from the Python-integer model: ONE call of 3 * rows segments, the result cut and padded to the domain"""
    from bn_amd import groth16
    l, nv, a, b, c, z = DC.r1cs(5, 2, [0, 1, 3], seed=1)
    system, Z = _system()
    calls = []

    class Model:
        def fr_dot_batch(self, coeff, x, offsets, index=None):
            calls.append((len(coeff), len(offsets) - 1))
            assert np.array_equal(x, Z)
            stacked = [v for m in (a, b, c) for v in m[2]]
            assert np.array_equal(coeff, FC.rows(stacked))
            return FC.rows(DC.model(stacked, z, offsets, index))
    ev = groth16.witness_map(system, Z, engine=Model())
    assert calls == [(len(a[2]) + len(b[2]) + len(c[2]), 15)]
    for got, mat in zip(ev, (a, b, c)):
        assert got.shape == (8, 4) and not got[5:].any()
        assert np.array_equal(got[:5], FC.rows(DC.model(mat[2], z, mat[0], mat[1])))
    az, bz, cz = (DC.model(m[2], z, m[0], m[1]) for m in (a, b, c))
    assert [x * y % FC.R for x, y in zip(az, bz)] == cz                                         # the generated assignment satisfies the system


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_dot_piece.argtypes = []; l.bn254_fr_dot_piece.restype = C.c_uint
    l.bn254_fr_dot_fan.argtypes = []; l.bn254_fr_dot_fan.restype = C.c_uint
    l.bn254_fr_dot_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_fr_dot_set_piece.argtypes = [C.c_uint]
    return l


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


def _off(*v):
    return (C.c_size_t * len(v))(*v)


def _both(lib, coeff, index, x, nx, offsets, m, out):
    return [lib.bn254_fr_dot_batch(None, coeff, index, x, nx, offsets, m, out), lib.bn254_fr_dot_batch_dev(None, coeff, index, x, nx, offsets, m, out, None)]


@pytest.mark.parametrize("case, coeff, x, nx, offsets, m, out", [
    ("offsets == NULL with m > 0", DUMMY, DUMMY, 3, None, 2, DUMMY),
    ("offsets[0] != 0", DUMMY, DUMMY, 3, _off(1, 2, 3), 2, DUMMY),
    ("decreasing offsets", DUMMY, DUMMY, 3, _off(0, 4, 3), 2, DUMMY),
    ("n > 2^40", DUMMY, DUMMY, (1 << 40) + 1, _off(0, (1 << 40) + 1), 1, DUMMY),
    ("NULL coeff with n > 0", None, DUMMY, 3, _off(0, 1, 3), 2, DUMMY),
    ("NULL x with n > 0", DUMMY, None, 3, _off(0, 1, 3), 2, DUMMY),
    ("NULL out", DUMMY, DUMMY, 3, _off(0, 1, 3), 2, None),
    ("NULL out, only empty segments", None, None, 0, _off(0, 0, 0), 2, None),
    ("index == NULL with nx != n", DUMMY, DUMMY, 4, _off(0, 1, 3), 2, DUMMY),
    ("index == NULL with nx != n", DUMMY, DUMMY, 2, _off(0, 1, 3), 2, DUMMY),
])
def test_argument_errors_answer_without_a_device(lib, case, coeff, x, nx, offsets, m, out):
    assert _both(lib, coeff, None, x, nx, offsets, m, out) == [BAD_ARG] * 2, case


def test_an_index_out_of_range_is_rejected_by_the_host_form_without_a_device(lib):
    for bad in (2, 1 << 63):
        index = (C.c_uint64 * 3)(0, bad, 1)
        assert lib.bn254_fr_dot_batch(None, DUMMY, index, DUMMY, 2, _off(0, 1, 3), 2, DUMMY) == BAD_ARG
    # with an index the length of x is free, but the other checks still come first
    index = (C.c_uint64 * 3)(0, 1, 1)
    assert _both(lib, DUMMY, index, DUMMY, 2, _off(0, 4, 3), 2, DUMMY) == [BAD_ARG] * 2
    assert _both(lib, DUMMY, index, DUMMY, 2, _off(0, 1, 3), 2, None) == [BAD_ARG] * 2


def test_an_empty_call_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 8)(*([7] * 8))
    for p in (None, DUMMY):                                                                   # m == 0 is answered before the arguments
        for offsets in (None, _off(5)):
            assert _both(lib, p, None, p, 9, offsets, 0, out) == [0] * 2 and _both(lib, p, p, p, 0, offsets, 0, None) == [0] * 2
    assert list(out) == [7] * 8


def test_the_hooks_check_their_bounds(lib):
    P, F = lib.bn254_fr_dot_piece(), lib.bn254_fr_dot_fan()
    assert P in (4, 8, 16, 32) and F in (2, 4, 16)                                              # the ones the host simulation runs
    try:
        assert lib.bn254_fr_dot_set_piece(65) == BAD_ARG and lib.bn254_fr_dot_set_piece(4) == 0 and lib.bn254_fr_dot_set_piece(32) == 0
        assert lib.bn254_fr_dot_set_launch_max((1 << 22) + 1) == BAD_ARG
        assert lib.bn254_fr_dot_set_launch_max(20) == 0
    finally:
        assert lib.bn254_fr_dot_set_piece(0) == 0 and lib.bn254_fr_dot_set_launch_max(0) == 0
    assert lib.bn254_fr_dot_piece() == P


def test_the_kernels_are_instances_of_fr_decode_k_and_spill_nothing():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    # the unit adds no kernel under any other name
    import lane_shell
    lane_shell.unit_source("bn254_dot.hip")      # the unit adds no kernel of its own: the shell is lane_launch.hpp's
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    meta = kernel_meta.instances(so)
    for op in OPS:
        mine = [n for n in meta if kernel_meta.short_name(n) == "bn254_fr_decode_k" and re.search(r"\d+" + op + "E", n)]
        assert len(mine) == 1, op
        assert meta[mine[0]]["spill"] == 0 and meta[mine[0]]["private"] == 0 and meta[mine[0]]["lds"] == 0, (op, meta[mine[0]])
