"""Poseidon hashes and Merkle trees over Fr (bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch, bn254_fr_merkle_tree and their _dev twins),
bn_amd.poseidon and bn_amd.merkle, without a GPU: the six symbols and their declarations in every layer that mirrors the C header, the
argument checks that answer before any device is touched, the level plan of a tree, the Python surface and its errors, bn_amd.merkle over a
stand-in engine that answers from the integer model, and the register budget of the device code - the kernels are template instances of an
existing kernel name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import fr_cases as FC
import poseidon_cases as PC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, FR_IN, FR_OUT, N, INT = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ()), ("int", ())
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_fr_poseidon_batch": [CTX, FR_IN, INT, FR_OUT, N],
    "bn254_fr_poseidon_batch_dev": [CTX, D_IN, INT, D_OUT, N, D_OUT],
    "bn254_fr_poseidon_permute_batch": [CTX, FR_IN, INT, FR_OUT, N],
    "bn254_fr_poseidon_permute_batch_dev": [CTX, D_IN, INT, D_OUT, N, D_OUT],
    "bn254_fr_merkle_tree": [CTX, FR_IN, INT, FR_OUT],
    "bn254_fr_merkle_tree_dev": [CTX, D_IN, INT, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("fr_poseidon", "fr_poseidon_permute", "fr_merkle_level")
HOOKS = ("bn254_fr_poseidon_set_launch_max", "bn254_fr_poseidon_fused_row")
BAD_ARG = -2
R = FC.R


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_poseidon_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_fr_poseidon_fused_row.argtypes = []
    return l


def test_every_new_symbol_resolves():
    """fails on the commit before the family: the library has none of them"""
    from bn_amd import _native
    raw = C.CDLL(str(_native.LIB_PATH))
    for name in NAMES + HOOKS:
        assert getattr(raw, name), name
    assert set(NAMES) <= set(_native.SIGNATURES)
    for name in NAMES:
        assert len(_native.SIGNATURES[name]) == len(EXPECTED[name]), name


def test_header_declares_the_six_entry_points_and_the_limits():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert re.search(r"^#define BN254_POSEIDON_ARITY_MAX 4$", hdr, re.M) and re.search(r"^#define BN254_MERKLE_LOG_MAX 24$", hdr, re.M)
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for name in NAMES:
        assert name in semantics, name
        assert name in threading, name
    assert "bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch and bn254_fr_merkle_tree serialise on the context" in threading
    own = " ".join(hdr[hdr.index("Poseidon hashes and Merkle trees over Fr"):hdr.index("#define BN254_POSEIDON_ARITY_MAX")].split())
    for word in ("R_F = 8", "56 / 57 / 56 / 60", "Grain", str(PC.KNOWN_HASH[(1, 2)]), "permute([0, x_1, .., x_arity])[0]", "row-major", "`out` may be exactly `in`",
                 "must not overlap", "nodes[n - 2]", "hash(child[2 i], child[2 i + 1])", "log_n == 0 writes nothing", "canonical", "2^22", "No workgroup waits".lower(),
                 "n == 0 returns BN254_OK", "BN254_E_BAD_ARG", "n * t > 2^40", "Threading"):
        assert word in own, word
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"fr_poseidon"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)
    src = (ROOT / "bn_amd" / "csrc" / "bn254_poseidon.hip").read_text()
    assert set(re.findall(r'"(fr_\w+)"', src)) == set(SCOPES)


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn fr_poseidon(input: &[Fr], arity: usize) -> Result<Vec<Fr>, GpuError>", "pub fn fr_poseidon_permute(states: &[Fr], t: usize) -> Result<Vec<Fr>, GpuError>",
               "pub fn fr_merkle_tree(leaves: &[Fr]) -> Result<Vec<Fr>, GpuError>"):
        assert fn in txt, fn
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<Fr> fr_poseidon(", "std::vector<Fr> fr_poseidon_permute(", "std::vector<Fr> fr_merkle_tree(", "bn254_fr_poseidon_batch(", "bn254_fr_poseidon_permute_batch(",
              "bn254_fr_merkle_tree("):
        assert s in hpp, s
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        for name in ("bn254_fr_poseidon_batch", "bn254_fr_poseidon_permute_batch", "bn254_fr_merkle_tree"):
            assert name in text, (doc, name)
        for word in ("factored partial rounds", "Poseidon2", "sponge", "arity 4", "several lanes"):          # the "not built" list
            assert word in text, (doc, word)
    assert "bn254_poseidon.hip" in [s.name for s in _native.SOURCES]
    assert (ROOT / "bn_amd" / "csrc" / "poseidon_ops.hpp").exists()
    assert " bn254_poseidon" in (ROOT / "tools" / "build_variant.sh").read_text()
    readme = (ROOT / "README.md").read_text()
    assert "profiles/r18_poseidon.txt" in readme and (ROOT / "profiles" / "r18_poseidon.txt").exists() and (ROOT / "tools" / "time_poseidon.py").exists()


def test_python_surface():
    import bn_amd
    from bn_amd import engine, merkle, poseidon
    for fn, first in ((bn_amd.fr_poseidon_batch, "inputs"), (bn_amd.fr_poseidon_permute_batch, "states"), (bn_amd.fr_merkle_tree, "leaves")):
        assert list(inspect.signature(fn).parameters) == [first, "engine"]
    E = engine.Engine
    assert list(inspect.signature(E.fr_poseidon_batch).parameters) == ["self", "x"]
    assert list(inspect.signature(E.fr_poseidon_permute_batch).parameters) == ["self", "states"]
    assert list(inspect.signature(E.fr_merkle_tree).parameters) == ["self", "leaves"]
    assert list(inspect.signature(E.fr_poseidon_batch_dev).parameters) == ["self", "d_in", "arity", "d_out", "n", "stream"]
    assert list(inspect.signature(E.fr_poseidon_permute_batch_dev).parameters) == ["self", "d_in", "t", "d_out", "n", "stream"]
    assert list(inspect.signature(E.fr_merkle_tree_dev).parameters) == ["self", "d_leaves", "log_n", "d_nodes", "stream"]
    assert (engine.POSEIDON_ARITY_MAX, engine.MERKLE_LOG_MAX) == (4, 24)
    assert list(inspect.signature(merkle.verify).parameters) == ["root", "leaf", "i", "path"]
    assert list(inspect.signature(merkle.verify_batch).parameters) == ["root", "leaves", "indices", "paths", "engine"]
    src = inspect.getsource(merkle.Tree.__init__)
    assert src.count("fr_merkle_tree(") == 1 and "fr_poseidon" not in src
    src = inspect.getsource(merkle.verify_batch)
    assert src.count("fr_poseidon_batch(") == 1 and "hash_host" not in src
    src = inspect.getsource(merkle.verify)
    assert "engine" not in src and "fr_" not in src                                             # host integer arithmetic only
    for word in ("Not built", "arity 4", "several-lanes"):
        assert word in inspect.getdoc(merkle), word
    assert poseidon.hash_host([1, 2]) == PC.KNOWN_HASH[(1, 2)] and poseidon.permute_host([0, 1, 2])[1] == PC.KNOWN_PERMUTE_012_1


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def test_bad_arguments_raise_before_any_device_call_and_name_the_operand():
    import bn_amd
    from bn_amd import merkle, poseidon
    one, nd = bn_amd.Fr.one(), NoDevice()
    with pytest.raises(ValueError, match="^inputs holds 5 records per row, arity = 1..4"):
        bn_amd.fr_poseidon_batch([[one] * 5], engine=nd)
    with pytest.raises(ValueError, match="^rows differ in length"):
        bn_amd.fr_poseidon_batch([[one] * 2, [one]], engine=nd)
    with pytest.raises(ValueError, match="^inputs must have shape"):
        bn_amd.fr_poseidon_batch(np.zeros((4, 2, 3), np.uint64), engine=nd)
    with pytest.raises(ValueError, match="^states holds 1 records per row, t = 2..5"):
        bn_amd.fr_poseidon_permute_batch([[one]], engine=nd)
    with pytest.raises(ValueError, match="^states holds 6 records per row"):
        bn_amd.fr_poseidon_permute_batch([[one] * 6], engine=nd)
    with pytest.raises(ValueError, match="^leaves holds 3 records: a tree needs a power of two"):
        bn_amd.fr_merkle_tree([one] * 3, engine=nd)
    with pytest.raises(ValueError, match="^leaves holds 0 records"):
        merkle.Tree([], engine=nd)
    with pytest.raises(ValueError, match="1 .. 4 inputs, not 5"):
        poseidon.hash([one] * 5, engine=nd)
    with pytest.raises(ValueError, match="1 .. 4 inputs, not 0"):
        poseidon.hash_host([])
    with pytest.raises(ValueError, match="paths differ in length"):
        merkle.verify_batch(one, [one, one], [0, 1], [[one], [one, one]], engine=nd)
    with pytest.raises(ValueError, match="^2 leaves, 1 indices"):
        merkle.verify_batch(one, [one, one], [0], [[one], [one]], engine=nd)
    assert merkle.verify_batch(one, [], [], [], engine=nd) == []


class Model:
    """a stand-in engine that answers from the integer model and records what was asked"""
    def __init__(self): self.calls = []

    @staticmethod
    def _ints(a):
        from bn_amd import Fr
        return [Fr.from_limbs(r).v for r in np.asarray(a, np.uint64).reshape(-1, 4)]

    def fr_merkle_tree(self, leaves):
        self.calls.append("fr_merkle_tree")
        return FC.rows(PC.tree(self._ints(leaves))).reshape(-1, 4)

    def fr_poseidon_batch(self, x):
        x = np.asarray(x, np.uint64)
        self.calls.append(("fr_poseidon_batch", x.shape[0]))
        flat = self._ints(x)
        k = x.shape[1]
        return FC.rows([PC.hash_(flat[i * k:(i + 1) * k]) for i in range(x.shape[0])])


def test_merkle_over_a_stand_in_engine_that_answers_from_the_model():
    from bn_amd import Fr, merkle
    m = Model()
    vals = PC.values(16, 41)
    tree = merkle.Tree([Fr(v) for v in vals], engine=m)
    assert m.calls == ["fr_merkle_tree"] and tree.depth == 4
    nodes = PC.tree(vals)
    assert [x.v for x in tree.nodes] == nodes and tree.root.v == nodes[-1]
    idx = [0, 1, 7, 15]
    paths = [tree.open(i) for i in idx]
    for i, p in zip(idx, paths):
        assert [x.v for x in p] == PC.path(vals, nodes, i)
        assert merkle.verify(tree.root, Fr(vals[i]), i, p)
        assert not merkle.verify(tree.root, Fr(vals[i]), i ^ 2, p) and not merkle.verify(tree.root, Fr(vals[i] + 1), i, p) and not merkle.verify(tree.root, Fr(vals[i]), 16 + i, p)
    m.calls.clear()
    assert merkle.verify_batch(tree.root, [Fr(vals[i]) for i in idx], idx, paths, engine=m) == [True] * 4
    assert m.calls == [("fr_poseidon_batch", 4)] * 4                                             # one call of m hashes per level
    spoiled = [list(p) for p in paths]
    spoiled[1][2] = spoiled[1][2] + Fr.one()
    assert merkle.verify_batch(tree.root, [Fr(vals[0]), Fr(vals[1]), Fr(vals[7] + 1), Fr(vals[15])], [0, 1, 7, 14], spoiled, engine=m) == [True, False, False, False]
    assert merkle.verify_batch(tree.root, [Fr(vals[0])], [16], [paths[0]], engine=m) == [False]
    one = merkle.Tree([Fr(5)], engine=m)
    assert one.root == Fr(5) and one.nodes == [] and one.open(0) == [] and merkle.verify(Fr(5), Fr(5), 0, [])
    with pytest.raises(IndexError):
        tree.open(16)


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


@pytest.mark.parametrize("case, in_, arity, out, n", [
    ("arity zero", DUMMY, 0, DUMMY, 4),
    ("arity five", DUMMY, 5, DUMMY, 4),
    ("arity negative", DUMMY, -1, DUMMY, 4),
    ("arity five without work", DUMMY, 5, DUMMY, 0),
    ("a NULL in", None, 2, DUMMY, 4),
    ("a NULL out", DUMMY, 2, None, 4),
    ("n * t > 2^40", DUMMY, 3, DUMMY, (1 << 38) + 1),
])
def test_hash_argument_errors_answer_without_a_device(lib, case, in_, arity, out, n):
    assert [lib.bn254_fr_poseidon_batch(None, in_, arity, out, n), lib.bn254_fr_poseidon_batch_dev(None, in_, arity, out, n, None)] == [BAD_ARG] * 2, case


@pytest.mark.parametrize("case, in_, t, out, n", [
    ("t one", DUMMY, 1, DUMMY, 4),
    ("t six", DUMMY, 6, DUMMY, 4),
    ("t zero without work", DUMMY, 0, DUMMY, 0),
    ("a NULL in", None, 3, DUMMY, 1),
    ("a NULL out", DUMMY, 3, None, 1),
    ("n * t > 2^40", DUMMY, 5, DUMMY, (1 << 40) // 5 + 1),
])
def test_permute_argument_errors_answer_without_a_device(lib, case, in_, t, out, n):
    assert [lib.bn254_fr_poseidon_permute_batch(None, in_, t, out, n), lib.bn254_fr_poseidon_permute_batch_dev(None, in_, t, out, n, None)] == [BAD_ARG] * 2, case


@pytest.mark.parametrize("case, leaves, log_n, nodes", [
    ("log_n negative", DUMMY, -1, DUMMY),
    ("log_n 25", DUMMY, 25, DUMMY),
    ("NULL leaves", None, 3, DUMMY),
    ("NULL nodes", DUMMY, 1, None),
])
def test_tree_argument_errors_answer_without_a_device(lib, case, leaves, log_n, nodes):
    assert [lib.bn254_fr_merkle_tree(None, leaves, log_n, nodes), lib.bn254_fr_merkle_tree_dev(None, leaves, log_n, nodes, None)] == [BAD_ARG] * 2, case


def test_no_work_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 8)(*([7] * 8))
    for p in (None, DUMMY):
        for arity in (1, 4):
            assert [lib.bn254_fr_poseidon_batch(None, p, arity, out, 0), lib.bn254_fr_poseidon_batch_dev(None, p, arity, out, 0, None)] == [0, 0]
            assert [lib.bn254_fr_poseidon_permute_batch(None, p, arity + 1, None, 0), lib.bn254_fr_poseidon_permute_batch_dev(None, p, arity + 1, None, 0, None)] == [0, 0]
        assert [lib.bn254_fr_merkle_tree(None, p, 0, out), lib.bn254_fr_merkle_tree_dev(None, p, 0, None, None)] == [0, 0]       # one leaf: it is the root
    assert list(out) == [7] * 8


def test_the_checks_of_host_plan_agree_with_the_entry_points():
    import hostsim_poseidon_lib as HP
    sim = HP.lib()
    assert [sim.hsp_poseidon_check(0x1000, t, 0x1000, 1) for t in (1, 2, 5, 6)] == [BAD_ARG, 0, 0, BAD_ARG]
    assert sim.hsp_poseidon_check(0x1000, 4, 0x1000, 1 << 38) == 0 and sim.hsp_poseidon_check(0x1000, 4, 0x1000, (1 << 38) + 1) == BAD_ARG
    assert [sim.hsp_merkle_check(0x1000, l, 0x1000) for l in (-1, 0, 24, 25)] == [BAD_ARG, 0, 0, BAD_ARG]
    assert sim.hsp_merkle_check(None, 0, None) == 0 and sim.hsp_merkle_check(None, 1, 0x1000) == BAD_ARG


def test_the_level_plan_of_a_tree():
    """counts and offsets for log_n = 0, 1, 2, 24, and the cut into sub-launches of at most 2^22 lanes"""
    import hostsim_poseidon_lib as HP
    assert HP.merkle_plan(0).tolist() == []
    assert HP.merkle_plan(1).tolist() == [[1, 0, 0, 1, 1]]                                       # (cnt, src, dst, parts, from_leaves)
    assert HP.merkle_plan(2).tolist() == [[2, 0, 0, 1, 1], [1, 0, 2, 1, 0]]
    assert HP.merkle_plan(3, step=3).tolist() == [[4, 0, 0, 2, 1], [2, 0, 4, 1, 0], [1, 4, 6, 1, 0]]
    plan = HP.merkle_plan(24)
    n = 1 << 24
    assert len(plan) == 24 and plan[:, 0].tolist() == [n >> (l + 1) for l in range(24)]
    assert plan[:, 2].tolist() == [n - (n >> l) for l in range(24)] and plan[1:, 1].tolist() == plan[:-1, 2].tolist()
    assert plan[-1, 2] == n - 2 and plan[:, 4].tolist() == [1] + [0] * 23
    assert plan[:, 3].tolist() == [2, 1] + [1] * 22                                              # 2^23 parents are two sub-launches of 2^22


def test_the_hooks_check_their_bounds(lib):
    try:
        assert lib.bn254_fr_poseidon_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_fr_poseidon_set_launch_max(20) == 0
    finally:
        assert lib.bn254_fr_poseidon_set_launch_max(0) == 0
    assert lib.bn254_fr_poseidon_fused_row() in (0, 1)


def test_the_kernels_are_instances_of_fr_decode_k_and_spill_nothing():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    import lane_shell
    lane_shell.unit_source("bn254_poseidon.hip")  # the unit adds no kernel under any other name: the shell is lane_launch.hpp's
    ops = (ROOT / "bn_amd" / "csrc" / "poseidon_ops.hpp").read_text()
    assert ops.count("#pragma unroll 1") == 3                                                   # full, partial, full: the rounds stay loops
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    meta = kernel_meta.instances(so)
    mine = [n for n in meta if kernel_meta.short_name(n) == "bn254_fr_decode_k" and re.search(r"\d+FrPoseidonOp(E|I)", n)]
    assert len(mine) == 4, mine                                                                 # one instance per width: hash and permutation share it
    for n in mine:
        assert meta[n]["spill"] == 0 and meta[n]["private"] == 0 and meta[n]["lds"] == 0, (n, meta[n])
