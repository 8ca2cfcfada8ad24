"""Wide Poseidon over Fr (bn254_fr_poseidon_ex_batch, bn254_fr_poseidon_chain_batch and their _dev twins), bn_amd.poseidon.hash_ex / hash_chain and
bn_amd.merkle.Tree.from_records, without a GPU: the four symbols and their declarations in every layer that mirrors the C header, the header's
text, the argument checks that answer before any device is touched, the internal table hook against the Python derivation, the Python surface
and its errors, Tree.from_records over a stand-in engine, and the register budget of the device code - the kernels are template instances of
an existing kernel name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import fr_cases as FC
import poseidon_cases as PC
import poseidon_wide_cases as WC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, FR_IN, FR_OUT, N, INT, OFF = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ()), ("int", ()), ("usize", CONST)
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_fr_poseidon_ex_batch": [CTX, FR_IN, INT, FR_IN, INT, FR_OUT, N],
    "bn254_fr_poseidon_ex_batch_dev": [CTX, D_IN, INT, D_IN, INT, D_OUT, N, D_OUT],
    "bn254_fr_poseidon_chain_batch": [CTX, FR_IN, OFF, N, INT, FR_OUT],
    "bn254_fr_poseidon_chain_batch_dev": [CTX, D_IN, OFF, N, INT, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("fr_poseidon_ex", "fr_poseidon_chain")
HOOKS = ("bn254_fr_poseidon_wide_table", "bn254_fr_poseidon_wide_lanes", "bn254_fr_poseidon_wide_block", "bn254_fr_poseidon_wide_set_launch_max")
BAD_ARG = -2
R = FC.R


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_poseidon_wide_table.argtypes = [C.c_int, C.c_void_p]
    l.bn254_fr_poseidon_wide_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_fr_poseidon_wide_lanes.argtypes = []
    l.bn254_fr_poseidon_wide_block.argtypes = []
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


def test_header_declares_the_four_entry_points_and_documents_them():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert re.search(r"^#define BN254_POSEIDON_EX_INPUTS_MAX 16$", hdr, re.M) and re.search(r"^#define BN254_POSEIDON_ARITY_MAX 4$", hdr, re.M)
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for name in NAMES:
        assert name in semantics, name
        assert name in threading, name
    assert "bn254_fr_poseidon_ex_batch and bn254_fr_poseidon_chain_batch serialise on the context" in threading
    assert "BLOCKING copy at the first use of the width" in threading
    own = " ".join(hdr[hdr.index("Wide Poseidon over Fr"):hdr.index("#define BN254_POSEIDON_EX_INPUTS_MAX")].split())
    for word in ("R_F = 8", "56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68", "Grain", str(WC.KNOWN[6]), str(WC.KNOWN[16]), "circomlibjs publishes",
                 "regression anchors and not external vectors", "PoseidonEx(n_inputs, n_outs)", "[init ? init[i] : 0, in[i * n_inputs]", "out[i * n_outs + j]", "`init` may be NULL",
                 "must not overlap", "c = Fr(L)", "max(1, ceil(L / rate))", "an empty record is one block of zeros", "THIS FRAMING IS THIS PROJECT'S OWN DEFINITION",
                 "not an additive sponge", "not a format of any other library", "canonical", "2^22", "no workgroup barrier", "n == 0 and m == 0 return BN254_OK",
                 "BN254_E_BAD_ARG", "above 2^40", "offsets[0] != 0", "Threading", "profiles/r27_poseidon_wide.txt"):
        assert word in own, word
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"fr_poseidon_ex"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)
    src = (ROOT / "bn_amd" / "csrc" / "bn254_poseidon_wide.hip").read_text()
    assert set(re.findall(r'"(fr_\w+)"', src)) == set(SCOPES)


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn fr_poseidon_ex(input: &[Fr], n_inputs: usize, init: Option<&[Fr]>, n_outs: usize) -> Result<Vec<Fr>, GpuError>",
               "pub fn fr_poseidon_chain(input: &[Fr], offsets: &[usize], rate: usize) -> Result<Vec<Fr>, GpuError>"):
        assert fn in txt, fn
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<Fr> fr_poseidon_ex(", "std::vector<Fr> fr_poseidon_chain(", "bn254_fr_poseidon_ex_batch(", "bn254_fr_poseidon_chain_batch("):
        assert s in hpp, s
    for doc in ("README.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        for name in ("bn254_fr_poseidon_ex_batch", "bn254_fr_poseidon_chain_batch", "profiles/r27_poseidon_wide.txt"):
            assert name in text, (doc, name)
        for word in ("additive sponge", "factored partial rounds", "rerouting", "Poseidon2", "multi-GPU"):       # the "not built" list
            assert word in text, (doc, word)
    assert "bn254_poseidon_wide.hip" in [s.name for s in _native.SOURCES]
    assert (ROOT / "bn_amd" / "csrc" / "poseidon_wide_ops.hpp").exists() and (ROOT / "bn_amd" / "csrc" / "poseidon_wide_table.hpp").exists()
    variant = (ROOT / "tools" / "build_variant.sh").read_text()
    assert " bn254_poseidon_wide " in variant and "-DBN254_POSEIDON_WIDE_LANES=" in variant
    assert (ROOT / "profiles" / "r27_poseidon_wide.txt").exists() and (ROOT / "tools" / "time_poseidon_wide.py").exists()


def test_the_older_limits_and_the_generated_constants_stand():
    import subprocess
    from bn_amd import engine, poseidon
    assert poseidon.ARITY_MAX == 4 and engine.POSEIDON_ARITY_MAX == 4 and engine.POSEIDON_EX_INPUTS_MAX == 16
    assert subprocess.run([sys.executable, str(ROOT / "tools" / "gen_poseidon_constants.py"), "--check"]).returncode == 0


@pytest.mark.parametrize("t", [2, 3, 6, 17])
def test_the_table_hook_is_the_python_derivation(lib, t):
    """every element of (C, M) as the kernels read it; tests/test_hostsim_poseidon_wide.py runs the same header at all sixteen widths"""
    import hostsim_poseidon_wide_lib as H
    from bn_amd import poseidon
    n = (8 + poseidon.R_P[t]) * t + t * t
    raw = np.zeros((n + 1, 4), np.uint64)
    raw[n] = 0x5a5a5a5a5a5a5a5a
    assert lib.bn254_fr_poseidon_wide_table(t, raw.ctypes.data) == 0
    assert (raw[n] == 0x5a5a5a5a5a5a5a5a).all()                                                 # nothing behind the table is written
    Cc, M = H.split_table(t, raw[:n])
    pC, pM = poseidon.constants(t)
    assert Cc == list(pC) and M == [list(r) for r in pM]


def test_the_hooks_check_their_bounds(lib):
    buf = np.zeros(8, np.uint32)
    assert [lib.bn254_fr_poseidon_wide_table(t, buf.ctypes.data) for t in (1, 18, -3)] == [BAD_ARG] * 3 and lib.bn254_fr_poseidon_wide_table(2, None) == BAD_ARG
    try:
        assert lib.bn254_fr_poseidon_wide_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_fr_poseidon_wide_set_launch_max(20) == 0
    finally:
        assert lib.bn254_fr_poseidon_wide_set_launch_max(0) == 0
    G, block = lib.bn254_fr_poseidon_wide_lanes(), lib.bn254_fr_poseidon_wide_block()
    assert G in (4, 8, 16) and block % 64 == 0 and 64 % G == 0                                   # a group never straddles a wave
    ops = (ROOT / "bn_amd" / "csrc" / "poseidon_wide_ops.hpp").read_text()
    assert int(re.search(r"^#define BN254_POSEIDON_WIDE_LANES (\d+)$", ops, re.M).group(1)) == G


DUMMY = C.c_void_p(0x100000)       # never dereferenced: every case below is answered before the data is read
FAR = C.c_void_p(0x100000 + (1 << 44))


@pytest.mark.parametrize("case, in_, n_inputs, init, n_outs, out, n", [
    ("no inputs", DUMMY, 0, None, 1, FAR, 4),
    ("seventeen inputs", DUMMY, 17, None, 1, FAR, 4),
    ("negative inputs", DUMMY, -1, None, 1, FAR, 4),
    ("seventeen inputs without work", DUMMY, 17, None, 1, FAR, 0),
    ("no outputs", DUMMY, 3, None, 0, FAR, 4),
    ("more outputs than the state holds", DUMMY, 3, None, 5, FAR, 4),
    ("more outputs than the state holds, without work", DUMMY, 3, None, 5, FAR, 0),
    ("a NULL in", None, 2, None, 1, FAR, 4),
    ("a NULL out", DUMMY, 2, None, 1, None, 4),
    ("n * t > 2^40", DUMMY, 16, None, 1, FAR, (1 << 40) // 17 + 1),
])
def test_ex_argument_errors_answer_without_a_device(lib, case, in_, n_inputs, init, n_outs, out, n):
    assert [lib.bn254_fr_poseidon_ex_batch(None, in_, n_inputs, init, n_outs, out, n), lib.bn254_fr_poseidon_ex_batch_dev(None, in_, n_inputs, init, n_outs, out, n, None)] == [BAD_ARG] * 2, case


def test_ex_overlap_is_an_error_of_the_host_buffer_form(lib):
    base = 0x100000
    inside_in, inside_init = C.c_void_p(base + 32), C.c_void_p(base + 4096 + 96)
    assert lib.bn254_fr_poseidon_ex_batch(None, DUMMY, 2, None, 1, inside_in, 4) == BAD_ARG
    assert lib.bn254_fr_poseidon_ex_batch(None, DUMMY, 2, C.c_void_p(base + 4096), 1, inside_init, 4) == BAD_ARG
    assert lib.bn254_fr_poseidon_ex_batch(None, DUMMY, 2, None, 1, DUMMY, 4) == BAD_ARG


def _off(*v):
    return (C.c_size_t * len(v))(*v)


@pytest.mark.parametrize("case, in_, offsets, m, rate, out", [
    ("rate zero", DUMMY, _off(0, 2), 1, 0, FAR),
    ("rate seventeen", DUMMY, _off(0, 2), 1, 17, FAR),
    ("rate seventeen without work", DUMMY, _off(0), 0, 17, FAR),
    ("NULL offsets", DUMMY, None, 1, 16, FAR),
    ("NULL out", DUMMY, _off(0, 2), 1, 16, None),
    ("NULL in with elements", None, _off(0, 2), 1, 16, FAR),
    ("offsets do not start at 0", DUMMY, _off(1, 2), 1, 16, FAR),
    ("offsets decrease", DUMMY, _off(0, 3, 2), 2, 16, FAR),
    ("more than 2^40 elements", DUMMY, _off(0, (1 << 40) + 1), 1, 16, FAR),
])
def test_chain_argument_errors_answer_without_a_device(lib, case, in_, offsets, m, rate, out):
    assert [lib.bn254_fr_poseidon_chain_batch(None, in_, offsets, m, rate, out), lib.bn254_fr_poseidon_chain_batch_dev(None, in_, offsets, m, rate, out, None)] == [BAD_ARG] * 2, case


def test_chain_overlap_is_an_error_of_the_host_buffer_form(lib):
    assert lib.bn254_fr_poseidon_chain_batch(None, DUMMY, _off(0, 4), 1, 16, C.c_void_p(0x100000 + 96)) == BAD_ARG


def test_no_work_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 8)(*([7] * 8))
    for p in (None, DUMMY):
        for k in (1, 16):
            assert [lib.bn254_fr_poseidon_ex_batch(None, p, k, None, 1, out, 0), lib.bn254_fr_poseidon_ex_batch_dev(None, p, k, p, k + 1, None, 0, None)] == [0, 0]
            assert [lib.bn254_fr_poseidon_chain_batch(None, p, None, 0, k, out), lib.bn254_fr_poseidon_chain_batch_dev(None, p, _off(0), 0, k, None, None)] == [0, 0]
    assert list(out) == [7] * 8


def test_python_surface():
    import bn_amd
    from bn_amd import engine, merkle, poseidon
    assert list(inspect.signature(bn_amd.fr_poseidon_ex_batch).parameters) == ["inputs", "init", "n_outs", "engine"]
    assert list(inspect.signature(bn_amd.fr_poseidon_chain_batch).parameters) == ["records", "rate", "engine"]
    assert inspect.signature(bn_amd.fr_poseidon_ex_batch).parameters["n_outs"].default == 1 and inspect.signature(bn_amd.fr_poseidon_chain_batch).parameters["rate"].default == 16
    E = engine.Engine
    assert list(inspect.signature(E.fr_poseidon_ex_batch).parameters) == ["self", "x", "init", "n_outs"]
    assert list(inspect.signature(E.fr_poseidon_chain_batch).parameters) == ["self", "x", "offsets", "rate"]
    assert list(inspect.signature(E.fr_poseidon_ex_batch_dev).parameters) == ["self", "d_in", "n_inputs", "d_init", "n_outs", "d_out", "n", "stream"]
    assert list(inspect.signature(E.fr_poseidon_chain_batch_dev).parameters) == ["self", "d_in", "offsets", "rate", "d_out", "stream"]
    assert list(inspect.signature(poseidon.hash_ex).parameters) == ["inputs", "init", "n_outs", "engine"]
    assert list(inspect.signature(poseidon.hash_ex_host).parameters) == ["inputs", "init", "n_outs"]
    assert list(inspect.signature(poseidon.hash_chain).parameters) == ["values", "rate", "engine"]
    assert list(inspect.signature(poseidon.hash_chain_host).parameters) == ["values", "rate"]
    assert list(inspect.signature(merkle.Tree.from_records).parameters) == ["rows", "rate", "engine"]
    src = inspect.getsource(merkle.Tree.from_records)
    assert src.count("fr_poseidon_chain_batch(") == 1 and "hash_chain_host" not in src.split('"""')[2]
    for word in ("own", "not an additive sponge"):
        assert word in inspect.getdoc(bn_amd.fr_poseidon_chain_batch), word


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def test_bad_arguments_raise_before_any_device_call_and_name_the_operand():
    import bn_amd
    from bn_amd import poseidon
    one, nd = bn_amd.Fr.one(), NoDevice()
    with pytest.raises(ValueError, match="^inputs holds 17 records per row, n_inputs = 1..16"):
        bn_amd.fr_poseidon_ex_batch([[one] * 17], engine=nd)
    with pytest.raises(ValueError, match="^rows differ in length"):
        bn_amd.fr_poseidon_ex_batch([[one] * 2, [one]], engine=nd)
    with pytest.raises(ValueError, match="^n_outs = 4: 1..3 for 2 inputs per row"):
        bn_amd.fr_poseidon_ex_batch([[one] * 2], n_outs=4, engine=nd)
    with pytest.raises(ValueError, match="^n_outs = 0"):
        bn_amd.fr_poseidon_ex_batch([[one] * 2], n_outs=0, engine=nd)
    with pytest.raises(ValueError, match="^init holds 3 records but x has 2 rows"):
        bn_amd.fr_poseidon_ex_batch([[one] * 2] * 2, init=[one] * 3, engine=nd)
    for rate in (0, 17):
        with pytest.raises(ValueError, match="^rate = %d: 1..16" % rate):
            bn_amd.fr_poseidon_chain_batch([[one]], rate=rate, engine=nd)
    with pytest.raises(ValueError, match="^offsets must start at 0 and never decrease"):
        bn_amd.fr_poseidon_chain_batch(([one] * 3, [0, 2, 1]), engine=nd)
    with pytest.raises(ValueError, match="^x holds 3 records but offsets\\[m\\] = 2"):
        bn_amd.fr_poseidon_chain_batch(([one] * 3, [0, 2]), engine=nd)
    with pytest.raises(ValueError, match="1 .. 16 inputs, not 17"):
        poseidon.hash_ex([one] * 17, engine=nd)
    with pytest.raises(ValueError, match="n_outs = 3: 1 .. 2 for 1 inputs"):
        poseidon.hash_ex([one], n_outs=3, engine=nd)
    with pytest.raises(ValueError, match="rate = 17"):
        poseidon.hash_chain([one], rate=17, engine=nd)
    assert bn_amd.fr_poseidon_chain_batch([], engine=nd) == []


class Model:
    """a stand-in engine that answers from the integer model and records what was asked"""
    def __init__(self): self.calls = []

    @staticmethod
    def _ints(a):
        from bn_amd import Fr
        return [Fr.from_limbs(r).v for r in np.asarray(a, np.uint64).reshape(-1, 4)]

    def fr_poseidon_chain_batch(self, x, offsets, rate=16):
        flat, o = self._ints(x), [int(v) for v in offsets]
        self.calls.append(("fr_poseidon_chain_batch", len(o) - 1, rate))
        return FC.rows([WC.hash_chain(flat[a:b], rate) for a, b in zip(o, o[1:])])

    def fr_poseidon_ex_batch(self, x, init=None, n_outs=1):
        x = np.asarray(x, np.uint64)
        self.calls.append(("fr_poseidon_ex_batch", x.shape[0], n_outs))
        flat, k = self._ints(x), x.shape[1]
        inits = self._ints(init) if init is not None else [0] * x.shape[0]
        return FC.rows([v for i in range(x.shape[0]) for v in WC.hash_ex(flat[i * k:(i + 1) * k], inits[i], n_outs)]).reshape(x.shape[0], n_outs, 4)

    def fr_merkle_tree(self, leaves):
        self.calls.append("fr_merkle_tree")
        return FC.rows(PC.tree(self._ints(leaves))).reshape(-1, 4)


def test_the_python_layers_over_a_stand_in_engine_that_answers_from_the_model():
    import bn_amd
    from bn_amd import Fr, merkle, poseidon
    m = Model()
    lengths = [0, 1, 3, 4, 5, 14, 2, 7]
    recs, flat, off = WC.records(lengths, 5)
    want = [WC.hash_chain(r, 4) for r in recs]
    rows = [[Fr(v) for v in r] for r in recs]
    assert [x.v for x in bn_amd.fr_poseidon_chain_batch(rows, rate=4, engine=m)] == want
    assert [x.v for x in bn_amd.fr_poseidon_chain_batch(([Fr(v) for v in flat], off), rate=4, engine=m)] == want
    assert m.calls == [("fr_poseidon_chain_batch", 8, 4)] * 2
    m.calls.clear()
    tree = merkle.Tree.from_records(rows, rate=4, engine=m)
    assert m.calls == [("fr_poseidon_chain_batch", 8, 4), "fr_merkle_tree"]                      # the leaves are ONE call, the tree the existing one
    assert [x.v for x in tree.leaves] == want and tree.root.v == PC.tree(want)[-1] and tree.depth == 3
    assert merkle.verify(tree.root, tree.leaves[5], 5, tree.open(5))
    assert poseidon.hash_chain(rows[5], rate=4, engine=m).v == want[5] == poseidon.hash_chain_host(recs[5], 4)
    assert poseidon.hash_chain([], rate=4, engine=m).v == want[0]
    x = WC.values(6, 9)
    got = bn_amd.fr_poseidon_ex_batch([[Fr(v) for v in x]] * 2, init=[Fr(3), Fr(4)], n_outs=2, engine=m)
    assert [[y.v for y in row] for row in got] == [WC.hash_ex(x, 3, 2), WC.hash_ex(x, 4, 2)]
    got = bn_amd.fr_poseidon_ex_batch([[Fr(v) for v in x]] * 2, init=Fr(3), engine=m)          # one initial state for every row
    assert [[y.v for y in row] for row in got] == [WC.hash_ex(x, 3, 1)] * 2
    assert [y.v for y in poseidon.hash_ex([Fr(v) for v in x], init=5, n_outs=7, engine=m)] == WC.permute([5] + x) == poseidon.hash_ex_host(x, 5, 7)


def test_the_kernels_are_instances_of_fr_decode_k_and_spill_nothing():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    import lane_shell
    src = lane_shell.unit_source("bn254_poseidon_wide.hip")  # the unit adds no kernel under any other name: the shell is lane_launch.hpp's
    assert "__syncthreads" not in src and "s_barrier" not in src                                  # wave-scope ordering only
    ops = (ROOT / "bn_amd" / "csrc" / "poseidon_wide_ops.hpp").read_text()
    assert "__syncthreads" not in ops and "#pragma unroll 1" in ops                              # rounds, elements and chunks stay loops
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    meta = kernel_meta.instances(so)
    mine = [n for n in meta if kernel_meta.short_name(n) == "bn254_fr_decode_k" and re.search(r"\d+FrPoseidonWide(Ex|Chain)OpI", n)]
    assert len(mine) == 2, mine                                                                 # one instance per call kind: the width is a run-time argument
    for n in mine:
        assert meta[n]["spill"] == 0 and meta[n]["private"] == 0 and 0 < meta[n]["lds"] <= 2 * 17 * 32 * 32, (n, meta[n])
