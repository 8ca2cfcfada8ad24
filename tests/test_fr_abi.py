"""Batched Fr arithmetic (bn254_fr_{add,mul,inverse,pow,interpret}_batch and their _dev twins) without a GPU: the ten declarations in every
layer that mirrors the C header, the Python surface, the argument checks that answer before any device is touched, the new profiling scopes,
and the register budget of the device code - the kernels are template instances of an existing kernel name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import pytest

import test_binding_signatures as B
from test_product_batch_abi import _instances

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST = ("const",)
MUT = ("mut",)
CTX, FR_IN, FR_OUT, N, INT = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ()), ("int", ())
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_fr_add_batch": [CTX, FR_IN, FR_IN, FR_OUT, N, INT],
    "bn254_fr_mul_batch": [CTX, FR_IN, FR_IN, FR_OUT, N],
    "bn254_fr_inverse_batch": [CTX, FR_IN, FR_OUT, ("i32", MUT), N],
    "bn254_fr_pow_batch": [CTX, FR_IN, FR_IN, FR_OUT, N],
    "bn254_fr_interpret_batch": [CTX, ("u8", CONST), FR_OUT, N],
    "bn254_fr_add_batch_dev": [CTX, D_IN, D_IN, D_OUT, N, INT, D_OUT],
    "bn254_fr_mul_batch_dev": [CTX, D_IN, D_IN, D_OUT, N, D_OUT],
    "bn254_fr_inverse_batch_dev": [CTX, D_IN, D_OUT, D_OUT, N, D_OUT],
    "bn254_fr_pow_batch_dev": [CTX, D_IN, D_IN, D_OUT, N, D_OUT],
    "bn254_fr_interpret_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("fr_add", "fr_mul", "fr_inverse", "fr_pow", "fr_interpret")
OPS = ("FrAddOp", "FrMulOp", "FrInverseOp", "FrPowOp", "FrInterpretOp")
BAD_ARG = -2


def test_header_declares_the_ten_entry_points():
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
    assert "bn254_fr_{add,mul,inverse,pow,interpret}_batch serialise on the context" in threading
    assert "bn254_fr_inverse_batch_dev" in threading and "bn254_fr_{add,mul,pow,interpret}_batch_dev" in threading
    own = " ".join(hdr[hdr.index("Batched scalar-field arithmetic"):hdr.index("int bn254_fr_add_batch(")].split())
    for word in ("canonical", "0^0 = 1", "0^e = 0", "ok may be NULL", "Montgomery's trick", "R^2", "R^3", "exactly `a` or exactly `b`", "BN254_E_BAD_ARG", "Threading",
                 "memory safe"):
        assert word in own, word


def test_no_new_type_and_no_new_option():
    hdr = B.HEADER.read_text()
    types = "".join(re.findall(r"typedef[^;]*;", hdr))
    assert "fr_add" not in types and "fr_inverse" not in types
    assert B.c_enum("BN254_OPT_")["COUNT_"] == 16
    assert "bn254_fr_set_launch_max" not in hdr and "bn254_fr_inverse_run" not in hdr            # the test hooks are internal


def test_the_scope_names_follow_wire_decode():
    stats = re.search(r"/\* kernel: (.*?)\n", B.HEADER.read_text()).group(1)
    names = re.findall(r'"(\w+)"', stats)
    at = names.index("wire_decode")
    assert tuple(names[at + 1:at + 6]) == SCOPES, names[at:]
    assert names[at + 6] == "gt_inverse"                                                          # the older names keep their order
    assert names[-4:] == ["g1_normalize", "g2_normalize", "g1_eq", "g2_eq"]
    assert len(names) == len(set(names))
    src = (ROOT / "bn_amd" / "csrc" / "bn254_fr.hip").read_text()
    assert set(re.findall(r'"(fr_\w+)"', src)) == set(SCOPES)


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
    for fn in ("fr_add", "fr_sub", "fr_mul", "fr_pow"):
        assert re.search(r"pub fn %s\(a: &\[Fr\], \w: &\[Fr\]\) -> Result<Vec<Fr>, GpuError>" % fn, txt), fn
    assert "pub fn fr_inverse(a: &[Fr]) -> Result<Vec<Option<Fr>>, GpuError>" in txt
    assert "pub fn fr_interpret(bufs: &[[u8; 64]]) -> Result<Vec<Fr>, GpuError>" in txt
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<Fr> fr_add(const std::vector<Fr> &a, const std::vector<Fr> &b)", "std::vector<Fr> fr_sub(", "std::vector<Fr> fr_mul(", "std::vector<Fr> fr_pow(",
              "fr_inverse(const std::vector<Fr> &a)", "fr_interpret(", "bn254_fr_add_batch(", "bn254_fr_mul_batch", "bn254_fr_pow_batch", "bn254_fr_inverse_batch(",
              "bn254_fr_interpret_batch("):
        assert s in hpp, s
    for doc in ("README.md", "DESIGN.md"):
        assert "bn254_fr_" in (ROOT / doc).read_text() and "verify_aggregate" in (ROOT / doc).read_text(), doc
    assert "bn254_fr.hip" in [s.name for s in _native.SOURCES]


def test_python_surface():
    import bn_amd
    from bn_amd import engine, groth16
    for name, params in (("fr_add_batch", ["a", "b", "engine"]), ("fr_sub_batch", ["a", "b", "engine"]), ("fr_neg_batch", ["a", "engine"]),
                         ("fr_mul_batch", ["a", "b", "engine"]), ("fr_pow_batch", ["a", "e", "engine"]), ("fr_inverse_batch", ["a", "engine"]),
                         ("fr_interpret_batch", ["bufs", "engine"])):
        assert list(inspect.signature(getattr(bn_amd, name)).parameters) == params, name
    E = engine.Engine
    assert list(inspect.signature(E.fr_add_batch).parameters) == ["self", "a", "b", "negate_b"]
    assert inspect.signature(E.fr_add_batch).parameters["negate_b"].default is False
    assert list(inspect.signature(E.fr_mul_batch).parameters) == ["self", "a", "b"]
    assert list(inspect.signature(E.fr_pow_batch).parameters) == ["self", "a", "e"]
    assert list(inspect.signature(E.fr_inverse_batch).parameters) == ["self", "a"]
    assert list(inspect.signature(E.fr_interpret_batch).parameters) == ["self", "buf"]
    for name in ("fr_add_batch_dev", "fr_mul_batch_dev", "fr_pow_batch_dev", "fr_inverse_batch_dev", "fr_interpret_batch_dev"):
        assert list(inspect.signature(getattr(E, name)).parameters)[-1] == "stream", name
    assert list(inspect.signature(groth16.verify_aggregate).parameters) == ["vk", "proofs", "public_inputs", "engine", "rng"]
    doc = " ".join(groth16.verify_aggregate.__doc__.split())
    assert "2^-128" in doc and "verify_batch" in doc
    src = inspect.getsource(groth16.verify_aggregate)
    for call in ("g1_mul_batch(", "fr_mul_batch(", "g1_msm_batch(", "g1_add_batch(", "pairing_product(", "secrets.randbits(128)"):
        assert src.count(call) == 1, call
    # Fr.interpret on the host, and the scalar operators stay Python integers
    Fr = bn_amd.Fr
    r = bn_amd.api.R_MOD
    assert Fr.interpret(bytes(64)) == Fr.zero() and Fr.interpret(b"\xff" * 64) == Fr(((1 << 512) - 1) % r)
    assert Fr.interpret((r + 5).to_bytes(64, "big")) == Fr(5) and Fr.interpret(bytes(31) + b"\x01" + bytes(32)) == Fr((1 << 256) % r)
    with pytest.raises(ValueError):
        Fr.interpret(bytes(63))
    for op in (Fr.__add__, Fr.__mul__, Fr.inverse, Fr.pow):
        assert "engine" not in inspect.getsource(op)


def test_verify_aggregate_rejects_bad_arguments_and_answers_an_empty_block_without_a_device():
    from bn_amd import groth16

    class NoDevice:
        def __getattr__(self, name): raise AssertionError("a device call was made: " + name)
    vk = groth16.VerifyingKey(None, None, None, None, [None, None, None])                         # l = 2
    assert groth16.verify_aggregate(vk, [], [], engine=NoDevice()) is True
    with pytest.raises(ValueError, match="2 proofs but 1 sets"):
        groth16.verify_aggregate(vk, [None, None], [[1, 2]], engine=NoDevice())
    with pytest.raises(ValueError, match="every proof takes 2 public inputs"):
        groth16.verify_aggregate(vk, [None], [[1]], engine=NoDevice())


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


def _binary_all(lib, a, b, out, n):
    return [lib.bn254_fr_add_batch(None, a, b, out, n, 0), lib.bn254_fr_add_batch(None, a, b, out, n, 1), lib.bn254_fr_mul_batch(None, a, b, out, n),
            lib.bn254_fr_pow_batch(None, a, b, out, n), lib.bn254_fr_add_batch_dev(None, a, b, out, n, 0, None), lib.bn254_fr_mul_batch_dev(None, a, b, out, n, None),
            lib.bn254_fr_pow_batch_dev(None, a, b, out, n, None)]


def _unary_all(lib, a, out, ok, n):
    return [lib.bn254_fr_inverse_batch(None, a, out, ok, n), lib.bn254_fr_inverse_batch_dev(None, a, out, ok, n, None),
            lib.bn254_fr_interpret_batch(None, a, out, n), lib.bn254_fr_interpret_batch_dev(None, a, out, n, None)]


@pytest.mark.parametrize("case, a, b, out, n", [
    ("NULL a", None, DUMMY, DUMMY, 2),
    ("NULL b", DUMMY, None, DUMMY, 2),
    ("NULL out", DUMMY, DUMMY, None, 2),
    ("n > 2^40", DUMMY, DUMMY, DUMMY, (1 << 40) + 1),
])
def test_binary_argument_errors_answer_without_a_device(lib, case, a, b, out, n):
    assert _binary_all(lib, a, b, out, n) == [BAD_ARG] * 7, case


@pytest.mark.parametrize("case, a, out, n", [
    ("NULL input", None, DUMMY, 2),
    ("NULL out", DUMMY, None, 2),
    ("n > 2^40", DUMMY, DUMMY, (1 << 40) + 1),
])
def test_unary_argument_errors_answer_without_a_device(lib, case, a, out, n):
    assert _unary_all(lib, a, out, DUMMY, n) == [BAD_ARG] * 4, case
    assert _unary_all(lib, a, out, None, n) == [BAD_ARG] * 4, case


def test_an_empty_batch_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 8)(*([7] * 8))
    for p in (None, DUMMY):                                                                   # n == 0 is answered before the arguments
        assert _binary_all(lib, p, p, out, 0) == [0] * 7 and _binary_all(lib, p, p, None, 0) == [0] * 7
        assert _unary_all(lib, p, out, out, 0) == [0] * 4 and _unary_all(lib, p, None, None, 0) == [0] * 4
    assert list(out) == [7] * 8


def test_the_shipped_choices_are_measured_ones(lib):
    lib.bn254_fr_inverse_run.argtypes = []; lib.bn254_fr_inverse_run.restype = C.c_uint
    lib.bn254_fr_pow_window.argtypes = []; lib.bn254_fr_pow_window.restype = C.c_uint
    assert lib.bn254_fr_inverse_run() in (1, 4, 8, 16) and lib.bn254_fr_pow_window() in (1, 2, 4)
    lib.bn254_fr_set_launch_max.argtypes = [C.c_size_t]
    assert lib.bn254_fr_set_launch_max((1 << 22) + 1) == BAD_ARG
    assert lib.bn254_fr_set_launch_max(0) == 0


def test_every_kernel_is_an_instance_of_fr_decode_k_and_spills_nothing():
    """what tests/test_build_quality.py::test_spill_ceilings_of_every_kernel checks per short name, here for EVERY instance, and the new
    instances are really in the library"""
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    inst = _instances(so)
    for name, s in inst.items():
        short = kernel_meta.short_name(name)
        assert short in SPILL_CEILING, name
        assert s <= SPILL_CEILING[short], f"{name}: {s} spilled VGPRs, ceiling {SPILL_CEILING[short]}"
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    for op in OPS:
        mine = [n for n in inst if kernel_meta.short_name(n) == "bn254_fr_decode_k" and op in n]
        assert len(mine) >= 1, op
        assert all(inst[n] == 0 for n in mine), mine
    # the unit adds no kernel under any other name
    import lane_shell
    lane_shell.unit_source("bn254_fr.hip")      # the unit adds no kernel of its own: the shell is lane_launch.hpp's
