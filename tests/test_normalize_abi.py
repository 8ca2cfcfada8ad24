"""Batched normalize and projective equality (bn254_g{1,2}_normalize_batch*, bn254_g{1,2}_eq_batch*) without a GPU: the eight declarations
in every layer that mirrors the C header, the Python surface, the argument checks that answer before any device is touched, the new
profiling scopes, and the register budget of the device code - the kernels are template instances of existing kernel names
(bn254_g{1,2}_add_M<NormalizeArgs> and bn254_g{1,2}_add_M<EqArgs>)."""
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


def _norm(g):
    return [("void", MUT), (g, CONST), (g, MUT), ("usize", ())]


def _eq(g):
    return [("void", MUT), (g, CONST), (g, CONST), ("i32", MUT), ("usize", ())]


NORM_DEV = [("void", MUT), ("void", CONST), ("void", MUT), ("usize", ()), ("void", MUT)]
EQ_DEV = [("void", MUT), ("void", CONST), ("void", CONST), ("void", MUT), ("usize", ()), ("void", MUT)]
EXPECTED = {
    "bn254_g1_normalize_batch": _norm("g1"), "bn254_g2_normalize_batch": _norm("g2"),
    "bn254_g1_eq_batch": _eq("g1"), "bn254_g2_eq_batch": _eq("g2"),
    "bn254_g1_normalize_batch_dev": NORM_DEV, "bn254_g2_normalize_batch_dev": NORM_DEV,
    "bn254_g1_eq_batch_dev": EQ_DEV, "bn254_g2_eq_batch_dev": EQ_DEV,
}
NAMES = tuple(EXPECTED)
SCOPES = ("g1_normalize", "g2_normalize", "g1_eq", "g2_eq")
BAD_ARG = -2


def test_header_declares_the_eight_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]                 # the "Semantics replaced" list
    assert "bn254_g1_normalize_batch / bn254_g2_normalize_batch" in semantics and "bn254_g1_eq_batch / bn254_g2_eq_batch" in semantics
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_g{1,2}_normalize_batch and bn254_g{1,2}_eq_batch serialise" in threading
    assert "bn254_g{1,2}_normalize_batch_dev" in threading and "bn254_g{1,2}_eq_batch_dev" in threading
    own = " ".join(hdr[hdr.index("Batched normalisation and projective equality"):hdr.index("int bn254_g1_normalize_batch(")].split())
    for word in ("(0, 1, 0)", "Fr::one()", "parity definition", "exactly `p`", "Montgomery's trick", "no inversion", "profiles/r12_normalize.txt",
                 "BN254_E_BAD_ARG", "Threading"):
        assert word in own, word


def test_no_new_type_and_no_new_option():
    hdr = B.HEADER.read_text()
    types = "".join(re.findall(r"typedef[^;]*;", hdr))
    assert "normalize" not in types and "_eq" not in types
    added = [l for l in hdr.splitlines() if "normalize_batch" in l or "eq_batch" in l]
    assert added and not any("typedef" in l or "struct" in l for l in added)
    assert B.c_enum("BN254_OPT_")["COUNT_"] == 16


def test_the_scope_names_are_appended_to_the_stats_line():
    stats = re.search(r"/\* kernel: (.*?)\n", B.HEADER.read_text()).group(1)
    names = re.findall(r'"(\w+)"', stats)
    at = names.index("g2_base_table")
    assert tuple(names[at + 1:at + 5]) == SCOPES, names[at:]
    assert names[-4:] == list(SCOPES)                                                            # the older names keep their order, in front


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
    for g in ("G1", "G2"):
        assert re.search(r"pub fn %s_normalize\(p: &\[%s\]\) -> Result<Vec<%s>, GpuError>" % (g.lower(), g, g), txt)
        assert re.search(r"pub fn %s_eq\(a: &\[%s\], b: &\[%s\]\) -> Result<Vec<bool>, GpuError>" % (g.lower(), g, g), txt)
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<G1> g1_normalize(const std::vector<G1> &p)", "std::vector<G2> g2_normalize(const std::vector<G2> &p)",
              "std::vector<bool> g1_eq(const std::vector<G1> &a, const std::vector<G1> &b)", "std::vector<bool> g2_eq(const std::vector<G2> &a, const std::vector<G2> &b)",
              "bool operator==(const G1 &o) const", "bool operator==(const G2 &o) const",
              "void normalize() { check(bn254_g1_normalize_batch(", "void normalize() { check(bn254_g2_normalize_batch(",
              "bn254_g1_eq_batch(", "bn254_g2_eq_batch("):
        assert s in hpp, s
    assert "Fr::one(); }" not in hpp                                                             # normalize() is no longer a multiplication by one


def test_python_surface():
    import bn_amd
    from bn_amd import api, engine
    for g in ("g1", "g2"):
        assert list(inspect.signature(getattr(bn_amd, g + "_normalize_batch")).parameters) == ["points", "engine"]
        assert list(inspect.signature(getattr(bn_amd, g + "_eq_batch")).parameters) == ["a", "b", "engine"]
        assert list(inspect.signature(getattr(engine.Engine, g + "_normalize")).parameters) == ["self", "p"]
        assert list(inspect.signature(getattr(engine.Engine, g + "_eq")).parameters) == ["self", "a", "b"]
        assert list(inspect.signature(getattr(engine.Engine, g + "_normalize_dev")).parameters) == ["self", "d_p", "d_out", "n", "stream"]
        assert list(inspect.signature(getattr(engine.Engine, g + "_eq_dev")).parameters) == ["self", "d_a", "d_b", "d_out", "n", "stream"]
    for cls in (bn_amd.G1, bn_amd.G2):
        assert callable(cls.normalize) and callable(cls.__eq__)
        for fn in (cls.normalize, cls.__eq__):
            src = inspect.getsource(fn)
            assert "Fr.one()" not in src and "__mul__" not in src and "self *" not in src, src
        assert ".normalize(" not in inspect.getsource(cls.__eq__)                                 # one comparison, nothing normalized
    assert "_eq(" in inspect.getsource(api._Point.__eq__) and "_normalize(" in inspect.getsource(api._Point.normalize)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


def _normalize_all(lib, p, out, n):
    return [lib.bn254_g1_normalize_batch(None, p, out, n), lib.bn254_g2_normalize_batch(None, p, out, n),
            lib.bn254_g1_normalize_batch_dev(None, p, out, n, None), lib.bn254_g2_normalize_batch_dev(None, p, out, n, None)]


def _eq_all(lib, a, b, out, n):
    return [lib.bn254_g1_eq_batch(None, a, b, out, n), lib.bn254_g2_eq_batch(None, a, b, out, n),
            lib.bn254_g1_eq_batch_dev(None, a, b, out, n, None), lib.bn254_g2_eq_batch_dev(None, a, b, out, n, None)]


@pytest.mark.parametrize("case, p, out, n", [
    ("NULL p", None, DUMMY, 2),
    ("NULL out", DUMMY, None, 2),
    ("n > 2^40", DUMMY, DUMMY, (1 << 40) + 1),
])
def test_normalize_argument_errors_answer_without_a_device(lib, case, p, out, n):
    assert _normalize_all(lib, p, out, n) == [BAD_ARG] * 4, case


@pytest.mark.parametrize("case, a, b, out, n", [
    ("NULL a", None, DUMMY, DUMMY, 2),
    ("NULL b", DUMMY, None, DUMMY, 2),
    ("NULL out", DUMMY, DUMMY, None, 2),
    ("n > 2^40", DUMMY, DUMMY, DUMMY, (1 << 40) + 1),
])
def test_eq_argument_errors_answer_without_a_device(lib, case, a, b, out, n):
    assert _eq_all(lib, a, b, out, n) == [BAD_ARG] * 4, case


def test_an_empty_batch_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 24)(*([7] * 24))
    for p in (None, DUMMY):                                                                   # n == 0 is answered before the arguments
        assert _normalize_all(lib, p, out, 0) == [0] * 4
        assert _normalize_all(lib, p, None, 0) == [0] * 4
        assert _eq_all(lib, p, p, out, 0) == [0] * 4
        assert _eq_all(lib, p, p, None, 0) == [0] * 4
    assert list(out) == [7] * 24


def test_the_run_length_is_one_of_the_measured_ones(lib):
    lib.bn254_normalize_run.argtypes = []; lib.bn254_normalize_run.restype = C.c_uint
    assert lib.bn254_normalize_run() in (1, 4, 8, 16)
    lib.bn254_normalize_set_launch_max.argtypes = [C.c_size_t]
    assert lib.bn254_normalize_set_launch_max((1 << 22) + 1) == BAD_ARG
    assert lib.bn254_normalize_set_launch_max(0) == 0


def test_every_kernel_is_a_known_name_under_its_spill_ceiling():
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
    for short in ("bn254_g1_add_M", "bn254_g2_add_M"):
        assert SPILL_CEILING[short] == 0
        for args in ("NormalizeArgs", "EqArgs"):
            mine = [n for n in inst if kernel_meta.short_name(n) == short and args in n]
            assert len(mine) == 1, (short, args, mine)
            assert inst[mine[0]] == 0, mine
    # the instance counts other tests pin stay as they were
    assert sum(kernel_meta.short_name(n) in ("bn254_g1_mul_M", "bn254_g2_mul_M") for n in inst) == 4
