"""Fixed-base scalar multiplication (bn254_g{1,2}_mul_base_batch*) without a GPU: the four declarations in every layer that mirrors the C
header, the Python surface, the argument checks that answer before any device is touched, the scalars a table is built with, the new
profiling scopes, and the register budget of the device code - every kernel added is a template instance of an existing kernel name
(bn254_g{1,2}_add_M<BaseMulArgs> are the chains, bn254_fr_decode_k<BaseTileOp|BaseRepackOp> the two ends of a table build)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import pytest

import bn_model as M
import test_binding_signatures as B
from test_product_batch_abi import _instances

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST = ("const",)
MUT = ("mut",)
R = M.R_ORD


def _host(g):
    return [("void", MUT), (g, CONST), ("fr", CONST), (g, MUT), ("usize", ())]


def _dev(g):
    return [("void", MUT), (g, CONST), ("void", CONST), ("void", MUT), ("usize", ()), ("void", MUT)]


EXPECTED = {
    "bn254_g1_mul_base_batch": _host("g1"), "bn254_g2_mul_base_batch": _host("g2"),
    "bn254_g1_mul_base_batch_dev": _dev("g1"), "bn254_g2_mul_base_batch_dev": _dev("g2"),
}
NAMES = tuple(EXPECTED)
SCOPES = ("g1_mul_base", "g2_mul_base", "g1_base_table", "g2_base_table")
BAD_ARG = -2


def test_header_declares_the_four_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    semantics = hdr[:hdr.index("Error behaviour")]
    assert "bn254_g1_mul_base_batch / bn254_g2_mul_base_batch" in semantics                     # the "Semantics replaced" list
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_g{1,2}_mul_base_batch serialise" in threading and "bn254_g{1,2}_mul_base_batch_dev" in threading
    own = hdr[hdr.index("Fixed-base scalar multiplication"):hdr.index("int bn254_g1_mul_base_batch(")]
    for word in ("FOUR", "3 604 480", "7 208 960", "miss", "BN254_E_BAD_ARG", "Threading"):       # table size, slots, cost of a miss, threading
        assert word in own, word


def test_no_new_type_and_no_new_option():
    hdr = B.HEADER.read_text()
    assert "mul_base" not in "".join(re.findall(r"typedef struct[^;]*;", hdr))
    assert B.c_enum("BN254_OPT_")["COUNT_"] == 16


def test_the_scope_names_are_on_the_stats_line():
    stats = re.search(r"/\* kernel: (.*?)\n", B.HEADER.read_text()).group(1)
    for s in SCOPES:
        assert f'"{s}"' in stats, s
        assert stats.index('"g2_msm_reduce"') < stats.index(f'"{s}"')                           # appended: the older names keep their order


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
    assert re.search(r"pub fn g1_mul_base\(base: &G1, k: &\[Fr\]\) -> Result<Vec<G1>, GpuError>", txt)
    assert re.search(r"pub fn g2_mul_base\(base: &G2, k: &\[Fr\]\) -> Result<Vec<G2>, GpuError>", txt)
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<G1> g1_mul_base(const G1 &base, const std::vector<Fr> &k)", "std::vector<G2> g2_mul_base(const G2 &base, const std::vector<Fr> &k)",
              "bn254_g1_mul_base_batch(", "bn254_g2_mul_base_batch("):
        assert s in hpp, s


def test_python_surface():
    import bn_amd
    from bn_amd import distributed, engine
    for g in ("g1", "g2"):
        assert list(inspect.signature(getattr(bn_amd, g + "_mul_base")).parameters) == ["base", "scalars", "engine"]
        assert list(inspect.signature(getattr(engine.Engine, g + "_mul_base_batch")).parameters) == ["self", "base", "k"]
        assert list(inspect.signature(getattr(engine.Engine, g + "_mul_base_batch_dev")).parameters) == ["self", "base", "d_k", "d_out", "n", "stream"]
        assert list(inspect.signature(getattr(distributed.TorchEngine, g + "_mul_base")).parameters) == ["self", "base", "k"]
    assert list(inspect.signature(bn_amd.G1.mul_base).parameters) == ["self", "scalars"]
    assert list(inspect.signature(bn_amd.G2.mul_base).parameters) == ["self", "scalars"]


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


def _call_all(lib, base, k, out, n):
    return [lib.bn254_g1_mul_base_batch(None, base, k, out, n), lib.bn254_g2_mul_base_batch(None, base, k, out, n),
            lib.bn254_g1_mul_base_batch_dev(None, base, k, out, n, None), lib.bn254_g2_mul_base_batch_dev(None, base, k, out, n, None)]


@pytest.mark.parametrize("case, base, k, out, n", [
    ("NULL base", None, DUMMY, DUMMY, 2),
    ("NULL k", DUMMY, None, DUMMY, 2),
    ("NULL out", DUMMY, DUMMY, None, 2),
    ("n > 2^40", DUMMY, DUMMY, DUMMY, (1 << 40) + 1),
])
def test_argument_errors_answer_without_a_device(lib, case, base, k, out, n):
    assert _call_all(lib, base, k, out, n) == [BAD_ARG] * 4, case


def test_an_empty_batch_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 24)(*([7] * 24))
    for base, k in ((None, None), (DUMMY, DUMMY)):                                            # n == 0 is answered before the arguments
        assert _call_all(lib, base, k, out, 0) == [0] * 4
        assert _call_all(lib, base, k, None, 0) == [0] * 4
    assert list(out) == [7] * 24


def _getters(lib):
    lib.bn254_mul_base_window.argtypes = [C.c_int]; lib.bn254_mul_base_window.restype = C.c_uint
    lib.bn254_mul_base_table_bytes.argtypes = [C.c_int]; lib.bn254_mul_base_table_bytes.restype = C.c_size_t
    lib.bn254_mul_base_slots.argtypes = []; lib.bn254_mul_base_slots.restype = C.c_uint
    lib.bn254_mul_base_table_scalars.argtypes = [C.c_uint, C.c_void_p, C.c_size_t]; lib.bn254_mul_base_table_scalars.restype = C.c_size_t
    return lib


@pytest.mark.parametrize("g", [1, 2])
def test_table_scalars_are_d_times_two_to_the_c_w(lib, g):
    """the exported host helper against Python integers, for the shipped width of the group (and the two other widths of the sweep)"""
    import numpy as np
    _getters(lib)
    shipped = lib.bn254_mul_base_window(g)
    assert lib.bn254_mul_base_slots() == 4
    for c in sorted({shipped, 8, 10, 12}):
        W = (254 + c - 1) // c
        half = 1 << (c - 1)
        assert W * c >= 254
        assert W * c > 254, "the top window of a scalar below r must not carry"
        count = lib.bn254_mul_base_table_scalars(c, None, 0)
        assert count == W * half
        buf = np.zeros((count, 4), np.uint64)
        assert lib.bn254_mul_base_table_scalars(c, buf.ctypes.data_as(C.c_void_p), buf.size) == count
        for w in range(W):
            for d in sorted({1, 2, 3, half - 1, half} | {(7 * w + 5) % half + 1}):
                want = d * (1 << (c * w)) % R * (1 << 256) % R
                got = sum(int(x) << (64 * i) for i, x in enumerate(buf[w * half + d - 1]))
                assert got == want, (c, w, d)
        # every entry, as one sum per window: sum_d d * 2^(c w) = 2^(c w) * half (half + 1) / 2
        for w in range(W):
            tot = sum(sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in buf[w * half:(w + 1) * half]) % R
            assert tot == (half * (half + 1) // 2) * (1 << (c * w)) % R * (1 << 256) % R, (c, w)
    assert lib.bn254_mul_base_table_bytes(g) == ((254 + shipped - 1) // shipped) * (1 << (shipped - 1)) * 80 * g


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
    for short, args in (("bn254_g1_add_M", "BaseMulArgs"), ("bn254_g2_add_M", "BaseMulArgs"), ("bn254_fr_decode_k", "BaseTileOp"), ("bn254_fr_decode_k", "BaseRepackOp")):
        assert any(kernel_meta.short_name(n) == short and args in n for n in inst), (short, args)
        assert SPILL_CEILING[short] == 0
    # the instance counts other tests pin stay as they were
    assert sum(kernel_meta.short_name(n) in ("bn254_g1_mul_M", "bn254_g2_mul_M") for n in inst) == 4
