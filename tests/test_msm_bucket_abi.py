"""One large multi-scalar multiplication (bn254_g{1,2}_msm*) without a GPU: the six declarations in every layer that mirrors the C header,
the three options, the argument checks that answer before any device is touched, the new profiling scopes, and the register budget of the
device code - every kernel it added is a template instance of an existing kernel name (bn254_g{1,2}_add_M<MsmAccArgs|MsmReduceArgs> sum and
reduce the buckets, bn254_fr_decode_k<MsmDigitsOp|MsmScanOp> are the counting sort)."""
import ctypes as C
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


def _host(g):
    return [("void", MUT), (g, CONST), ("fr", CONST), ("usize", ()), (g, MUT)]


DEV = [("void", MUT), ("void", CONST), ("void", CONST), ("usize", ()), ("void", MUT), ("void", MUT)]
EXPECTED = {
    "bn254_g1_msm": _host("g1"), "bn254_g2_msm": _host("g2"),
    "bn254_g1_msm_dev": DEV, "bn254_g2_msm_dev": DEV,
    "bn254_g1_msm_multi": _host("g1"), "bn254_g2_msm_multi": _host("g2"),
}
NAMES = tuple(EXPECTED)
SCOPES = tuple(f"g{g}_msm_{s}" for g in (1, 2) for s in ("digits", "bucket", "reduce"))
OPTIONS = {"msm_bucket_min": ("BN254_OPT_MSM_BUCKET_MIN", "MsmBucketMin", 13), "msm_window_bits": ("BN254_OPT_MSM_WINDOW_BITS", "MsmWindowBits", 14),
           "msm_chunk": ("BN254_OPT_MSM_CHUNK", "MsmChunk", 15)}
BAD_ARG = -2


def test_header_declares_the_six_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    semantics = hdr[:hdr.index("Error behaviour")]
    assert "bn254_g1_msm / bn254_g2_msm" in semantics                                            # the "Semantics replaced" list
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_g{1,2}_msm_dev" in threading and "bn254_g{1,2}_msm serialise" in threading
    stats = re.search(r"/\* kernel: (.*?)\n", hdr).group(1)
    for s in SCOPES + ("g1_msm_mul", "g2_msm_fold", "g1_mul", "gt_segment"):                     # appended: the old names stay on the line
        assert f'"{s}"' in stats, s
    assert stats.index('"g2_msm_fold"') < stats.index('"g1_msm_digits"')
    note = hdr[hdr.index("Segmented multi-scalar multiplication"):hdr.index("int bn254_g1_msm_batch(")]
    assert "Pippenger" in note and "bn254_g{1,2}_msm below" in note                              # the old note now points to the new call
    own = hdr[hdr.index("One large multi-scalar multiplication"):hdr.index("int bn254_g1_msm(")]
    for word in ("BN254_OPT_MSM_BUCKET_MIN", "BN254_OPT_MSM_WINDOW_BITS", "BN254_OPT_MSM_CHUNK", "Workspace", "BN254_E_BAD_ARG"):
        assert word in own, word


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    rust = B.rust_declarations(B.RUST_LIB.read_text())
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    txt = B.RUST_LIB.read_text()
    assert re.search(r"pub fn g1_msm\(p: &\[G1\], k: &\[Fr\]\) -> Result<G1, GpuError>", txt)
    assert re.search(r"pub fn g2_msm\(p: &\[G2\], k: &\[Fr\]\) -> Result<G2, GpuError>", txt)
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("G1 g1_msm(", "G2 g2_msm(", "bn254_g1_msm(", "bn254_g2_msm(", "bn254_g1_msm_multi(", "bn254_g2_msm_multi("):
        assert s in hpp, s


def test_the_three_options_are_mirrored():
    from bn_amd import _native
    enum = B.c_enum("BN254_OPT_")
    rust = B.rust_option_enum(B.RUST_LIB.read_text())
    assert B.option_mismatches(enum, rust) == []
    src = (ROOT / "bn_amd" / "csrc" / "bn254_hip.hip").read_text()
    for py, (cname, rname, value) in OPTIONS.items():
        assert enum[cname[len("BN254_OPT_"):]] == value and _native.OPTIONS[py] == value, py
        assert re.search(rf"\b{rname} = {value}\b", B.RUST_LIB.read_text()), rname
        assert f'{{"BN254_{py.upper()}", {cname}}}' in src, py                                   # the environment seed
        assert "BN254_" + py.upper() in B.HEADER.read_text()
    assert len(set(_native.OPTIONS.values())) == len(_native.OPTIONS) == 15


def test_python_surface():
    import inspect
    import bn_amd
    from bn_amd import engine
    for name in ("g1_msm", "g2_msm"):
        assert callable(getattr(bn_amd, name))
        assert list(inspect.signature(getattr(bn_amd, name)).parameters) == ["points", "scalars", "engine"]
        assert callable(getattr(engine.Engine, name)) and callable(getattr(engine.Engine, name + "_dev"))
        assert callable(getattr(engine.MultiEngine, name))
    assert callable(bn_amd.G1.msm) and callable(bn_amd.G2.msm)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


@pytest.mark.parametrize("case, p, k, n, out", [
    ("NULL p", None, DUMMY, 2, DUMMY),
    ("NULL k", DUMMY, None, 2, DUMMY),
    ("NULL out", DUMMY, DUMMY, 2, None),
    ("NULL out, no terms", None, None, 0, None),
    ("n > 2^40", DUMMY, DUMMY, (1 << 40) + 1, DUMMY),
])
def test_argument_errors_answer_without_a_device(lib, case, p, k, n, out):
    got = [lib.bn254_g1_msm(None, p, k, n, out), lib.bn254_g1_msm_dev(None, p, k, n, out, None),
           lib.bn254_g2_msm(None, p, k, n, out), lib.bn254_g2_msm_dev(None, p, k, n, out, None),
           lib.bn254_g1_msm_multi(None, p, k, n, out), lib.bn254_g2_msm_multi(None, p, k, n, out)]      # the arguments first, then the handle
    assert got == [BAD_ARG] * 6, case


def test_a_null_multi_handle_is_a_bad_argument(lib):
    assert lib.bn254_g1_msm_multi(None, None, None, 0, DUMMY) == BAD_ARG and lib.bn254_g2_msm_multi(None, None, None, 0, DUMMY) == BAD_ARG


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
    for short, args in (("bn254_g1_add_M", "MsmAccArgs"), ("bn254_g2_add_M", "MsmAccArgs"), ("bn254_g1_add_M", "MsmReduceArgs"), ("bn254_g2_add_M", "MsmReduceArgs"),
                        ("bn254_fr_decode_k", "MsmDigitsOp"), ("bn254_fr_decode_k", "MsmScanOp")):
        assert any(kernel_meta.short_name(n) == short and args in n for n in inst), (short, args)
        assert SPILL_CEILING[short] == 0
