"""Multi-scalar multiplication against prepared bases (bn254_g{1,2}_msm_prepare*, bn254_msm_prepared_*, bn254_g{1,2}_msm_prepared*) without
a GPU: the fourteen declarations in every layer that mirrors the C header, the argument checks that answer before any device or context
is touched, the Python surface, and the register budget of the device code - every kernel it added is a template instance of an existing
kernel name (bn254_g{1,2}_add_M<MsmAccPrepArgs|MsmPrepDoubleArgs>, bn254_fr_decode_k<MsmSignedDigitsOp>).  No option was added."""
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
VOID_C, VOID_M, SZ, INT = ("void", CONST), ("void", MUT), ("usize", ()), ("int", ())


def _prepare(g):
    return [VOID_M, (g, CONST), SZ, INT, ("void", ("mut", "mut"))]


def _call(g):
    return [VOID_M, VOID_C, SZ, ("fr", CONST), SZ, (g, MUT)]


PREPARE_DEV = [VOID_M, VOID_C, SZ, INT, ("void", ("mut", "mut")), VOID_M]
CALL_DEV = [VOID_M, VOID_C, SZ, VOID_C, SZ, VOID_M, VOID_M]
EXPECTED = {
    "bn254_g1_msm_prepare": (_prepare("g1"), INT), "bn254_g2_msm_prepare": (_prepare("g2"), INT),
    "bn254_g1_msm_prepare_dev": (PREPARE_DEV, INT), "bn254_g2_msm_prepare_dev": (PREPARE_DEV, INT),
    "bn254_msm_prepared_destroy": ([VOID_M], ("void", ())),
    "bn254_msm_prepared_count": ([VOID_C], SZ), "bn254_msm_prepared_bytes": ([VOID_C], SZ),
    "bn254_msm_prepared_group": ([VOID_C], INT), "bn254_msm_prepared_window_bits": ([VOID_C], INT),
    "bn254_msm_prepared_export": ([VOID_M, VOID_C, VOID_M, SZ], INT),
    "bn254_g1_msm_prepared": (_call("g1"), INT), "bn254_g2_msm_prepared": (_call("g2"), INT),
    "bn254_g1_msm_prepared_dev": (CALL_DEV, INT), "bn254_g2_msm_prepared_dev": (CALL_DEV, INT),
}
NAMES = tuple(EXPECTED)
SCOPES = tuple(f"g{g}_msmp_{s}" for g in (1, 2) for s in ("table", "digits", "bucket", "reduce"))
BAD_ARG = -2


def test_header_declares_the_fourteen_entry_points():
    assert len(NAMES) == 14
    decls = B.c_declarations()
    for name, (params, ret) in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ret, name
    hdr = B.HEADER.read_text()
    assert "bn254_msm_prepared" not in re.sub(r"bn254_msm_prepared_\w+", "", hdr), "the handle is a plain void * in the header: no struct name"
    for s in SCOPES:
        assert f'"{s}"' in hdr, s
    own = hdr[hdr.index("multi-scalar multiplication against PREPARED bases"):hdr.index("int bn254_g1_msm_prepare(")]
    for word in ("BN254_OPT_MSM_BUCKET_MIN", "BN254_OPT_MSM_CHUNK", "BN254_E_BAD_ARG", "window_bits", "first + n > count", "80-byte", "(0, 1, 0)"):
        assert word in own, word
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_g{1,2}_msm_prepared_dev" in threading


def test_no_option_was_added():
    from bn_amd import _native
    assert B.c_enum("BN254_OPT_")["COUNT_"] == 16
    assert len(set(_native.OPTIONS.values())) == len(_native.OPTIONS) == 15
    assert B.option_mismatches(B.c_enum("BN254_OPT_"), B.rust_option_enum(B.RUST_LIB.read_text())) == []


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    rust = B.rust_declarations(B.RUST_LIB.read_text())
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    txt = B.RUST_LIB.read_text()
    for g in ("G1", "G2"):
        assert re.search(rf"pub struct PreparedMsm{g}\(\*mut c_void\);", txt)
        assert re.search(rf"pub fn new\(p: &\[{g}\], window_bits: i32\) -> Result<PreparedMsm{g}, GpuError>", txt)
        assert re.search(rf"pub fn msm\(&self, first: usize, k: &\[Fr\]\) -> Result<{g}, GpuError>", txt)
        assert re.search(rf"impl Drop for PreparedMsm{g} \{{\s*fn drop\(&mut self\) \{{ unsafe \{{ bn254_msm_prepared_destroy\(self\.0\) \}} \}}", txt)
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    assert "class PreparedMsm" in hpp
    for name in NAMES:
        assert name + "(" in hpp, name


def test_python_surface():
    import bn_amd
    from bn_amd import engine, groth16, kzg, mkzg
    params = lambda f: list(inspect.signature(f).parameters)
    E = engine.Engine
    for g in ("g1", "g2"):
        assert params(getattr(E, f"{g}_msm_prepare")) == ["self", "points", "window_bits"]
        assert inspect.signature(getattr(E, f"{g}_msm_prepare")).parameters["window_bits"].default is None
        assert params(getattr(E, f"{g}_msm_prepare_dev"))[:3] == ["self", "d_p", "n"]
        assert params(getattr(E, f"{g}_msm_prepared")) == ["self", "prep", "k", "first"]
        assert inspect.signature(getattr(E, f"{g}_msm_prepared")).parameters["first"].default == 0
        assert params(getattr(E, f"{g}_msm_prepared_dev")) == ["self", "prep", "first", "d_k", "n", "d_out", "stream"]
        assert params(getattr(bn_amd, f"{g}_msm_prepare")) == ["points", "window_bits", "engine"]
    P = engine.PreparedMSM
    assert bn_amd.PreparedMSM is P
    for prop in ("count", "group", "window_bits", "device_bytes"):
        assert isinstance(getattr(P, prop), property), prop
    assert params(P.msm) == ["self", "scalars", "first"] and inspect.signature(P.msm).parameters["first"].default == 0
    assert callable(P.export) and callable(P.close) and callable(P.__del__)
    assert params(kzg.prepare)[0] == "srs" and params(mkzg.prepare)[0] == "srs" and params(groth16.prepare_proving_key)[0] == "pk"
    assert kzg.PreparedSRS._fields == kzg.SRS._fields + ("prepared",) and kzg.PreparedLagrangeSRS._fields == kzg.LagrangeSRS._fields + ("prepared",)
    assert groth16.PreparedProvingKey._fields == groth16.ProvingKey._fields + ("prepared",)
    assert mkzg.PreparedSRS._fields == mkzg.SRS._fields + ("prepared",)


def test_a_closed_handle_raises_without_a_device():
    from bn_amd import _native, engine
    h = engine.PreparedMSM(None, None)
    for use in (lambda: h.count, lambda: h.group, lambda: h.window_bits, lambda: h.device_bytes, h.export, lambda: h.msm([])):
        with pytest.raises(_native.Bn254Error):
            use()
    h.close(); h.close()


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


@pytest.mark.parametrize("case, p, n, bits, out", [
    ("NULL p", None, 2, 0, True),
    ("NULL out", DUMMY, 2, 0, False),
    ("NULL out, no points", None, 0, 0, False),
    ("window_bits 1", DUMMY, 2, 1, True),
    ("window_bits 2", DUMMY, 2, 2, True),
    ("window_bits 17", DUMMY, 2, 17, True),
    ("window_bits -1", DUMMY, 2, -1, True),
    ("W * count = 2^31 at c = 16", DUMMY, 1 << 27, 16, True),
    ("W * count >= 2^31 at c = 3", DUMMY, ((1 << 31) + 84) // 85, 3, True),
    ("W * count >= 2^31 at the default width", DUMMY, 1 << 28, 0, True),
    ("n > 2^40", DUMMY, (1 << 40) + 1, 16, True),
])
def test_prepare_argument_errors_answer_without_a_context(lib, case, p, n, bits, out):
    h = C.c_void_p(0xdead)
    o = C.byref(h) if out else None
    got = [lib.bn254_g1_msm_prepare(None, p, n, bits, o), lib.bn254_g2_msm_prepare(None, p, n, bits, o),
           lib.bn254_g1_msm_prepare_dev(None, p, n, bits, o, None), lib.bn254_g2_msm_prepare_dev(None, p, n, bits, o, None)]
    assert got == [BAD_ARG] * 4, case


class _Handle(C.Structure):
    """the library's private handle, as far as the checks read it (bn_amd/csrc/host_ctx.hpp bn254_msm_prepared): built by hand here so that the
    checks of a call can be reached without a device.  table and pts stay NULL: nothing may follow them."""
    _fields_ = [("device", C.c_int), ("group", C.c_int), ("c", C.c_uint), ("W", C.c_uint), ("count", C.c_size_t), ("table", C.c_void_p), ("pts", C.c_void_p),
                ("table_bytes", C.c_size_t)]


def _handle(g, count, c=13):
    return _Handle(0, g, c, (254 + c - 1) // c, count, None, None, ((254 + c - 1) // c) * count * 80 * g)


@pytest.mark.parametrize("case, g_handle, first, k, n, out", [
    ("NULL handle", None, 0, DUMMY, 2, DUMMY),
    ("NULL k", 0, 0, None, 2, DUMMY),
    ("NULL out", 0, 0, DUMMY, 2, None),
    ("NULL out, no terms", 0, 0, None, 0, None),
    ("first + n one past the end", 0, 3, DUMMY, 8, DUMMY),
    ("first past the end, no terms", 0, 11, None, 0, DUMMY),
    ("first + n wraps around", 0, (1 << 64) - 1, DUMMY, 2, DUMMY),
    ("a handle of the other group", 1, 0, DUMMY, 2, DUMMY),
])
def test_call_argument_errors_answer_without_a_context(lib, case, g_handle, first, k, n, out):
    """g_handle: None, or 0 for a handle of the call's own group and 1 for one of the other group; the handles hold 10 points"""
    for g in (1, 2):
        hs = None if g_handle is None else _handle(g if g_handle == 0 else 3 - g, 10)
        ref = None if hs is None else C.byref(hs)
        f, fd = getattr(lib, f"bn254_g{g}_msm_prepared"), getattr(lib, f"bn254_g{g}_msm_prepared_dev")
        assert [f(None, ref, first, k, n, out), fd(None, ref, first, k, n, out, None)] == [BAD_ARG] * 2, (case, g)


def test_handle_queries_and_export_checks(lib):
    h = _handle(2, 10, 16)
    ref = C.byref(h)
    assert (lib.bn254_msm_prepared_count(ref), lib.bn254_msm_prepared_group(ref), lib.bn254_msm_prepared_window_bits(ref)) == (10, 2, 16)
    assert lib.bn254_msm_prepared_bytes(ref) == 16 * 10 * 160 + 10 * 192
    h1 = _handle(1, 1 << 20, 16)
    assert lib.bn254_msm_prepared_bytes(C.byref(h1)) == 16 * (1 << 20) * 80 + (1 << 20) * 96          # 1.34 GB of table, 0.1 GB of points
    assert (lib.bn254_msm_prepared_count(None), lib.bn254_msm_prepared_bytes(None), lib.bn254_msm_prepared_group(None), lib.bn254_msm_prepared_window_bits(None)) == (0, 0, 0, 0)
    lib.bn254_msm_prepared_destroy(None)                                                               # harmless
    assert lib.bn254_msm_prepared_export(None, None, DUMMY, 0) == BAD_ARG
    assert lib.bn254_msm_prepared_export(None, ref, DUMMY, 16 * 10 * 160 - 1) == BAD_ARG              # not the table's size
    assert lib.bn254_msm_prepared_export(None, ref, None, 16 * 10 * 160) == BAD_ARG


def test_defaults_the_library_reports(lib):
    """the default width is host_plan.hpp's function and the table the sweep recorded (tests/test_host_plan_msm_prepared.py checks the
    function on every size); the default crossover is one value per group, the one the profile's crossover lines state"""
    from test_host_plan_msm_prepared import recorded_width_table
    lib.bn254_msm_prepared_default_window_bits.restype = C.c_uint; lib.bn254_msm_prepared_default_window_bits.argtypes = [C.c_size_t]
    lib.bn254_msm_prepared_default_min.restype = C.c_long; lib.bn254_msm_prepared_default_min.argtypes = [C.c_int]
    for (g, lg), c in recorded_width_table().items():
        assert lib.bn254_msm_prepared_default_window_bits(1 << lg) == c, (g, lg)
    text = (ROOT / "profiles" / "r29_msm_prepared.txt").read_text()
    for g in (1, 2):
        m = re.search(rf"^# G{g} crossover: (never|2\^(\d+))", text, re.M)
        assert m, g
        want = (1 << 40) + 1 if m.group(1) == "never" else 1 << int(m.group(2))                      # never: above every batch the library takes
        assert lib.bn254_msm_prepared_default_min(g) == want, (g, m.group(0))


def test_profile_scopes_are_in_the_host_unit():
    src = (ROOT / "bn_amd" / "csrc" / "bn254_seg.hip").read_text()
    for s in ("table", "digits", "bucket", "reduce"):
        assert f'g == 1 ? "g1_msmp_{s}" : "g2_msmp_{s}"' in src, s


def test_every_new_kernel_is_a_known_name_at_zero_spills():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    inst = _instances(so)
    for short, args in (("bn254_g1_add_M", "MsmAccPrepArgs"), ("bn254_g2_add_M", "MsmAccPrepArgs"), ("bn254_g1_add_M", "MsmPrepDoubleArgs"),
                        ("bn254_g2_add_M", "MsmPrepDoubleArgs"), ("bn254_fr_decode_k", "MsmSignedDigitsOp")):
        hit = [n for n in inst if kernel_meta.short_name(n) == short and args in n]
        assert len(hit) == 1, (short, args, hit)
        assert SPILL_CEILING[short] == 0 and inst[hit[0]] == 0, (hit[0], inst[hit[0]])
    assert set(kernel_meta.short_name(n) for n in inst) <= set(SPILL_CEILING)                           # no new kernel name
