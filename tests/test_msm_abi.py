"""The segmented multi-scalar multiplication (bn254_g{1,2}_msm_batch*) without a GPU: its declarations in every layer that mirrors the C
header, the argument checks that answer before any device is touched, and the register budget of the device code it added - template
instances of existing kernel names: bn254_g{1,2}_mul_M<true> is the term kernel (the GLV / GLS chain without normalisation),
bn254_g{1,2}_add_M<true> the segmented fold."""
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
    return [("void", MUT), (g, CONST), ("fr", CONST), ("usize", CONST), ("usize", ()), (g, MUT)]


DEV = [("void", MUT), ("void", CONST), ("void", CONST), ("usize", CONST), ("usize", ()), ("void", MUT), ("void", MUT)]
EXPECTED = {
    "bn254_g1_msm_batch": _host("g1"), "bn254_g2_msm_batch": _host("g2"),
    "bn254_g1_msm_batch_dev": DEV, "bn254_g2_msm_batch_dev": DEV,
    "bn254_g1_msm_batch_multi": _host("g1"), "bn254_g2_msm_batch_multi": _host("g2"),
}
NAMES = tuple(EXPECTED)
SCOPES = ("g1_msm_mul", "g1_msm_fold", "g2_msm_mul", "g2_msm_fold")
BAD_ARG = -2


def test_header_declares_the_six_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    semantics = hdr[:hdr.index("Error behaviour")]
    assert "bn254_g1_msm_batch" in semantics and "bn254_g2_msm_batch" in semantics              # the "Semantics replaced" list
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "msm_batch" in threading
    stats = re.search(r"/\* kernel: (.*?)\n", hdr).group(1)
    for s in SCOPES + ("g1_mul", "g2_add", "gt_segment"):                                       # appended: the old names stay on the line
        assert f'"{s}"' in stats, s
    note = hdr[hdr.index("Segmented multi-scalar multiplication"):hdr.index("int bn254_g1_msm_batch(")]
    assert "Pippenger" in note                                                                   # the limit is stated where the call is declared


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    rust = B.rust_declarations(B.RUST_LIB.read_text())
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    txt = B.RUST_LIB.read_text()
    assert re.search(r"pub fn g1_msm_batch\(p: &\[G1\], k: &\[Fr\], offsets: &\[usize\]\) -> Result<Vec<G1>, GpuError>", txt)
    assert re.search(r"pub fn g2_msm_batch\(p: &\[G2\], k: &\[Fr\], offsets: &\[usize\]\) -> Result<Vec<G2>, GpuError>", txt)
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert "bn254_g1_msm_batch" in md and "bn254_g2_msm_batch" in md
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("g1_msm_batch(", "g2_msm_batch(", "bn254_g1_msm_batch(", "bn254_g2_msm_batch(", "bn254_g1_msm_batch_multi(", "bn254_g2_msm_batch_multi("):
        assert s in hpp, s


def test_python_surface():
    import bn_amd
    from bn_amd import engine, groth16
    for name in ("g1_msm_batch", "g2_msm_batch"):
        assert callable(getattr(bn_amd, name))
        assert callable(getattr(engine.Engine, name)) and callable(getattr(engine.Engine, name + "_dev"))
        assert callable(getattr(engine.MultiEngine, name))
    assert callable(bn_amd.G1.msm) and callable(bn_amd.G2.msm)
    assert callable(groth16.verify_batch)
    assert groth16.VerifyingKey._fields == ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "ic")


def _offsets(vals):
    return (C.c_size_t * len(vals))(*vals)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


def _call_all(lib, p, k, offsets, m, out):
    """the four single-device entry points with the same arguments (ctx NULL: the checks come before the default context's device lookup)"""
    return [lib.bn254_g1_msm_batch(None, p, k, offsets, m, out), lib.bn254_g1_msm_batch_dev(None, p, k, offsets, m, out, None),
            lib.bn254_g2_msm_batch(None, p, k, offsets, m, out), lib.bn254_g2_msm_batch_dev(None, p, k, offsets, m, out, None)]


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


@pytest.mark.parametrize("case, offs, m, p, k, out", [
    ("offsets NULL with m > 0", None, 2, DUMMY, DUMMY, DUMMY),
    ("offsets[0] != 0", [1, 2, 3], 2, DUMMY, DUMMY, DUMMY),
    ("decreasing offsets", [0, 3, 2, 4], 3, DUMMY, DUMMY, DUMMY),
    ("n > 2^40", [0, 1, (1 << 40) + 1], 2, DUMMY, DUMMY, DUMMY),
    ("NULL p", [0, 2], 1, None, DUMMY, DUMMY),
    ("NULL k", [0, 2], 1, DUMMY, None, DUMMY),
    ("NULL out", [0, 2], 1, DUMMY, DUMMY, None),
    ("NULL out, no terms", [0, 0], 1, None, None, None),
])
def test_argument_errors_answer_without_a_device(lib, case, offs, m, p, k, out):
    o = _offsets(offs) if offs is not None else None
    assert _call_all(lib, p, k, o, m, out) == [BAD_ARG] * 4, case
    # with a NULL handle the multi entry points answer the same way (they check the segments first, then the handle)
    assert lib.bn254_g1_msm_batch_multi(None, p, k, o, m, out) == BAD_ARG and lib.bn254_g2_msm_batch_multi(None, p, k, o, m, out) == BAD_ARG


def test_no_segments_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 24)(*([7] * 24))
    for offs in (None, _offsets([0]), _offsets([5])):                        # m == 0: offsets are not even read
        assert _call_all(lib, None, None, offs, 0, out) == [0] * 4
        assert lib.bn254_g1_msm_batch_multi(None, None, None, offs, 0, out) == 0          # m == 0 is answered before the handle
        assert lib.bn254_g2_msm_batch_multi(None, None, None, offs, 0, out) == 0
    assert list(out) == [7] * 24


CEILINGS = {"bn254_g1_add_M": 0, "bn254_g2_add_M": 0, "bn254_g1_mul_M": 7, "bn254_g2_mul_M": 0}      # tests/test_build_quality.py SPILL_CEILING


def _library():
    import isa_mix
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists() or not (isa_mix.LLVM / "llvm-objdump").exists():
        pytest.skip("library or the LLVM tools not present")
    return so


def test_spill_ceiling_of_every_instance_of_the_group_kernels():
    """tests/test_build_quality.py sees one instance per short name; here every name has two - the plain kernel and the <true> instance -
    and both stay at the name's ceiling"""
    import kernel_meta
    seen = {k: [] for k in CEILINGS}
    for name, s in _instances(_library()).items():
        short = kernel_meta.short_name(name)
        if short in CEILINGS:
            seen[short].append(name)
            assert s <= CEILINGS[short], f"{name}: {s} spilled VGPRs, ceiling {CEILINGS[short]}"
    for short, names in seen.items():
        assert len(names) >= 2, seen
        assert any(short + "E" in n for n in names), (short, names)            # the plain, non-template kernel is still there
        assert any(short + "ILb1E" in n for n in names), (short, names)        # ... beside the <true> instance


def test_private_segment_of_the_term_kernels():
    """both instances of bn254_g{1,2}_mul_M keep their private segment (the window-table setup) below PRIVATE_CEILING of test_build_quality.py"""
    import subprocess
    import tempfile
    import kernel_meta
    d = _library().read_bytes()
    offs = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", d)]
    found = {}
    with tempfile.TemporaryDirectory() as t:
        for i, o in enumerate(offs):
            e = offs[i + 1] if i + 1 < len(offs) else len(d)
            b = pathlib.Path(t) / f"b{i}.bin"; b.write_bytes(d[o:e])
            co = pathlib.Path(t) / f"k{i}.co"
            subprocess.check_call([str(kernel_meta.LLVM / "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--input={b}", f"--output={co}", "--unbundle"])
            txt = subprocess.check_output([str(kernel_meta.LLVM / "llvm-readelf"), "--notes", str(co)], text=True)
            for blk in txt.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if kernel_meta.short_name(name) in ("bn254_g1_mul_M", "bn254_g2_mul_M"):
                    found[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert len(found) == 4, found
    assert all(v <= 1400 for v in found.values()), found


def test_window_loops_of_the_term_kernels_do_not_store_to_scratch():
    """the block scan of test_scalar_multiplication_loops_do_not_store_to_scratch on the template instances (mangled ...mul_MILb1E...), with
    the same rule: from the fourth big block from the end to the end of the function there is no scratch store.  These kernels have no
    normalisation after the loop, so the region starts at the doubling block (G1: doubling, the two halves of the mixed addition, the
    epilogue that leaves the isomorphic curve and converts the limbs) or one block earlier (G2) - never later."""
    import isa_mix
    so = _library()
    for kernel in ("bn254_g1_mul_MILb1E", "bn254_g2_mul_MILb1E"):
        blocks = []                                   # (instructions, scratch stores) of every basic block, in address order
        for text in isa_mix.disassemble(so):
            on = False; n = st = 0
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    if on and n: blocks.append((n, st))
                    on = kernel in m.group(1); n = st = 0; continue
                if not on: continue
                m = re.match(r"^\s+([a-z_0-9]+)\s", line)
                if not m: continue
                op = m.group(1); n += 1
                if op.startswith("scratch_store"): st += 1
                if op.startswith(("s_cbranch", "s_branch")):
                    blocks.append((n, st)); n = st = 0
            if on and n: blocks.append((n, st))
        big = [i for i, (n, _) in enumerate(blocks) if n >= 900]
        assert len(big) >= 4, (kernel, blocks)
        region = blocks[big[-4]:]
        assert sum(st for _, st in region) == 0, f"scratch stores inside the window loop of {kernel}: {region}"
