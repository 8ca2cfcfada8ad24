"""The batched multi-pairing (bn254_pairing_product_batch*) without a GPU: its declarations in every layer that mirrors the C header, the
argument checks that answer before any device is touched, and the register budget of the device code it added (instances of existing
kernel names: bn254_gt_mul_B<true> is the segmented fold, bn254_gt_tail_W<true> the ragged tail)."""
import ctypes as C
import pathlib
import re
import sys

import pytest

import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

NAMES = ("bn254_pairing_product_batch", "bn254_pairing_product_batch_dev", "bn254_pairing_product_batch_multi")
CONST = ("const",)
MUT = ("mut",)
EXPECTED = {
    "bn254_pairing_product_batch": [("void", MUT), ("g1", CONST), ("g2", CONST), ("usize", CONST), ("usize", ()), ("gt", MUT)],
    "bn254_pairing_product_batch_dev": [("void", MUT), ("void", CONST), ("void", CONST), ("usize", CONST), ("usize", ()), ("void", MUT), ("void", MUT)],
    "bn254_pairing_product_batch_multi": [("void", MUT), ("g1", CONST), ("g2", CONST), ("usize", CONST), ("usize", ()), ("gt", MUT)],
}
BAD_ARG = -2


def test_header_declares_the_three_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    semantics = hdr[:hdr.index("Error behaviour")]
    assert "bn254_pairing_product_batch" in semantics                     # the "Semantics replaced" list
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_pairing_product_batch" in threading
    stats = re.search(r"/\* kernel: (.*?)\n", hdr).group(1)
    assert '"gt_segment"' in stats and '"gt_tail_seg"' in stats


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    rust = B.rust_declarations(B.RUST_LIB.read_text())
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    txt = B.RUST_LIB.read_text()
    assert re.search(r"pub fn pairing_product_batch\(p: &\[G1\], q: &\[G2\], offsets: &\[usize\]\) -> Result<Vec<Gt>, GpuError>", txt)
    assert re.search(r"pub fn pairing_check_batch\(p: &\[G1\], q: &\[G2\], offsets: &\[usize\]\) -> Result<Vec<bool>, GpuError>", txt)
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert "bn254_pairing_product_batch" in md
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    assert "pairing_product_batch(" in hpp and "pairing_check_batch(" in hpp and "bn254_pairing_product_batch_multi(" in hpp


def test_python_surface():
    import bn_amd
    from bn_amd import engine
    for name in ("pairing_product_batch", "pairing_check_batch"):
        assert callable(getattr(bn_amd, name))
    assert callable(engine.Engine.pairing_product_batch) and callable(engine.Engine.pairing_product_batch_dev)
    assert callable(engine.MultiEngine.pairing_product_batch)


def _offsets(vals):
    a = (C.c_size_t * len(vals))(*vals)
    return a


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


def _call_all(lib, p, q, offsets, m, out):
    """both single-device entry points with the same arguments (ctx NULL: the checks come before the default context's device lookup)"""
    return [lib.bn254_pairing_product_batch(None, p, q, offsets, m, out),
            lib.bn254_pairing_product_batch_dev(None, p, q, offsets, m, out, None)]


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


@pytest.mark.parametrize("case, offs, m, p, q, out", [
    ("offsets NULL with m > 0", None, 2, DUMMY, DUMMY, DUMMY),
    ("offsets[0] != 0", [1, 2, 3], 2, DUMMY, DUMMY, DUMMY),
    ("decreasing offsets", [0, 3, 2, 4], 3, DUMMY, DUMMY, DUMMY),
    ("n > 2^40", [0, 1, (1 << 40) + 1], 2, DUMMY, DUMMY, DUMMY),
    ("NULL p", [0, 2], 1, None, DUMMY, DUMMY),
    ("NULL q", [0, 2], 1, DUMMY, None, DUMMY),
    ("NULL out", [0, 2], 1, DUMMY, DUMMY, None),
    ("NULL out, no pairs", [0, 0], 1, None, None, None),
])
def test_argument_errors_answer_without_a_device(lib, case, offs, m, p, q, out):
    o = _offsets(offs) if offs is not None else None
    assert _call_all(lib, p, q, o, m, out) == [BAD_ARG, BAD_ARG], case
    # (the multi entry point needs a handle, which needs a GPU: with a NULL one the code cannot tell a bad offset from the missing
    # handle - its offset checks on a real handle are in tests/test_gpu_product_batch.py::test_multi_engine_matches_one_engine)


def test_no_segments_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 48)(*([7] * 48))
    for offs in (None, _offsets([0]), _offsets([5])):                        # m == 0: offsets are not even read
        assert _call_all(lib, None, None, offs, 0, out) == [0, 0]
        assert lib.bn254_pairing_product_batch_multi(None, None, None, offs, 0, out) == 0          # m == 0 is answered before the handle
    assert list(out) == [7] * 48


def _instances(so):
    """{full mangled name: vgpr_spill_count} of every kernel in the library's gfx950 code objects"""
    import kernel_meta
    return {name: m["spill"] for name, m in kernel_meta.instances(so).items()}


def test_spill_ceiling_of_every_instance_of_the_fold_kernels():
    """tests/test_build_quality.py checks one instance per short name; the templates added here give two each - both must stay at the
    name's ceiling (0 for the lane-pair product and the wave tail, 2 for the product tree)"""
    import isa_mix
    import kernel_meta
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    ceilings = {"bn254_gt_mul_B": 0, "bn254_gt_tail_W": 0, "bn254_gt_reduce_W": 2}
    spills = _instances(so)
    seen = {k: [] for k in ceilings}
    for name, s in spills.items():
        short = kernel_meta.short_name(name)
        if short in ceilings:
            seen[short].append(name)
            assert s <= ceilings[short], f"{name}: {s} spilled VGPRs, ceiling {ceilings[short]}"
    assert len(seen["bn254_gt_mul_B"]) == 2 and len(seen["bn254_gt_tail_W"]) == 2, seen       # the plain and the segmented instance
    assert any("ILb1E" in n for n in seen["bn254_gt_mul_B"]) and any("ILb1E" in n for n in seen["bn254_gt_tail_W"]), seen
