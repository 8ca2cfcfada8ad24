"""The batched multi-pairing over prepared points (bn254_pairing_product_batch_prepared_native*) without a GPU: its declarations in every layer
that mirrors the C header, the argument checks that answer before any device is touched, the register budget of the device code it added
(instances of existing kernel names: bn254_miller_native_shared4_B<true> is the segmented Miller loop, bn254_tile_k<true> the gather of the
small route) and the Python surface."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import test_binding_signatures as B
from test_product_batch_abi import _instances

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

NAMES = ("bn254_pairing_product_batch_prepared_native", "bn254_pairing_product_batch_prepared_native_dev")
CONST = ("const",)
MUT = ("mut",)
EXPECTED = {
    "bn254_pairing_product_batch_prepared_native": [("void", MUT), ("g1", CONST), ("void", CONST), ("usize", CONST), ("usize", CONST), ("usize", ()), ("gt", MUT)],
    "bn254_pairing_product_batch_prepared_native_dev": [("void", MUT), ("void", CONST), ("void", CONST), ("void", CONST), ("usize", CONST), ("usize", ()), ("void", MUT),
                                                        ("void", MUT)],
}
BAD_ARG = -2


def test_header_declares_both_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert "bn254_pairing_product_batch_prepared_native" in hdr[:hdr.index("Error behaviour")]                     # the "Semantics replaced" list
    assert "bn254_pairing_product_batch_prepared_native" in hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    stats = re.search(r"/\* kernel: (.*?)\n", hdr).group(1)
    assert '"miller_native_seg"' in stats
    # the header says what an index the host cannot check does
    dev_doc = hdr[hdr.index("bn254_pairing_product_batch_prepared_native on device-resident"):hdr.index("int bn254_pairing_product_batch_prepared_native_dev")]
    assert "memory safe" in dev_doc and "identity" in dev_doc


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    rust = B.rust_declarations(B.RUST_LIB.read_text())
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    txt = B.RUST_LIB.read_text()
    assert re.search(r"pub fn pairing_product_batch\(&self, p: &\[G1\], q_index: Option<&\[usize\]>, offsets: &\[usize\]\) -> Result<Vec<Gt>, GpuError>", txt)
    assert re.search(r"pub fn pairing_check_batch\(&self, p: &\[G1\], q_index: Option<&\[usize\]>, offsets: &\[usize\]\) -> Result<Vec<bool>, GpuError>", txt)
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    cls = hpp[hpp.index("class PreparedG2"):hpp.index("// tunables of the default context")]
    assert "pairing_product_batch(" in cls and "pairing_check_batch(" in cls and "bn254_pairing_product_batch_prepared_native(" in cls


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


def _sz(vals):
    return (C.c_size_t * len(vals))(*vals)


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


def _call_all(lib, p, prep, qi, offsets, m, out):
    """both entry points with the same arguments (ctx NULL: the checks come before the default context's device lookup)"""
    return [lib.bn254_pairing_product_batch_prepared_native(None, p, prep, qi, offsets, m, out),
            lib.bn254_pairing_product_batch_prepared_native_dev(None, p, prep, qi, offsets, m, out, None)]


@pytest.mark.parametrize("case, offs, m, p, prep, out", [
    ("offsets NULL with m > 0", None, 2, DUMMY, DUMMY, DUMMY),
    ("offsets[0] != 0", [1, 2, 3], 2, DUMMY, DUMMY, DUMMY),
    ("decreasing offsets", [0, 3, 2, 4], 3, DUMMY, DUMMY, DUMMY),
    ("n > 2^40", [0, 1, (1 << 40) + 1], 2, DUMMY, DUMMY, DUMMY),
    ("NULL p", [0, 2], 1, None, DUMMY, DUMMY),
    ("NULL out", [0, 2], 1, DUMMY, DUMMY, None),
    ("NULL out, no pairs", [0, 0], 1, None, DUMMY, None),
    ("NULL prep", [0, 2], 1, DUMMY, None, DUMMY),
    ("NULL prep, no pairs", [0, 0], 1, None, None, DUMMY),
])
def test_argument_errors_answer_without_a_device(lib, case, offs, m, p, prep, out):
    o = _sz(offs) if offs is not None else None
    assert _call_all(lib, p, prep, None, o, m, out) == [BAD_ARG, BAD_ARG], case
    # (what needs the handle's contents - an index >= count, n > count without indices, a handle of another device - needs a real handle,
    # which needs a GPU: tests/test_gpu_product_batch_prepared.py::test_index_conventions_and_errors)


def test_no_segments_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 48)(*([7] * 48))
    for offs in (None, _sz([0]), _sz([5])):                        # m == 0: offsets are not even read, nor is the handle
        assert _call_all(lib, None, None, None, offs, 0, out) == [0, 0]
    assert list(out) == [7] * 48


def test_spill_ceiling_of_every_instance_of_the_touched_kernels():
    """tests/test_build_quality.py checks one instance per short name; the templates this feature made give two each - both must stay at the
    name's ceiling (0 spilled VGPRs for the native shared Miller kernel and the tile / gather kernel), and the Miller kernel keeps its two
    waves per SIMD (amdgpu_waves_per_eu(BN_WAVES, BN_WAVES): at most 256 VGPRs)"""
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    ceilings = {k: SPILL_CEILING[k] for k in ("bn254_miller_native_shared4_B", "bn254_tile_k")}
    assert ceilings == {"bn254_miller_native_shared4_B": 0, "bn254_tile_k": 0}
    seen = {k: [] for k in ceilings}
    for name, s in _instances(so).items():
        short = kernel_meta.short_name(name)
        if short in ceilings:
            seen[short].append(name)
            assert s <= ceilings[short], f"{name}: {s} spilled VGPRs, ceiling {ceilings[short]}"
    for short, names in seen.items():
        assert len(names) == 2 and any("ILb0E" in n for n in names) and any("ILb1E" in n for n in names), seen       # the plain and the new instance
    src = (ROOT / "bn_amd" / "csrc" / "bn254_kernels_b.hip").read_text()
    decl = src[src.index("template <bool SEG>\n__global__"):]
    decl = decl[:decl.index("{")]
    assert "bn254_miller_native_shared4_B" in decl and "amdgpu_waves_per_eu(BN_WAVES, BN_WAVES)" in decl
    assert kernel_meta.kernel_meta(so)["bn254_miller_native_shared4_B"]["vgpr"] <= 256


def test_python_surface():
    import bn_amd
    from bn_amd import engine, groth16
    assert callable(engine.Engine.pairing_product_batch_prepared_native) and callable(engine.Engine.pairing_product_batch_prepared_native_dev)
    assert list(inspect.signature(engine.Engine.pairing_product_batch_prepared_native).parameters) == ["self", "p", "prepared", "offsets", "q_index"]
    assert list(inspect.signature(bn_amd.PreparedG2.pairing_product_batch).parameters) == ["self", "segments", "q_index", "offsets"]
    assert list(inspect.signature(bn_amd.PreparedG2.pairing_check_batch).parameters) == ["self", "segments", "q_index", "offsets"]
    sig = inspect.signature(groth16.verify_batch)
    assert list(sig.parameters) == ["vk", "proofs", "public_inputs", "engine", "prepared"] and sig.parameters["prepared"].default is False


def test_python_argument_errors_need_no_device():
    """the ValueErrors of the Python layer are raised before the library is asked for anything"""
    from bn_amd import Fr, groth16
    from bn_amd.engine import Engine

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was used ({name})")
    vk = groth16.VerifyingKey(None, None, None, None, [None, None, None])
    for prepared in (False, True):
        with pytest.raises(ValueError):
            groth16.verify_batch(vk, [(None, None, None)], [], engine=NoDevice(), prepared=prepared)                      # one proof, no inputs
        with pytest.raises(ValueError):
            groth16.verify_batch(vk, [(None, None, None)], [[Fr.one()]], engine=NoDevice(), prepared=prepared)            # one input, the key takes two
        assert groth16.verify_batch(vk, [], [], engine=NoDevice(), prepared=prepared).shape == (0,)
    eng = object.__new__(Engine)                                                            # no context: only the argument checks may run
    eng._ctx = None
    p = np.zeros((5, 12), np.uint64)
    with pytest.raises(ValueError):
        Engine.pairing_product_batch_prepared_native(eng, p, None, [0, 2, 4])                # offsets end at 4, five pairs given
    with pytest.raises(ValueError):
        Engine.pairing_product_batch_prepared_native(eng, p, None, [0, 2, 5], q_index=[0, 1, 2])     # three indices for five pairs
    with pytest.raises(ValueError):
        Engine.pairing_product_batch_prepared_native(eng, p, None, [], q_index=None)         # no offsets at all
