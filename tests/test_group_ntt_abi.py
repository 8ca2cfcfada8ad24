"""Transforms over G1 and G2 (bn254_g{1,2}_ntt_batch and their _dev twins) without a GPU: the four declarations in every layer that mirrors
the C header, the Python surface, the argument checks that answer before any device is touched and their order, the test hook, and the
device code - further instances of kernel names that already have a register ceiling, reached through the shared launchers only."""
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
CSRC = ROOT / "bn_amd" / "csrc"

CONST = ("const",)
MUT = ("mut",)
CTX, FR_IN, N, INT = ("void", MUT), ("fr", CONST), ("usize", ()), ("int", ())
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_g1_ntt_batch": [CTX, ("g1", CONST), ("g1", MUT), INT, N, INT, FR_IN],
    "bn254_g2_ntt_batch": [CTX, ("g2", CONST), ("g2", MUT), INT, N, INT, FR_IN],
    "bn254_g1_ntt_batch_dev": [CTX, D_IN, D_OUT, INT, N, INT, FR_IN, D_OUT],
    "bn254_g2_ntt_batch_dev": [CTX, D_IN, D_OUT, INT, N, INT, FR_IN, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("g1_ntt", "g2_ntt", "g1_ntt_scale", "g2_ntt_scale", "g1_ntt_normalize", "g2_ntt_normalize")
BAD_ARG = -2


def test_header_declares_the_four_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert re.search(r"#define BN254_GROUP_NTT_LOG_MAX 22\b", hdr)
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    for name in NAMES:
        assert name in semantics, name
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_g{1,2}_ntt_batch serialise on the context" in threading and "bn254_g{1,2}_ntt_batch_dev" in threading
    own = " ".join(hdr[hdr.index("The same transforms over G1 and G2"):hdr.index("int bn254_g1_ntt_batch(")].split())
    for word in ("out[t n + k] = sum_j [s^j w_n^(j k)] in[t n + j]", "out[t n + j] = [n^-1 s^-j] sum_k [w_n^(-j k)] in[t n + k]", "NORMALISED", "exactly `in`", "HOST",
                 "BN254_E_BAD_ARG", "z == 0", "2^40", "n / 2 (log_n - 1) chains", "Stockham", "complete addition", "tools/time_group_ntt.py"):
        assert word in own, word
    assert "bn254_group_ntt_set_launch_max" not in hdr                                          # the test hook is internal
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    names = re.findall(r'"(\w+)"', block)
    assert set(SCOPES) <= set(names) and len(names) == len(set(names))


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
        assert f"pub fn {g.lower()}_ntt(points: &[{g}], log_n: u32, inverse: bool, shift: Option<&Fr>) -> Result<Vec<{g}>, GpuError>" in txt
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<G1> g1_ntt(const std::vector<G1> &points, int log_n, bool inverse = false, const Fr *shift = nullptr)",
              "std::vector<G2> g2_ntt(const std::vector<G2> &points, int log_n, bool inverse = false, const Fr *shift = nullptr)", "bn254_g1_ntt_batch(", "bn254_g2_ntt_batch("):
        assert s in hpp, s
    assert "bn254_group_ntt.hip" in [s.name for s in _native.SOURCES]
    assert (CSRC / "group_ntt_ops.hpp").exists()
    assert " bn254_group_ntt" in (ROOT / "tools" / "build_variant.sh").read_text()


def test_python_surface():
    import bn_amd
    from bn_amd import engine, kzg
    for g in ("g1", "g2"):
        assert list(inspect.signature(getattr(bn_amd, g + "_ntt")).parameters) == ["points", "inverse", "shift", "engine"]
        assert list(inspect.signature(getattr(bn_amd, g + "_ntt_batch")).parameters) == ["points", "log_n", "inverse", "shift", "engine"]
        host = inspect.signature(getattr(engine.Engine, g + "_ntt_batch"))
        assert list(host.parameters) == ["self", "p", "log_n", "inverse", "shift"]
        assert host.parameters["inverse"].default is False and host.parameters["shift"].default is None
        assert list(inspect.signature(getattr(engine.Engine, g + "_ntt_batch_dev")).parameters) == ["self", "d_in", "d_out", "log_n", "count", "inverse", "shift", "stream"]
    assert list(inspect.signature(kzg.lagrange_srs).parameters) == ["srs", "log_n", "engine"]
    assert list(inspect.signature(kzg.commit_evals).parameters) == ["lsrs", "evals", "engine"]
    assert list(inspect.signature(kzg.open_all).parameters) == ["srs", "p", "log_n", "engine"]
    assert kzg.LagrangeSRS._fields == ("g1_lagrange", "log_n", "g2_one", "tau_g2")
    src = inspect.getsource(kzg.lagrange_srs)
    assert src.count("g1_ntt_batch(") == 1 and "True" in src                                    # ONE inverse transform
    src = inspect.getsource(kzg.open_all)
    assert src.count("g1_ntt_batch(") == 3 and src.count("fr_ntt_batch(") == 2 and src.count("g1_mul_batch(") == 1 and "g1_msm" not in src


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def test_bad_lengths_raise_before_any_device_call():
    import numpy as np
    import bn_amd
    from bn_amd import engine
    for g, words in (("g1", 12), ("g2", 24)):
        one, batch = getattr(bn_amd, g + "_ntt"), getattr(bn_amd, g + "_ntt_batch")
        for n in (0, 3, 5, 6, 12):
            with pytest.raises(ValueError, match="power of two"):
                one(np.zeros((n, words), np.uint64), engine=NoDevice())
        with pytest.raises(ValueError, match="whole transforms"):
            batch(np.zeros((6, words), np.uint64), 2, engine=NoDevice())
        with pytest.raises(ValueError, match="0..22"):
            batch(np.zeros((4, words), np.uint64), 23, engine=NoDevice())
        with pytest.raises(ValueError, match="non-zero"):
            one(np.zeros((4, words), np.uint64), shift=0, engine=NoDevice())
        assert batch([], 3, engine=NoDevice()) == []
    with pytest.raises(ValueError, match="0..22"):
        engine._group_ntt_count(8, 23)
    with pytest.raises(ValueError, match="whole transforms"):
        engine._group_ntt_count(12, 3)
    assert engine._group_ntt_count(24, 3) == 3 and engine._group_ntt_count(0, 5) == 0


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


def _all(lib, a, out, log_n, count, inverse, shift):
    return [lib.bn254_g1_ntt_batch(None, a, out, log_n, count, inverse, shift), lib.bn254_g1_ntt_batch_dev(None, a, out, log_n, count, inverse, shift, None),
            lib.bn254_g2_ntt_batch(None, a, out, log_n, count, inverse, shift), lib.bn254_g2_ntt_batch_dev(None, a, out, log_n, count, inverse, shift, None)]


@pytest.mark.parametrize("case, a, out, log_n, count", [
    ("log_n < 0", DUMMY, DUMMY, -1, 1),
    ("log_n > 22", DUMMY, DUMMY, 23, 1),
    ("log_n > 22 before the pointers", None, None, 24, 1),
    ("NULL in", None, DUMMY, 3, 2),
    ("NULL out", DUMMY, None, 3, 2),
    ("count 2^log_n > 2^40", DUMMY, DUMMY, 0, (1 << 40) + 1),
    ("count 2^log_n > 2^40", DUMMY, DUMMY, 22, (1 << 18) + 1),
    ("count 2^log_n overflows", DUMMY, DUMMY, 22, 1 << 62),
])
def test_argument_errors_answer_without_a_device(lib, case, a, out, log_n, count):
    for inverse in (0, 1):
        assert _all(lib, a, out, log_n, count, inverse, None) == [BAD_ARG] * 4, case


def test_a_zero_shift_is_rejected_without_a_device(lib):
    zero = (C.c_uint64 * 4)(0, 0, 0, 0)
    for inverse in (0, 1):
        assert _all(lib, DUMMY, DUMMY, 3, 2, inverse, zero) == [BAD_ARG] * 4


def test_an_empty_call_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 24)(*([7] * 24))
    zero = (C.c_uint64 * 4)(0, 0, 0, 0)
    for p in (None, DUMMY):                                                                   # count == 0 is answered before the arguments
        for log_n in (-1, 0, 3, 99):
            assert _all(lib, p, out, log_n, 0, 0, None) == [0] * 4 and _all(lib, p, None, log_n, 0, 1, zero) == [0] * 4
    assert list(out) == [7] * 24


def test_the_hook_checks_its_bound(lib):
    lib.bn254_group_ntt_set_launch_max.argtypes = [C.c_size_t]
    try:
        assert lib.bn254_group_ntt_set_launch_max((1 << 22) + 1) == BAD_ARG
        assert lib.bn254_group_ntt_set_launch_max(4) == 0
    finally:
        assert lib.bn254_group_ntt_set_launch_max(0) == 0


def test_the_host_unit_reaches_the_kernels_through_the_shared_launchers_only():
    import lane_shell
    src = lane_shell.unit_source("bn254_group_ntt.hip")                                       # no kernel of its own
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert set(re.findall(r"\b(bn254_launch_\w+)\(", src)) == {"bn254_launch_group_ntt_stage_M", "bn254_launch_group_ntt_scale_M", "bn254_launch_normalize_M"}
    assert "bn_group_ntt_run(" in src and "bn_group_ntt_group(" in src and "bn_group_ntt_check(" in src and "bn_ntt_tables(" in src
    assert "bn_staged(" in src and src.count("bn_dev_entry(ctx, stream, true") == 1          # staging; the _dev forms under the scratch guard
    assert set(re.findall(r'"(g[12]_ntt\w*)"', src)) == set(SCOPES)
    # the bodies are pure per-lane functions of a header the host simulation shares
    ops = (CSRC / "group_ntt_ops.hpp").read_text()
    assert "__global__" not in ops and "threadIdx" not in ops and "blockIdx" not in ops
    assert '#include "../../bn_amd/csrc/group_ntt_ops.hpp"' in (ROOT / "tests" / "hostsim" / "hostsim_group_ntt.cpp").read_text()
    mul = (CSRC / "bn254_kernels_mul.hip").read_text()
    assert '#include "group_ntt_ops.hpp"' in mul
    for name in ("bn254_launch_group_ntt_stage_M", "bn254_launch_group_ntt_scale_M"):
        assert re.search(r"^int " + name + r"\(", mul, re.M), name
        assert name in (CSRC / "host_ctx.hpp").read_text()


def test_the_kernels_are_instances_of_names_with_a_ceiling():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    inst = kernel_meta.instances(so)
    spills = _instances(so)
    # stage 0, the stages with a chain, the passes: instances of the generic point kernels, which may not spill; their private memory is the
    # window-table setup of the chains, held to the ceiling of the term kernels that run the same chains
    from test_build_quality import PRIVATE_CEILING
    chain_private = PRIVATE_CEILING["bn254_g1_mul_M"]
    for args, private in (("GroupNttStageArgs", None), ("GroupNttChainArgs", chain_private), ("GroupNttPassArgs", chain_private)):
        for name in ("bn254_g1_add_M", "bn254_g2_add_M"):
            assert SPILL_CEILING[name] == 0
            mine = [n for n in inst if kernel_meta.short_name(n) == name and args in n]
            assert len(mine) == 1, (args, name, mine)
            assert inst[mine[0]]["spill"] == spills[mine[0]] == 0, (mine, inst[mine[0]])
            assert private is None or inst[mine[0]]["private"] <= private, (mine, inst[mine[0]])
    assert sorted({kernel_meta.short_name(n) for n in inst if "GroupNtt" in n}) == ["bn254_g1_add_M", "bn254_g2_add_M"]
    # the instance counts other tests pin stay as they were
    assert sum(kernel_meta.short_name(n) in ("bn254_g1_mul_M", "bn254_g2_mul_M") for n in inst) == 4
