"""Segmented scans over Fr (bn254_fr_scan_batch and its _dev twin), bn_amd.poly's users of them and bn_amd.kzg, without a GPU: the two
declarations in every layer that mirrors the C header, the argument checks that answer before any device is touched, the profiling scopes,
the Python surface and its errors, the test hooks, and the register budget of the device code - the kernels are template instances of an
existing kernel name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import fr_cases as FC
import scan_cases as SC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST = ("const",)
MUT = ("mut",)
CTX, FR_IN, FR_OUT, N, FLAGS = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ()), ("int", ())
D_IN, D_OUT, OFF = ("void", CONST), ("void", MUT), ("usize", CONST)
EXPECTED = {
    "bn254_fr_scan_batch": [CTX, FR_IN, FR_IN, FR_IN, OFF, N, FLAGS, FR_OUT],
    "bn254_fr_scan_batch_dev": [CTX, D_IN, D_IN, D_IN, OFF, N, FLAGS, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("fr_scan", "fr_scan_reduce", "fr_scan_up", "fr_scan_down")
HOOKS = ("bn254_fr_scan_piece", "bn254_fr_scan_fan", "bn254_fr_scan_set_launch_max", "bn254_fr_scan_set_piece")
BAD_ARG = -2


def test_header_declares_the_two_entry_points_and_the_flags():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert re.search(r"unsigned int flags, bn_fr \*out\);", hdr) and re.search(r"unsigned int flags, void \*d_out,", hdr)
    flags = dict(re.findall(r"#define BN254_SCAN_(\w+) (\d+)", hdr))
    assert flags == {"REVERSE": "1", "EXCLUSIVE": "2", "A_PER_SEGMENT": "4"}
    assert (SC.REVERSE, SC.EXCLUSIVE, SC.A_PER_SEGMENT) == (1, 2, 4)
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    for name in NAMES:
        assert name in semantics, name
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_fr_scan_batch serialises on the context" in threading and "bn254_fr_scan_batch_dev" in threading
    own = " ".join(hdr[hdr.index("Segmented scans over Fr"):hdr.index("#define BN254_SCAN_REVERSE")].split())
    for word in ("out[t] = a[t] * prev + b[t]", "a == NULL", "b == NULL", "init == NULL", "BN254_SCAN_REVERSE", "BN254_SCAN_EXCLUSIVE", "BN254_SCAN_A_PER_SEGMENT", "canonical",
                 "An empty segment writes nothing", "HOST", "BN254_E_BAD_ARG", "2 u + 3", "Threading"):
        assert word in own, word
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook


def test_the_scope_names_are_documented_and_used():
    hdr = B.HEADER.read_text()
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    lines = [l for l in block.split("\n") if '"fr_scan"' in l]
    assert len(lines) == 1 and re.findall(r'"(\w+)"', lines[0]) == list(SCOPES)                 # a line of their own
    names = re.findall(r'"(\w+)"', block)
    assert len(names) == len(set(names))
    src = (ROOT / "bn_amd" / "csrc" / "bn254_scan.hip").read_text()
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
    assert "pub fn fr_scan(a: Option<&[Fr]>, b: Option<&[Fr]>, init: Option<&[Fr]>, offsets: &[usize], flags: c_int) -> Result<Vec<Fr>, GpuError>" in txt
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<Fr> fr_scan(", "bn254_fr_scan_batch("):
        assert s in hpp, s
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "bn254_fr_scan_batch" in (ROOT / doc).read_text(), doc
    assert "bn254_scan.hip" in [s.name for s in _native.SOURCES]
    assert (ROOT / "bn_amd" / "csrc" / "scan_ops.hpp").exists()
    assert " bn254_scan" in (ROOT / "tools" / "build_variant.sh").read_text()


def test_python_surface():
    import bn_amd
    from bn_amd import engine, groth16, kzg, poly
    assert list(inspect.signature(bn_amd.fr_scan_batch).parameters) == ["a", "b", "offsets", "init", "reverse", "exclusive", "a_per_segment", "engine"]
    E = engine.Engine
    sig = inspect.signature(E.fr_scan_batch)
    assert list(sig.parameters) == ["self", "a", "b", "offsets", "init", "reverse", "exclusive", "a_per_segment"]
    assert sig.parameters["init"].default is None and [sig.parameters[k].default for k in ("reverse", "exclusive", "a_per_segment")] == [False] * 3
    assert list(inspect.signature(E.fr_scan_batch_dev).parameters)[:7] == ["self", "d_a", "d_b", "d_init", "offsets", "m", "d_out"]
    assert engine._scan_flags(True, False, True) == 5 and engine._scan_flags(False, True, False) == 2
    assert list(inspect.signature(poly.evaluate).parameters)[:2] == ["p", "z"] and list(inspect.signature(poly.divide_linear).parameters)[:2] == ["p", "z"]
    assert list(inspect.signature(poly.powers).parameters)[:2] == ["x", "n"]
    assert inspect.getsource(poly._horner).count("fr_scan_batch(") == 1 and inspect.getsource(poly.powers).count("fr_scan_batch(") == 1
    assert kzg.SRS._fields == ("g1_powers", "g2_one", "tau_g2")
    assert list(inspect.signature(kzg.setup).parameters)[:2] == ["n", "rng"]
    assert list(inspect.signature(kzg.commit).parameters)[:2] == ["srs", "p"] and list(inspect.signature(kzg.open).parameters)[:3] == ["srs", "p", "z"]
    assert list(inspect.signature(kzg.verify).parameters)[:5] == ["srs", "c", "z", "y", "proof"]
    assert list(inspect.signature(kzg.verify_batch).parameters)[:5] == ["srs", "cs", "zs", "ys", "proofs"]
    assert "tests and development" in kzg.setup.__doc__.lower()
    src = inspect.getsource(kzg.verify_batch)
    assert src.count("g1_msm_batch(") == 1 and src.count("g1_add_batch(") == 1 and src.count("pairing_check_batch(") == 1
    src = inspect.getsource(kzg.setup)
    assert src.count("poly.powers(") == 1 and src.count("g1_mul_base_batch(") == 1 and src.count("g2_mul_base_batch(") == 1
    src = inspect.getsource(groth16.setup)
    assert "poly.powers(" in src and "powers.append" not in src


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def test_bad_arguments_raise_before_any_device_call_and_name_the_operand():
    import bn_amd
    from bn_amd import kzg
    one = [bn_amd.Fr.one()]
    scan = lambda *a, **k: bn_amd.fr_scan_batch(*a, engine=NoDevice(), **k)
    with pytest.raises(ValueError, match="a and b are both None"):
        scan(None, None, [0, 3])
    for offsets in ([1, 3], [0, 2, 1, 3], []):
        with pytest.raises(ValueError, match="offsets"):
            scan(one * 3, one * 3, offsets)
    with pytest.raises(ValueError, match="^b holds 3 terms"):
        scan(one * 4, one * 3, [0, 4])
    with pytest.raises(ValueError, match="^a holds 3 records"):
        scan(one * 3, one * 4, [0, 4])
    with pytest.raises(ValueError, match="^a holds 4 records but a_per_segment"):
        scan(one * 4, one * 4, [0, 1, 4], a_per_segment=True)
    with pytest.raises(ValueError, match="^init holds 1 values"):
        scan(one * 4, one * 4, [0, 1, 4], init=one)
    with pytest.raises(ValueError, match="^a holds 3 records"):
        scan(np.zeros((3, 4), np.uint64), None, np.array([0, 4]))
    srs = kzg.SRS(np.zeros((4, 12), np.uint64), None, None)
    for f in (kzg.commit, lambda s, p, engine: kzg.open(s, p, one[0], engine=engine)):
        with pytest.raises(ValueError, match="5 coefficients"):
            f(srs, one * 5, engine=NoDevice())
    with pytest.raises(ValueError, match="2 commitments, 1 points"):
        kzg.verify_batch(srs, [None, None], one, one * 2, [None, None], engine=NoDevice())
    with pytest.raises(ValueError, match="at least one power"):
        kzg.setup(0, None, engine=NoDevice())


def test_poly_and_kzg_over_a_stand_in_engine_that_answers_from_the_model():
    """divide_linear is ONE reverse scan with a = z per segment and b = p; powers ONE exclusive scan with init one"""
    from bn_amd import Fr, poly
    calls = []

    class Model:
        def fr_scan_batch(self, a, b, offsets, init=None, reverse=False, exclusive=False, a_per_segment=False):
            calls.append((None if a is None else len(a), None if b is None else len(b), [int(v) for v in offsets], reverse, exclusive, a_per_segment))
            ints = lambda v: None if v is None else [Fr.from_limbs(r).v for r in np.asarray(v).reshape(-1, 4)]
            return FC.rows(SC.model(ints(a), ints(b), offsets, ints(init), reverse=reverse, exclusive=exclusive, a_per_segment=a_per_segment))
    p = [Fr(v) for v in SC.values(9, 3)]
    z = Fr(77)
    q, y = poly.divide_linear(p, z, engine=Model())
    assert calls == [(1, 9, [0, 9], True, False, True)]
    assert y == Fr(sum(c.v * pow(77, i, FC.R) for i, c in enumerate(p))) and len(q) == 8
    assert poly.evaluate(p, z, engine=Model()) == y and len(calls) == 2
    back = [Fr.zero()] * 9
    for i, c in enumerate(q):
        back[i + 1] = back[i + 1] + c
        back[i] = back[i] - c * z
    back[0] = back[0] + y
    assert back == p
    del calls[:]
    assert poly.powers(z, 5, engine=Model()) == [Fr(pow(77, i, FC.R)) for i in range(5)]
    assert calls == [(1, None, [0, 5], False, True, True)]
    assert poly.powers(z, 0, engine=NoDevice()) == [] and poly.divide_linear([], z, engine=NoDevice()) == ([], Fr.zero()) and poly.evaluate([], z, engine=NoDevice()) == Fr.zero()
    assert poly.powers(Fr.zero(), 3, engine=Model()) == [Fr.one(), Fr.zero(), Fr.zero()]
    assert poly.powers(z, 4, engine=Model(), limbs=True).shape == (4, 4)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_scan_piece.argtypes = []; l.bn254_fr_scan_piece.restype = C.c_uint
    l.bn254_fr_scan_fan.argtypes = []; l.bn254_fr_scan_fan.restype = C.c_uint
    l.bn254_fr_scan_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_fr_scan_set_piece.argtypes = [C.c_uint]
    return l


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


def _off(*v):
    return (C.c_size_t * len(v))(*v)


def _both(lib, a, b, init, offsets, m, flags, out):
    return [lib.bn254_fr_scan_batch(None, a, b, init, offsets, m, flags, out), lib.bn254_fr_scan_batch_dev(None, a, b, init, offsets, m, flags, out, None)]


@pytest.mark.parametrize("case, a, b, offsets, m, flags, out", [
    ("both operands NULL", None, None, _off(0, 1, 3), 2, 0, DUMMY),
    ("an unknown flag bit", DUMMY, DUMMY, _off(0, 1, 3), 2, 8, DUMMY),
    ("an unknown flag bit beside known ones", DUMMY, DUMMY, _off(0, 1, 3), 2, 7 | 64, DUMMY),
    ("decreasing offsets", DUMMY, DUMMY, _off(0, 4, 3), 2, 0, DUMMY),
    ("offsets[0] != 0", DUMMY, DUMMY, _off(1, 2, 3), 2, 0, DUMMY),
    ("offsets == NULL with m > 0", DUMMY, DUMMY, None, 2, 0, DUMMY),
    ("n > 2^40", DUMMY, DUMMY, _off(0, (1 << 40) + 1), 1, 0, DUMMY),
    ("a NULL out", DUMMY, DUMMY, _off(0, 1, 3), 2, 0, None),
    ("a NULL out, only empty segments", DUMMY, None, _off(0, 0, 0), 2, 0, None),
    ("both operands NULL, only empty segments", None, None, _off(0, 0, 0), 2, 0, DUMMY),
])
def test_argument_errors_answer_without_a_device(lib, case, a, b, offsets, m, flags, out):
    for init in (None, DUMMY):
        assert _both(lib, a, b, init, offsets, m, flags, out) == [BAD_ARG] * 2, case


def test_an_empty_call_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 8)(*([7] * 8))
    for p in (None, DUMMY):                                                                     # m == 0 is answered before the arguments
        for offsets in (None, _off(5)):
            assert _both(lib, p, p, p, offsets, 0, 0, out) == [0] * 2 and _both(lib, p, p, p, offsets, 0, 99, None) == [0] * 2
    for flags in range(8):                                                                      # n == 0: after the arguments, before any device
        assert _both(lib, DUMMY, None, None, _off(0, 0, 0, 0), 3, flags, out) == [0] * 2
        assert _both(lib, None, DUMMY, DUMMY, _off(0, 0), 1, flags, out) == [0] * 2
    assert list(out) == [7] * 8


def test_the_hooks_check_their_bounds(lib):
    P, F = lib.bn254_fr_scan_piece(), lib.bn254_fr_scan_fan()
    assert P in (8, 16, 32, 64) and F in (2, 4, 16)                                             # the ones the host simulation runs
    try:
        assert lib.bn254_fr_scan_set_piece(65) == BAD_ARG and lib.bn254_fr_scan_set_piece(8) == 0 and lib.bn254_fr_scan_set_piece(64) == 0
        assert lib.bn254_fr_scan_set_launch_max((1 << 22) + 1) == BAD_ARG
        assert lib.bn254_fr_scan_set_launch_max(20) == 0
    finally:
        assert lib.bn254_fr_scan_set_piece(0) == 0 and lib.bn254_fr_scan_set_launch_max(0) == 0
    assert lib.bn254_fr_scan_piece() == P


def test_the_kernels_are_instances_of_fr_decode_k_and_spill_nothing():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    import lane_shell
    src = lane_shell.unit_source("bn254_scan.hip")  # the unit adds no kernel under any other name: the shell is lane_launch.hpp's
    assert "bn_lane_launch<SCAN_BLOCK>(" in src and "SCAN_BLOCK = 256" in src
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    meta = kernel_meta.instances(so)
    mine = [n for n in meta if kernel_meta.short_name(n) == "bn254_fr_decode_k" and "FrScanOp" in n]
    assert len(mine) == 4, mine                                                                 # reduce, up, down, apply
    for n in mine:
        assert meta[n]["spill"] == 0 and meta[n]["private"] == 0 and meta[n]["lds"] == 0, (n, meta[n])
