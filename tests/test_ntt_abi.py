"""Number-theoretic transforms over Fr (bn254_fr_ntt_batch, its _dev twin, bn254_fr_root_of_unity) without a GPU: the three declarations in
every layer that mirrors the C header, the Python surface, the argument checks that answer before any device is touched, the root of every
size, the model the other tests compare against (tests/ntt_cases.py) against the sums of the definition, the test hooks, and the register
budget of the device code - the kernels are template instances of an existing kernel name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import fr_cases as FC
import ntt_cases as NC
import test_binding_signatures as B
from test_product_batch_abi import _instances

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST = ("const",)
MUT = ("mut",)
CTX, FR_IN, FR_OUT, N, INT = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ()), ("int", ())
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_fr_root_of_unity": [INT, FR_OUT],
    "bn254_fr_ntt_batch": [CTX, FR_IN, FR_OUT, INT, N, INT, FR_IN],
    "bn254_fr_ntt_batch_dev": [CTX, D_IN, D_OUT, INT, N, INT, FR_IN, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("ntt", "ntt_table")
OPS = ("NttPassOp", "NttTableOp")
BAD_ARG = -2


def test_header_declares_the_three_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert re.search(r"#define BN254_NTT_LOG_MAX 24\b", hdr)
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    for name in NAMES:
        assert name in semantics, name
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_fr_ntt_batch serialises on the context" in threading and "bn254_fr_ntt_batch_dev" in threading
    own = " ".join(hdr[hdr.index("Number-theoretic transforms"):hdr.index("int bn254_fr_root_of_unity(")].split())
    for word in ("19103219067921713944291392827692070036145651957329286315305642004821462161904", "w_28^(2^(28 - log_n))", "out[t n + k] = sum_j in[t n + j] s^j w_n^(j k)",
                 "out[t n + j] = s^-j n^-1 sum_k in[t n + k] w_n^(-j k)", "canonical", "exactly `in`", "HOST", "BN254_E_BAD_ARG", "Fr::zero()", "2^40", "512 KiB",
                 "profiles/r14_ntt.txt", "Threading"):
        assert word in own, word


def test_no_new_type_and_no_new_option():
    hdr = B.HEADER.read_text()
    types = "".join(re.findall(r"typedef[^;]*;", hdr))
    assert "ntt" not in types
    assert B.c_enum("BN254_OPT_")["COUNT_"] == 16
    for hook in ("bn254_ntt_tile_log", "bn254_ntt_set_tile_log", "bn254_ntt_set_launch_max"):             # the test hooks are internal
        assert hook not in hdr, hook


def test_the_scope_names_follow_the_pinned_line():
    hdr = B.HEADER.read_text()
    first = re.search(r"/\* kernel: (.*?)\n", hdr).group(1)
    assert "ntt" not in first                                                                     # the first line stays as other tests pin it
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    names = re.findall(r'"(\w+)"', block)
    assert tuple(names[-2:]) == SCOPES and len(names) == len(set(names))
    src = (ROOT / "bn_amd" / "csrc" / "bn254_ntt.hip").read_text()
    assert set(re.findall(r'BnScope \w+\(\w+, \w+, "(\w+)"\)', src)) == set(SCOPES)
    assert set(re.findall(r'"(fr_\w+)"', (ROOT / "bn_amd" / "csrc" / "bn254_fr.hip").read_text())) == {"fr_add", "fr_mul", "fr_inverse", "fr_pow", "fr_interpret"}


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
    assert "pub fn fr_ntt(values: &[Fr], log_n: u32, inverse: bool, shift: Option<&Fr>) -> Result<Vec<Fr>, GpuError>" in txt
    assert "pub fn fr_root_of_unity(log_n: u32) -> Result<Fr, GpuError>" in txt
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<Fr> fr_ntt(const std::vector<Fr> &values, int log_n, bool inverse = false, const Fr *shift = nullptr)", "Fr fr_root_of_unity(int log_n)",
              "bn254_fr_ntt_batch(", "bn254_fr_root_of_unity("):
        assert s in hpp, s
    for doc in ("README.md", "DESIGN.md"):
        txt = (ROOT / doc).read_text()
        assert "bn254_fr_ntt_batch" in txt and "profiles/r14_ntt.txt" in txt, doc
    assert "bn254_ntt.hip" in [s.name for s in _native.SOURCES]
    assert (ROOT / "bn_amd" / "csrc" / "ntt_ops.hpp").exists()
    assert " bn254_ntt" in (ROOT / "tools" / "build_variant.sh").read_text()


def test_python_surface():
    import bn_amd
    from bn_amd import engine, poly
    assert list(inspect.signature(bn_amd.fr_ntt).parameters) == ["values", "inverse", "shift", "engine"]
    assert list(inspect.signature(bn_amd.fr_ntt_batch).parameters) == ["rows", "inverse", "shift", "engine"]
    E = engine.Engine
    assert list(inspect.signature(E.fr_ntt_batch).parameters) == ["self", "a", "log_n", "inverse", "shift"]
    assert inspect.signature(E.fr_ntt_batch).parameters["inverse"].default is False and inspect.signature(E.fr_ntt_batch).parameters["shift"].default is None
    assert list(inspect.signature(E.fr_ntt_batch_dev).parameters) == ["self", "d_in", "d_out", "log_n", "count", "inverse", "shift", "stream"]
    assert list(inspect.signature(poly.mul).parameters) == ["a", "b", "engine"]
    assert list(inspect.signature(poly.quotient).parameters) == ["a_evals", "b_evals", "c_evals", "engine"]
    Fr = bn_amd.Fr
    assert Fr.root_of_unity(28) == Fr(NC.ROOT_28) and Fr.root_of_unity(0) == Fr.one() and Fr.root_of_unity(1) == Fr(FC.R - 1)
    for log_n in range(29):
        assert Fr.root_of_unity(log_n).v == NC.root(log_n)
    for bad in (-1, 29):
        with pytest.raises(ValueError):
            Fr.root_of_unity(bad)
    assert "engine" not in inspect.getsource(Fr.root_of_unity)
    src = inspect.getsource(poly.mul)
    assert src.count("fr_ntt_batch(") == 2 and src.count("fr_mul_batch(") == 1
    src = inspect.getsource(poly.quotient)
    assert src.count("fr_ntt_batch(") == 3 and src.count("fr_mul_batch(") == 2 and src.count("fr_add_batch(") == 1 and "negate_b=True" in src


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def test_bad_lengths_raise_before_any_device_call():
    import bn_amd
    from bn_amd import poly
    Fr = bn_amd.Fr
    one = [Fr.one()]
    for n in (0, 3, 5, 6, 12):
        with pytest.raises(ValueError, match="power of two"):
            bn_amd.fr_ntt(one * n, engine=NoDevice())
        with pytest.raises(ValueError, match="power of two"):
            poly.quotient(one * n, one * n, one * n, engine=NoDevice())
    with pytest.raises(ValueError, match="power of two"):
        bn_amd.fr_ntt(np.zeros((6, 4), np.uint64), engine=NoDevice())
    with pytest.raises(ValueError, match="same length"):
        bn_amd.fr_ntt_batch([one * 4, one * 8], engine=NoDevice())
    with pytest.raises(ValueError, match="non-zero"):
        bn_amd.fr_ntt(one * 4, shift=Fr.zero(), engine=NoDevice())
    for a, b, c in ((4, 4, 8), (4, 8, 4), (8, 4, 4)):
        with pytest.raises(ValueError, match="differ in length"):
            poly.quotient(one * a, one * b, one * c, engine=NoDevice())
    assert poly.mul([], one, engine=NoDevice()) == [] and poly.mul(one, [], engine=NoDevice()) == []
    assert bn_amd.fr_ntt_batch([], engine=NoDevice()) == []


def test_the_shift_outlives_its_conversion():
    """Engine.fr_ntt_batch[_dev] convert a shift that is a list, a strided view or another dtype into a fresh array: the C call must see ITS
    bytes, so the array has to live in the calling frame until the call returns (a bare address of a freed temporary would not do).  The
    library is a stand-in that churns the allocator and then reads the 32 bytes it was handed."""
    from bn_amd import engine
    want = np.array([0x1111111111111111, 0x2222222222222222, 0x3333333333333333, 0x0444444444444444], np.uint64)
    seen = []

    class Lib:
        @staticmethod
        def _read(p):
            junk = [np.full(4, 0xdeaddeaddeaddead, np.uint64) for _ in range(256)]           # reuses whatever small blocks are free
            seen.append(C.string_at(p, 32) if p is not None else None)
            del junk
            return 0
        def bn254_ctx_destroy(self, h): pass
        def bn254_fr_ntt_batch(self, h, a, out, log_n, count, inverse, shift): return self._read(shift)
        def bn254_fr_ntt_batch_dev(self, h, a, out, log_n, count, inverse, shift, stream): return self._read(shift)
    e = engine.Engine.__new__(engine.Engine)
    e._lib, e._ctx = Lib(), 1                                                                    # a handle the stand-in never looks at
    wide = np.zeros(8, np.uint64); wide[::2] = want
    shifts = ([int(x) for x in want], tuple(int(x) for x in want), wide[::2], want.astype(object), want)
    for sh in shifts:
        e.fr_ntt_batch(np.zeros((4, 4), np.uint64), 2, False, sh)
        e.fr_ntt_batch_dev(0x1000, 0x2000, 2, 1, True, sh, 0)
    assert seen == [want.tobytes()] * (2 * len(shifts))
    e.fr_ntt_batch(np.zeros((4, 4), np.uint64), 2)
    assert seen[-1] is None
    assert isinstance(engine._ntt_shift([1, 2, 3, 4]), np.ndarray) and engine._ntt_shift(None) is None
    with pytest.raises(ValueError, match="ONE scalar"):
        engine._ntt_shift([1, 2, 3])


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is rejected before the data is read


def _both(lib, a, out, log_n, count, inverse, shift):
    return [lib.bn254_fr_ntt_batch(None, a, out, log_n, count, inverse, shift), lib.bn254_fr_ntt_batch_dev(None, a, out, log_n, count, inverse, shift, None)]


@pytest.mark.parametrize("case, a, out, log_n, count", [
    ("log_n < 0", DUMMY, DUMMY, -1, 1),
    ("log_n > 24", DUMMY, DUMMY, 25, 1),
    ("NULL in", None, DUMMY, 3, 2),
    ("NULL out", DUMMY, None, 3, 2),
    ("count 2^log_n > 2^40", DUMMY, DUMMY, 0, (1 << 40) + 1),
    ("count 2^log_n > 2^40", DUMMY, DUMMY, 24, (1 << 16) + 1),
    ("count 2^log_n overflows", DUMMY, DUMMY, 24, 1 << 62),
])
def test_argument_errors_answer_without_a_device(lib, case, a, out, log_n, count):
    for inverse in (0, 1):
        assert _both(lib, a, out, log_n, count, inverse, None) == [BAD_ARG] * 2, case


def test_a_zero_shift_is_rejected_without_a_device(lib):
    zero = (C.c_uint64 * 4)(0, 0, 0, 0)
    for inverse in (0, 1):
        assert _both(lib, DUMMY, DUMMY, 3, 2, inverse, zero) == [BAD_ARG] * 2


def test_an_empty_call_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 8)(*([7] * 8))
    zero = (C.c_uint64 * 4)(0, 0, 0, 0)
    for p in (None, DUMMY):                                                                   # count == 0 is answered before the arguments
        for log_n in (-1, 0, 3, 99):
            assert _both(lib, p, out, log_n, 0, 0, None) == [0] * 2 and _both(lib, p, None, log_n, 0, 1, zero) == [0] * 2
    assert list(out) == [7] * 8


def test_root_of_unity(lib):
    out = np.zeros(4, np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.bn254_fr_root_of_unity(28, p) == 0 and np.array_equal(out, FC.rows([NC.ROOT_28])[0])
    assert lib.bn254_fr_root_of_unity(0, p) == 0 and np.array_equal(out, FC.rows([1])[0])
    from bn_amd import Fr
    for log_n in range(1, 29):
        assert lib.bn254_fr_root_of_unity(log_n, p) == 0
        w = Fr.from_limbs(out).v
        assert pow(w, 1 << (log_n - 1), FC.R) == FC.R - 1, log_n                                # w_n^(n/2) = -1: the order is exactly n
        assert w == pow(NC.ROOT_28, 1 << (28 - log_n), FC.R), log_n
    before = out.copy()
    assert lib.bn254_fr_root_of_unity(29, p) == BAD_ARG and lib.bn254_fr_root_of_unity(-1, p) == BAD_ARG and lib.bn254_fr_root_of_unity(3, None) == BAD_ARG
    assert np.array_equal(out, before)


@pytest.mark.parametrize("log_n", range(7))
def test_the_model_equals_the_sums_of_the_definition(log_n):
    from bn_amd import Fr
    assert Fr.root_of_unity(log_n).v == NC.root(log_n)                                          # the model and the package agree on the root
    for name, x in NC.inputs(log_n, seed=40 + log_n).items():
        for sh in NC.SHIFTS:
            for inverse in (False, True):
                assert NC.ntt(x, inverse, sh) == NC.naive(x, inverse, sh), (name, sh, inverse)
            assert NC.ntt(NC.ntt(x, False, sh), True, sh) == x, (name, sh)
    n = 1 << log_n
    sets = NC.inputs(log_n, seed=1)
    c = sets["constant"][0]
    assert NC.ntt(sets["delta 0"]) == [c] * n and NC.ntt(sets["constant"]) == [n * c % FC.R] + [0] * (n - 1)
    if n > 1:
        assert NC.ntt(sets["delta 1"]) == [c * pow(NC.root(log_n), k, FC.R) % FC.R for k in range(n)]
    ks = list(range(n))
    terms = [(j, v) for j, v in enumerate(sets["random"])]
    assert NC.sparse_outputs(terms, log_n, ks, False, 5) == NC.ntt(sets["random"], False, 5)
    assert NC.sparse_outputs(terms, log_n, ks, True, 5) == NC.ntt(sets["random"], True, 5)


def test_the_hooks_check_their_bounds(lib):
    lib.bn254_ntt_tile_log.argtypes = []; lib.bn254_ntt_tile_log.restype = C.c_uint
    lib.bn254_ntt_set_tile_log.argtypes = [C.c_uint]
    lib.bn254_ntt_set_launch_max.argtypes = [C.c_size_t]
    T = lib.bn254_ntt_tile_log()
    assert 8 <= T <= 11                                                                         # the measured ones
    try:
        assert lib.bn254_ntt_set_tile_log(T + 1) == BAD_ARG
        assert lib.bn254_ntt_set_tile_log(1) == 0 and lib.bn254_ntt_set_tile_log(T) == 0
        assert lib.bn254_ntt_set_launch_max((1 << 22) + 1) == BAD_ARG
        assert lib.bn254_ntt_set_launch_max(64) == 0
    finally:
        assert lib.bn254_ntt_set_tile_log(0) == 0 and lib.bn254_ntt_set_launch_max(0) == 0
    assert lib.bn254_ntt_tile_log() == T


def test_the_kernels_are_instances_of_fr_decode_k_and_spill_nothing():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    inst = _instances(so)
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    for op in OPS:
        mine = [n for n in inst if kernel_meta.short_name(n) == "bn254_fr_decode_k" and op in n]
        assert len(mine) >= 1, op
        assert all(inst[n] == 0 for n in mine), mine
    # the unit adds no kernel under any other name
    import lane_shell
    lane_shell.unit_source("bn254_ntt.hip")      # the unit adds no kernel of its own: the shell is lane_launch.hpp's
