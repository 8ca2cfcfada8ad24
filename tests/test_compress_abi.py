"""The compressed G1 / G2 encodings (bn254_g{1,2}_compress_batch, bn254_g{1,2}_decompress_batch and their _dev twins) without a GPU: the eight
symbols and their declarations in every layer that mirrors the C header, the argument checks that answer before any device is touched, the
Python surface and its errors over a stand-in engine that answers from the integer model of compress_cases.py, the round trip of
groth16.encode_proofs / decode_proofs over it, and the register budget of the device code - the kernels are template instances of two existing
kernel names (bn254_fr_decode_k<Op>, bn254_g2_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import bn_model as M
import compress_cases as CC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, N, INT, BYTES_IN, BYTES_OUT, ST = ("void", MUT), ("usize", ()), ("int", ()), ("u8", CONST), ("u8", MUT), ("i32", MUT)
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_g1_compress_batch": [CTX, ("g1", CONST), INT, BYTES_OUT, N],
    "bn254_g2_compress_batch": [CTX, ("g2", CONST), INT, BYTES_OUT, N],
    "bn254_g1_decompress_batch": [CTX, BYTES_IN, INT, ("g1", MUT), ST, N],
    "bn254_g2_decompress_batch": [CTX, BYTES_IN, INT, ("g2", MUT), ST, N],
    "bn254_g1_compress_batch_dev": [CTX, D_IN, INT, D_OUT, N, D_OUT],
    "bn254_g2_compress_batch_dev": [CTX, D_IN, INT, D_OUT, N, D_OUT],
    "bn254_g1_decompress_batch_dev": [CTX, D_IN, INT, D_OUT, D_OUT, N, D_OUT],
    "bn254_g2_decompress_batch_dev": [CTX, D_IN, INT, D_OUT, D_OUT, N, D_OUT],
}
NAMES = tuple(EXPECTED)
HOOKS = ("bn254_compress_set_launch_max", "bn254_compress_sqrt_window")
SCOPES = ("g1_compress", "g2_compress", "g1_decompress", "g2_decompress")
BAD_ARG = -2
WIRE_N_MAX = 0x7fffffff // 129


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_compress_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_compress_sqrt_window.argtypes = []
    return l


def test_every_new_symbol_resolves():
    """fails on the commit before the family: the library has none of them"""
    from bn_amd import _native
    raw = C.CDLL(str(_native.LIB_PATH))
    for name in NAMES + HOOKS:
        assert getattr(raw, name), name
    assert set(NAMES) <= set(_native.SIGNATURES)
    for name in NAMES:
        assert len(_native.SIGNATURES[name]) == len(EXPECTED[name]), name


def test_header_declares_the_eight_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    for d in ("BN254_COMPRESSED_ARK 0", "BN254_COMPRESSED_GNARK 1", "BN254_G1_COMPRESSED_BYTES 32", "BN254_G2_COMPRESSED_BYTES 64"):
        assert re.search(r"^#define " + d + "$", hdr, re.M), d
    own = " ".join(hdr[hdr.index("/* Compressed encodings"):hdr.index("#define BN254_COMPRESSED_ARK")].split())
    for word in ("laid out as ark-serialize / gnark-crypto describe; not checked against those libraries here", "LAST byte", "FIRST byte", "bit 7 = sign(y)",
                 "y > -y", "c1 is compared first", "G::zero()", "decompress(compress(p)) == decode(encode(p))", "compress(decompress(b)) == b", "BN254_E_BAD_ARG",
                 "n == 0 succeeds", "bn254_pairing_product_batch_dev"):
        assert word in own, word
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for text in (semantics, threading):
        for name in ("bn254_g{1,2}_compress_batch", "bn254_g{1,2}_decompress_batch", "bn254_g{1,2}_compress_batch_dev", "bn254_g{1,2}_decompress_batch_dev"):
            assert name in text, name
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"g1_compress"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)
    src = (ROOT / "bn_amd" / "csrc" / "bn254_wire.hip").read_text()
    assert set(SCOPES) <= set(re.findall(r'"(\w+)"', src))


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn g1_compress_batch(p: &[G1], format: CompressedFormat) -> Result<Vec<u8>, GpuError>",
               "pub fn g2_compress_batch(p: &[G2], format: CompressedFormat) -> Result<Vec<u8>, GpuError>",
               "pub fn g1_decompress_batch(records: &[u8], format: CompressedFormat) -> Result<Vec<Result<G1, i32>>, GpuError>",
               "pub fn g2_decompress_batch(records: &[u8], format: CompressedFormat) -> Result<Vec<Result<G2, i32>>, GpuError>"):
        assert fn in txt, fn
    assert "CompressedFormat::Ark => 0, CompressedFormat::Gnark => 1" in txt
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<uint8_t> g1_compress(", "std::vector<uint8_t> g2_compress(", "std::vector<G1> g1_decompress(", "std::vector<G2> g2_decompress(",
              "bn254_g1_compress_batch(", "bn254_g2_compress_batch(", "bn254_g1_decompress_batch(", "bn254_g2_decompress_batch("):
        assert s in hpp, s
    note = "laid out as ark-serialize / gnark-crypto describe; not checked against those libraries here"
    assert note in " ".join(hpp.split()) and note in " ".join((ROOT / "README.md").read_text().split())
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        for name in ("bn254_g{1,2}_compress_batch", "bn254_g{1,2}_decompress_batch"):
            assert name in text, (doc, name)
        for word in ("compressed `Gt`", "endomorphism", "stream forms", "multi-GPU", "proof-file framing"):      # the "not built" list
            assert word in text, (doc, word)
    assert (ROOT / "bn_amd" / "csrc" / "sqrt_ops.hpp").exists() and (ROOT / "bn_amd" / "csrc" / "io_compress.hpp").exists()
    assert (ROOT / "tools" / "time_compress.py").exists()


def test_python_surface():
    import bn_amd
    from bn_amd import engine, groth16
    E = engine.Engine
    for g in "12":
        assert list(inspect.signature(getattr(E, f"g{g}_compress_batch")).parameters) == ["self", "p", "format"]
        assert list(inspect.signature(getattr(E, f"g{g}_decompress_batch")).parameters) == ["self", "b", "format"]
        assert list(inspect.signature(getattr(E, f"g{g}_compress_batch_dev")).parameters) == ["self", "d_p", "d_out", "n", "format", "stream"]
        assert list(inspect.signature(getattr(E, f"g{g}_decompress_batch_dev")).parameters) == ["self", "d_in", "d_out", "d_status", "n", "format", "stream"]
        assert list(inspect.signature(getattr(bn_amd, f"g{g}_compress_batch")).parameters) == ["points", "format", "engine"]
        assert list(inspect.signature(getattr(bn_amd, f"g{g}_decompress_batch")).parameters) == ["b", "format", "engine"]
        for fn in (getattr(E, f"g{g}_compress_batch"), getattr(E, f"g{g}_decompress_batch"), getattr(bn_amd, f"g{g}_compress_batch")):
            assert inspect.signature(fn).parameters["format"].default == "ark"
    assert list(inspect.signature(bn_amd.G1.to_compressed).parameters) == ["self", "format"] and list(inspect.signature(bn_amd.G2.from_compressed).parameters) == ["b", "format"]
    assert list(inspect.signature(groth16.encode_proofs).parameters) == ["proofs", "format", "engine"]
    assert list(inspect.signature(groth16.decode_proofs).parameters) == ["blob", "format", "engine"]
    assert list(inspect.signature(groth16.verify_batch_compressed).parameters) == ["vk", "blob", "public_inputs", "format", "engine", "prepared"]
    assert engine.COMPRESSED_FORMATS == {"ark": 0, "gnark": 1} == CC.FORMATS and (engine.G1_COMPRESSED_BYTES, engine.G2_COMPRESSED_BYTES) == (32, 64)
    assert issubclass(bn_amd.DecodeError, ValueError)
    src = inspect.getsource(groth16.encode_proofs)
    assert src.count("g1_compress_batch(") == 1 and src.count("g2_compress_batch(") == 1        # one G1 call over 2 m points and one G2 call
    src = inspect.getsource(groth16.decode_proofs)
    assert src.count("g1_decompress_batch(") == 1 and src.count("g2_decompress_batch(") == 1


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


class Model:
    """a stand-in engine that answers from the integer model and records what was asked"""
    def __init__(self): self.calls = []

    @staticmethod
    def _affine(g, row):
        v = [M.from_mont_limbs(row[4 * i:4 * i + 4]) for i in range(len(row) // 4)]
        return CC.affine(g, tuple(v) if g == 1 else ((v[0], v[1]), (v[2], v[3]), (v[4], v[5])))

    def _compress(self, g, p, format):
        from bn_amd.engine import compressed_format
        p = np.asarray(p, np.uint64).reshape(-1, 12 * g)
        self.calls.append((f"g{g}_compress_batch", p.shape[0], format))
        return np.stack([np.frombuffer(CC.compress(g, self._affine(g, r), compressed_format(format)), np.uint8) for r in p])

    def _decompress(self, g, b, format):
        from bn_amd.engine import compressed_format
        b = np.asarray(b, np.uint8).reshape(-1, 32 * g)
        self.calls.append((f"g{g}_decompress_batch", b.shape[0], format))
        got = [CC.decompress(g, r.tobytes(), compressed_format(format)) for r in b]
        return np.stack([CC.words(g, pt) for _, pt in got]), np.array([st for st, _ in got], np.int32)

    def g1_compress_batch(self, p, format="ark"): return self._compress(1, p, format)
    def g2_compress_batch(self, p, format="ark"): return self._compress(2, p, format)
    def g1_decompress_batch(self, b, format="ark"): return self._decompress(1, b, format)
    def g2_decompress_batch(self, b, format="ark"): return self._decompress(2, b, format)


def test_errors_raise_before_any_device_call():
    import bn_amd
    nd = NoDevice()
    from bn_amd import engine
    with pytest.raises(ValueError, match="unknown compressed format 'zcash'"):
        engine.compressed_format("zcash")
    assert [engine.compressed_format(f) for f in ("ark", "gnark", 0, 1, 7)] == [0, 1, 0, 1, 7]        # numbers pass through: the library answers for them
    with pytest.raises(ValueError, match="^33 bytes are not whole records of 32"):
        bn_amd.g1_decompress_batch(b"\0" * 33, engine=nd)
    with pytest.raises(ValueError, match="^96 bytes are not whole records of 64"):
        bn_amd.g2_decompress_batch([b"\0" * 32] * 3, engine=nd)
    with pytest.raises(ValueError, match="^130 bytes are not whole proofs of 128"):
        bn_amd.groth16.decode_proofs(b"\0" * 130, engine=nd)
    assert bn_amd.groth16.encode_proofs([], engine=nd) == b""
    proofs, status = bn_amd.groth16.decode_proofs(b"", engine=nd)
    assert proofs == [] and status.shape == (0, 3) and status.dtype == np.int32


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_python_surface_over_a_stand_in_engine(fmt, monkeypatch):
    import bn_amd
    from bn_amd import api
    m = Model()
    monkeypatch.setattr(api, "_default_engine", m)
    f = CC.FORMATS[fmt]
    for g, cls, comp, decomp in ((1, bn_amd.G1, bn_amd.g1_compress_batch, bn_amd.g1_decompress_batch), (2, bn_amd.G2, bn_amd.g2_compress_batch, bn_amd.g2_decompress_batch)):
        recs = CC.records(g, f)
        points, status = decomp(b"".join(r[1] for r in recs), fmt, engine=m)
        assert status.tolist() == [r[2] for r in recs] and status.dtype == np.int32
        assert all(isinstance(p, cls) and np.array_equal(p.limbs, CC.words(g, r[3])) for p, r in zip(points, recs))
        good = [(p, r) for p, r in zip(points, recs) if r[2] == 0]
        assert comp([p for p, _ in good], fmt, engine=m) == [r[1] for _, r in good]
        assert comp(np.stack([p.limbs for p, _ in good]), fmt, engine=m) == [r[1] for _, r in good]            # arrays are taken as well
        p, r = good[0]
        assert p.to_compressed(fmt) == r[1] and np.array_equal(cls.from_compressed(r[1], fmt).limbs, p.limbs)
        assert cls.zero().to_compressed(fmt) == CC.compress(g, None, f) and cls.from_compressed(CC.compress(g, None, f), fmt).is_zero()
        for _, b, st, _ in CC.rejected(g, f):
            with pytest.raises(bn_amd.DecodeError) as err:
                cls.from_compressed(b, fmt)
            assert err.value.status == st and api.DECODE_STATUS[st] in str(err.value)
        with pytest.raises(ValueError, match="one record is expected, got 2"):
            cls.from_compressed(r[1] * 2, fmt)
    assert {c[2] for c in m.calls} == {fmt}


@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_groth16_proofs_round_trip_over_the_stand_in_engine(fmt):
    from bn_amd import G1, G2, groth16
    m = Model()
    f = CC.FORMATS[fmt]
    g1, g2 = CC.multiples(1), CC.multiples(2)
    proofs = [(G1(CC.words(1, g1[3 * j])), G2(CC.words(2, g2[j])), G1(CC.words(1, g1[3 * j + 1]))) for j in range(4)]
    proofs.append((G1.zero(), G2.zero(), G1(CC.words(1, g1[0]))))
    blob = groth16.encode_proofs(proofs, fmt, engine=m)
    assert m.calls == [("g1_compress_batch", 10, fmt), ("g2_compress_batch", 5, fmt)]
    assert len(blob) == 128 * 5
    assert blob[:128] == CC.compress(1, g1[0], f) + CC.compress(2, g2[0], f) + CC.compress(1, g1[1], f)          # A | B | C
    m.calls.clear()
    back, status = groth16.decode_proofs(blob, fmt, engine=m)
    assert m.calls == [("g1_decompress_batch", 10, fmt), ("g2_decompress_batch", 5, fmt)]
    assert status.shape == (5, 3) and not status.any()
    assert all(np.array_equal(x.limbs, y.limbs) for p, q in zip(proofs, back) for x, y in zip(p, q))
    spoiled = bytearray(blob)
    nopoint = CC.render(1, [CC.x_without_point(1)[0]], "sign0", f)
    outside = CC.render(2, list(CC.g2_outside_subgroup()[0]), "sign0", f)
    spoiled[128:160] = nopoint; spoiled[2 * 128 + 32:2 * 128 + 96] = outside; spoiled[3 * 128 + 96:4 * 128] = CC.render(1, [1], "bad", f)
    back, status = groth16.decode_proofs(bytes(spoiled), fmt, engine=m)
    assert status.tolist() == [[0, 0, 0], [4, 0, 0], [0, 5, 0], [0, 0, 3], [0, 0, 0]]
    assert back[1][0].is_zero() and back[2][1].is_zero() and back[3][2].is_zero() and not back[1][2].is_zero()


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


@pytest.mark.parametrize("case, a, fmt, b, st, n", [
    ("format 2", DUMMY, 2, DUMMY, DUMMY, 4),
    ("format negative", DUMMY, -1, DUMMY, DUMMY, 4),
    ("format 2 without work", DUMMY, 2, DUMMY, DUMMY, 0),
    ("a NULL input", None, 0, DUMMY, DUMMY, 1),
    ("a NULL output", DUMMY, 1, None, DUMMY, 1),
    ("n above the wire format's limit", DUMMY, 0, DUMMY, DUMMY, WIRE_N_MAX + 1),
])
def test_argument_errors_answer_without_a_device(lib, case, a, fmt, b, st, n):
    for g in "12":
        got = [getattr(lib, f"bn254_g{g}_compress_batch")(None, a, fmt, b, n), getattr(lib, f"bn254_g{g}_compress_batch_dev")(None, a, fmt, b, n, None),
               getattr(lib, f"bn254_g{g}_decompress_batch")(None, a, fmt, b, st, n), getattr(lib, f"bn254_g{g}_decompress_batch_dev")(None, a, fmt, b, st, n, None)]
        assert got == [BAD_ARG] * 4, (case, g)


def test_a_null_status_is_an_error_for_decompression_only_and_no_work_is_ok(lib):
    for g in "12":
        assert getattr(lib, f"bn254_g{g}_decompress_batch")(None, DUMMY, 0, DUMMY, None, 2) == BAD_ARG
        assert getattr(lib, f"bn254_g{g}_decompress_batch_dev")(None, DUMMY, 1, DUMMY, None, 2, None) == BAD_ARG
        for fmt in (0, 1):
            assert getattr(lib, f"bn254_g{g}_compress_batch")(None, None, fmt, None, 0) == 0 and getattr(lib, f"bn254_g{g}_compress_batch_dev")(None, None, fmt, None, 0, None) == 0
            assert getattr(lib, f"bn254_g{g}_decompress_batch")(None, None, fmt, None, None, 0) == 0 and getattr(lib, f"bn254_g{g}_decompress_batch_dev")(None, None, fmt, None, None, 0, None) == 0


def test_the_hooks_check_their_bounds(lib):
    try:
        assert lib.bn254_compress_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_compress_set_launch_max(64) == 0
    finally:
        assert lib.bn254_compress_set_launch_max(0) == 0
    assert lib.bn254_compress_sqrt_window() in (0, 1)
    ops = (ROOT / "bn_amd" / "csrc" / "sqrt_ops.hpp").read_text()
    assert re.search(r"^#define BN254_SQRT_WINDOW %d\b" % lib.bn254_compress_sqrt_window(), ops, re.M)            # the default of the source is what was built


def test_the_kernels_are_instances_of_existing_names_within_their_ceilings():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    import lane_shell
    src = lane_shell.unit_source("bn254_wire.hip", own_kernels=True)                            # the unit adds no kernel under a new name
    assert set(re.findall(r"__global__[^\n]*?(bn254_\w+)\(", src)) == {"bn254_g1_encode_k", "bn254_g2_encode_k", "bn254_g1_decode_k", "bn254_g2_decode_k", "bn254_fr_encode_k", "bn254_fr_decode_k"}
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    meta = kernel_meta.instances(so)
    where = {"G1CompressOp": "bn254_fr_decode_k", "G2CompressOp": "bn254_fr_decode_k", "G1DecompressOp": "bn254_fr_decode_k", "G2DecompressOp": "bn254_g2_decode_k"}
    for op, kernel in where.items():
        mine = [n for n in meta if re.search(r"\d+" + op + r"(E|I)", n)]
        assert len(mine) == 1, (op, mine)
        assert kernel_meta.short_name(mine[0]) == kernel, mine
        assert meta[mine[0]]["spill"] <= SPILL_CEILING[kernel], (mine[0], meta[mine[0]])
        assert meta[mine[0]]["lds"] == 0, (mine[0], meta[mine[0]])
    assert (SPILL_CEILING["bn254_fr_decode_k"], SPILL_CEILING["bn254_g2_decode_k"]) == (0, 18)
