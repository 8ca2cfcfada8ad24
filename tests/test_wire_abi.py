"""The wire format (bn254_{fr,g1,g2}_{encode,decode}_batch, bn254_g{1,2}_{encode,decode}_stream) without a GPU: the ten symbols, their
declarations in every layer that mirrors the C header, and the argument checks that answer before a context or a device is looked at - every
call below passes a NULL context, so an answer of BN254_E_BAD_ARG can only come from the check of the arguments."""
import ctypes as C
import re

import pytest

import test_binding_signatures as B
import wire_cases as W

CONST, MUT = ("const",), ("mut",)
CTX, N, BYTES_IN, BYTES_OUT, ST, SIZE_OUT = ("void", MUT), ("usize", ()), ("u8", CONST), ("u8", MUT), ("i32", MUT), ("usize", MUT)
EXPECTED = {
    "bn254_fr_encode_batch": [CTX, ("fr", CONST), BYTES_OUT, N],
    "bn254_fr_decode_batch": [CTX, BYTES_IN, ("fr", MUT), ST, N],
    "bn254_g1_encode_batch": [CTX, ("g1", CONST), BYTES_OUT, N],
    "bn254_g2_encode_batch": [CTX, ("g2", CONST), BYTES_OUT, N],
    "bn254_g1_decode_batch": [CTX, BYTES_IN, ("g1", MUT), ST, N],
    "bn254_g2_decode_batch": [CTX, BYTES_IN, ("g2", MUT), ST, N],
    "bn254_g1_encode_stream": [CTX, ("g1", CONST), N, BYTES_OUT, N, SIZE_OUT],
    "bn254_g2_encode_stream": [CTX, ("g2", CONST), N, BYTES_OUT, N, SIZE_OUT],
    "bn254_g1_decode_stream": [CTX, BYTES_IN, N, ("g1", MUT), ST, N, SIZE_OUT, SIZE_OUT],
    "bn254_g2_decode_stream": [CTX, BYTES_IN, N, ("g2", MUT), ST, N, SIZE_OUT, SIZE_OUT],
}
NAMES = tuple(EXPECTED)
ENCODERS = ("bn254_fr_encode_batch", "bn254_g1_encode_batch", "bn254_g2_encode_batch")
DECODERS = ("bn254_fr_decode_batch", "bn254_g1_decode_batch", "bn254_g2_decode_batch")
BAD_ARG = -2
WIRE_N_MAX = 0x7fffffff // 129
DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    return _native.lib()


def test_the_ten_symbols_resolve():
    from bn_amd import _native
    raw = C.CDLL(str(_native.LIB_PATH))
    for name in NAMES:
        assert getattr(raw, name), name
        assert len(_native.SIGNATURES[name]) == len(EXPECTED[name]), name


def test_header_ctypes_rust_and_cpp_agree():
    from bn_amd import _native
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
        for at, (base, levels) in zip(_native.SIGNATURES[name], params):                    # the ctypes table: pointers as pointers, sizes as size_t
            assert (at is C.c_void_p or hasattr(at, "_type_")) if levels else at is C.c_size_t, name
        if name.endswith("_stream"):
            assert all(at._type_ is C.c_size_t for at, (base, levels) in zip(_native.SIGNATURES[name], params) if (base, levels) == SIZE_OUT), name
    rust = B.rust_declarations(B.RUST_LIB.read_text())
    assert set(NAMES) <= set(rust)
    assert B.compare(decls, {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    hdr = B.HEADER.read_text()
    for d, v in (("FR", 32), ("G1", W.RS[1]), ("G2", W.RS[2])):
        assert re.search(r"^#define BN254_%s_WIRE_BYTES %d\b" % (d, v), hdr, re.M), d
    # the C++ binding takes the declarations from the C header itself and has none of its own that could drift
    hpp = (B.ROOT / "include" / "bn254.hpp").read_text()
    assert '#include "bn254_hip.h"' in hpp and not re.search(r"\bint\s+bn254_\w+\s*\(", hpp)
    # what the header promises of a short `cap` is what tests/test_gpu_wire.py pins
    own = " ".join(hdr[hdr.index("/* the crate's own byte stream"):hdr.index("int bn254_g1_encode_stream(")].split())
    for word in ("BN254_E_BAD_ARG if `cap` is too small", "`*written` is left as it was", "whole records that fit", "a truncated trailing record is left unconsumed"):
        assert word in own, word


@pytest.mark.parametrize("case, a, b, st, n", [
    ("a NULL input", None, DUMMY, DUMMY, 1),
    ("a NULL output", DUMMY, None, DUMMY, 1),
    ("n above the limit", DUMMY, DUMMY, DUMMY, WIRE_N_MAX + 1),
    ("n far above the limit", DUMMY, DUMMY, DUMMY, 1 << 40),
])
def test_batch_argument_errors_answer_before_the_context(lib, case, a, b, st, n):
    for name in ENCODERS:
        assert getattr(lib, name)(None, a, b, n) == BAD_ARG, (case, name)
    for name in DECODERS:
        assert getattr(lib, name)(None, a, b, st, n) == BAD_ARG, (case, name)


def test_a_null_status_is_an_error_for_decoders_and_no_work_is_ok(lib):
    for name in DECODERS:
        assert getattr(lib, name)(None, DUMMY, DUMMY, None, 1) == BAD_ARG, name
        assert getattr(lib, name)(None, None, None, None, 0) == 0, name
    for name in ENCODERS:
        assert getattr(lib, name)(None, None, None, 0) == 0, name


@pytest.mark.parametrize("g", "12")
def test_stream_argument_errors_answer_before_the_context(lib, g):
    enc, dec = getattr(lib, f"bn254_g{g}_encode_stream"), getattr(lib, f"bn254_g{g}_decode_stream")
    w, cnt, used = C.c_size_t(77), C.c_size_t(78), C.c_size_t(79)
    assert enc(None, DUMMY, 1, DUMMY, 1000, None) == BAD_ARG                                   # NULL written
    assert enc(None, None, 0, None, 0, None) == BAD_ARG                                        # ... even without work
    assert enc(None, None, 1, DUMMY, 1000, C.byref(w)) == BAD_ARG                              # points missing
    assert enc(None, DUMMY, 1, None, 1000, C.byref(w)) == BAD_ARG                              # output missing
    assert dec(None, DUMMY, 10, DUMMY, DUMMY, 4, None, C.byref(used)) == BAD_ARG               # NULL count
    assert dec(None, DUMMY, 10, DUMMY, DUMMY, 4, C.byref(cnt), None) == BAD_ARG                # NULL consumed
    assert dec(None, None, 10, DUMMY, DUMMY, 4, C.byref(cnt), C.byref(used)) == BAD_ARG        # len > 0 with NULL in
    assert dec(None, DUMMY, 10, None, DUMMY, 4, C.byref(cnt), C.byref(used)) == BAD_ARG        # max_points > 0 with NULL out
    assert dec(None, DUMMY, 10, DUMMY, None, 4, C.byref(cnt), C.byref(used)) == BAD_ARG        # ... or NULL status
    assert (w.value, cnt.value, used.value) == (77, 78, 79)                                    # a rejected call stores nothing
    assert enc(None, None, 0, None, 0, C.byref(w)) == 0 and w.value == 0                       # no points: no bytes, and no device is needed for that
