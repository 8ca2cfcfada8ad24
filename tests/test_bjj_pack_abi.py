"""The square root in Fr, Baby Jubjub point packing and the packed EdDSA-Poseidon verifier (bn254_fr_sqrt_batch, bn254_bjj_{pack,unpack}_batch,
bn254_eddsa_poseidon_verify_packed_batch and their _dev twins) without a GPU: the eight symbols and their declarations in every layer that
mirrors the C header, the argument checks that answer before any device is touched, the Python surface over a stand-in engine that answers
from the integer model of bjj_pack_cases.py, and the register budget of the kernels: template instances of bn254_fr_decode_k<Op> only, the
unpacked verifier's instance unchanged."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import babyjub_cases as BC
import bjj_pack_cases as PK
import fr_cases as FC
import test_binding_signatures as B
from test_babyjub_abi import Model as AffineModel

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, N, STATUS, FR_IN, FR_OUT, U8_IN, U8_OUT, D_IN, D_OUT = ("void", MUT), ("usize", ()), ("i32", MUT), ("fr", CONST), ("fr", MUT), ("u8", CONST), ("u8", MUT), ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_fr_sqrt_batch": [CTX, FR_IN, FR_OUT, STATUS, N],
    "bn254_bjj_pack_batch": [CTX, FR_IN, U8_OUT, N],
    "bn254_bjj_unpack_batch": [CTX, U8_IN, FR_OUT, STATUS, N],
    "bn254_eddsa_poseidon_verify_packed_batch": [CTX, U8_IN, U8_IN, FR_IN, STATUS, N],
    "bn254_fr_sqrt_batch_dev": [CTX, D_IN, D_OUT, D_OUT, N, D_OUT],
    "bn254_bjj_pack_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_bjj_unpack_batch_dev": [CTX, D_IN, D_OUT, D_OUT, N, D_OUT],
    "bn254_eddsa_poseidon_verify_packed_batch_dev": [CTX, D_IN, D_IN, D_IN, D_OUT, N, D_OUT],
}
NAMES = tuple(EXPECTED)
HOST = NAMES[:4]
OPTIONAL = {"bn254_fr_sqrt_batch": {2}}                       # pointer arguments (behind ctx) that may be NULL: ok
HOOKS = ("bn254_fr_sqrt_form", "bn254_fr_set_sqrt_form", "bn254_bjj_set_sqrt_form", "bn254_bjj_set_launch_max", "bn254_fr_set_launch_max")
SCOPES = ("fr_sqrt", "bjj_pack", "bjj_unpack", "eddsa_poseidon_verify_packed")
OPS = {"FrSqrtOp": 2, "BjjPackOp": 1, "BjjUnpackOp": 2, "EddsaVerifyPackedOp": 1}         # instances: both forms of the root where a hook picks one
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_bjj_set_sqrt_form.argtypes = [C.c_int]
    l.bn254_fr_set_sqrt_form.argtypes = [C.c_int]
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
    assert raw.bn254_fr_sqrt_form() in (0, 1)
    assert any(s.name == "bn254_fr_sqrt.hip" for s in _native.SOURCES)


def test_header_declares_the_eight_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert hdr.index("int bn254_fr_inverse_batch(") < hdr.index("int bn254_fr_sqrt_batch(") < hdr.index("int bn254_fr_ntt_batch(")          # with the other fr calls
    assert hdr.index("int bn254_eddsa_poseidon_verify_batch_dev(") < hdr.index("/* Packed points and signatures") < hdr.index("int bn254_bjj_pack_batch(") < hdr.index("/* ---- device-resident entry points")
    own = " ".join(hdr[hdr.index("/* Packed points and signatures"):hdr.index("int bn254_bjj_pack_batch(")].split())
    for word in ("little endian", "bit 7 of byte 31", "above (r - 1) / 2", "its top bit is no flag", "unspecified bytes, never a fault", "no point has this y",
                 "non-canonical encoding of (0, 1) or (0, -1)", "A rejected record gives O = (0, 1)", "NO subgroup check", "bn254_bjj_validate_batch", "no inversion",
                 "the integer S is not below l", "a point has no x", "a non-canonical sign, in either point", "[S]B8 != R8 + [8 hm]A", "One launch", "n > 2^40", "BN254_E_BAD_ARG",
                 "n == 0 succeeds", "at most 2^22 records", "read nothing back"):
        assert word in own, word
    assert [int(x) for x in re.findall(r"(?:^| )(\d) (?=the integer of y|x\^2 =|x == 0 and|otherwise: out|a y is not|a point has no|a non-canonical sign|\[S\]B8 !=|valid One)", own)] == [1, 4, 3, 0, 1, 4, 3, 6, 0]
    sq = " ".join(hdr[hdr.index("/* Option<Fr> square roots"):hdr.index("int bn254_fr_sqrt_batch(")].split())
    for word in ("not above (r - 1) / 2", "ok may be NULL and out may be a", "r - 1 = 2^28 t", "0 has the root 0", "same instruction stream"):
        assert word in sq, word
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for text in (semantics, threading):
        for name in NAMES:
            assert name in text, name
    for hook in HOOKS:                                                                          # the hooks are internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"bjj_unpack"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)                   # a line of its own
    src = (ROOT / "bn_amd" / "csrc" / "bn254_babyjub.hip").read_text() + (ROOT / "bn_amd" / "csrc" / "bn254_fr_sqrt.hip").read_text()
    assert set(SCOPES) <= set(re.findall(r'"(\w+)"', src))


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn fr_sqrt(a: &[Fr]) -> Result<Vec<Option<Fr>>, GpuError>", "pub fn bjj_pack_batch(p: &[Fr]) -> Result<Vec<u8>, GpuError>",
               "pub fn bjj_unpack_batch(in32: &[u8]) -> Result<(Vec<Fr>, Vec<i32>), GpuError>",
               "pub fn eddsa_poseidon_verify_packed_batch(a32: &[u8], sig64: &[u8], msg: &[Fr]) -> Result<Vec<i32>, GpuError>"):
        assert fn in txt, fn
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<bool>> fr_sqrt(", "std::vector<uint8_t> bjj_pack(", "std::vector<int32_t>> bjj_unpack(", "std::vector<int32_t> eddsa_poseidon_verify_packed(") + HOST:
        assert s + ("(" if s.startswith("bn254_") else "") in hpp, s
    variant = (ROOT / "tools" / "build_variant.sh").read_text()
    assert re.search(r"^for u in .*\bbn254_fr_sqrt\b.*; do$", variant, re.M) and "-DBN254_FR_SQRT_FORM=0" in variant and "-DBN254_FR_SQRT_FORM=1" in variant
    ops = (ROOT / "bn_amd" / "csrc" / "fr_sqrt_ops.hpp").read_text()
    assert re.search(r"^#ifndef BN254_FR_SQRT_FORM\n#define BN254_FR_SQRT_FORM [01]\b", ops, re.M)
    for doc in ("README.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        for name in HOST + ("packPoint", "Pedersen"):
            assert name in text, (doc, name)
    readme = (ROOT / "README.md").read_text()
    assert "profiles/r26_bjj_pack.txt" in readme and "built since, below" in readme and (ROOT / "tools" / "time_bjj_pack.py").exists()


def test_python_surface():
    import bn_amd
    from bn_amd import babyjub, eddsa, engine
    E = engine.Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.fr_sqrt_batch) == ["self", "a"] and sig(E.bjj_pack_batch) == ["self", "p"] and sig(E.bjj_unpack_batch) == ["self", "in32"]
    assert sig(E.eddsa_poseidon_verify_packed_batch) == ["self", "a32", "sig64", "msg"]
    assert sig(E.fr_sqrt_batch_dev) == ["self", "d_a", "d_out", "d_ok", "n", "stream"] and sig(E.bjj_pack_batch_dev) == ["self", "d_p", "d_out32", "n", "stream"]
    assert sig(E.bjj_unpack_batch_dev) == ["self", "d_in32", "d_out", "d_status", "n", "stream"]
    assert sig(E.eddsa_poseidon_verify_packed_batch_dev) == ["self", "d_a32", "d_sig64", "d_msg", "d_status", "n", "stream"]
    for name in ("fr_sqrt_batch", "bjj_pack_batch", "bjj_unpack_batch", "eddsa_poseidon_verify_packed_batch"):
        assert getattr(bn_amd, name) is getattr(bn_amd.api, name) and "engine" in sig(getattr(bn_amd, name))
    assert callable(bn_amd.Fr.sqrt) and callable(babyjub.Point.pack) and callable(babyjub.Point.unpack)
    for name in ("pack_batch", "unpack_batch", "pack_host", "unpack_host", "sqrt_host", "PACK_STATUS"):
        assert hasattr(babyjub, name), name
    for name in ("pack_signature", "unpack_signature", "verify_packed_status_batch", "verify_packed_batch", "verify_packed", "verify_packed_status_host"):
        assert hasattr(eddsa, name), name
    assert inspect.signature(eddsa.sign_batch).parameters["packed"].default is False
    assert babyjub.PACK_STATUS[3] and "NO packed test vector" in babyjub.__doc__ and "NO packed vector" in eddsa.__doc__ and "may differ from circomlibjs" in babyjub.__doc__


# ------------------------------------------------------------------------------------------------------------------ a stand-in engine
class Model(AffineModel):
    """the new calls answered from the integer model, beside the five of test_babyjub_abi.py"""
    def fr_sqrt_batch(self, a):
        self.calls.append(("fr_sqrt_batch", len(a)))
        out, ok = PK.model_sqrt(self._ints(a))
        return out, ok != 0

    def bjj_pack_batch(self, p):
        self.calls.append(("bjj_pack_batch", len(p)))
        return PK.byte_rows([PK.pack(q) for q in self._pts(p)])

    def bjj_unpack_batch(self, in32):
        self.calls.append(("bjj_unpack_batch", len(in32)))
        got = [PK.unpack(r.tobytes()) for r in np.asarray(in32, np.uint8).reshape(-1, 32)]
        return BC.point_rows([p for p, _ in got]).reshape(-1, 2, 4), np.array([st for _, st in got], np.int32)

    def eddsa_poseidon_verify_packed_batch(self, a32, sig64, msg):
        self.calls.append(("eddsa_poseidon_verify_packed_batch", len(msg)))
        return np.array([PK.verify_packed_status(a.tobytes(), s.tobytes(), m) for a, s, m in zip(a32, sig64, self._ints(msg))], np.int32)


def test_the_package_over_the_model_makes_the_calls_it_promises():
    import bn_amd
    from bn_amd import Fr, babyjub as BJ, eddsa
    m = Model()
    assert bn_amd.fr_sqrt_batch([Fr(4), Fr(5), Fr(0)], engine=m) == [Fr(2), None, Fr(0)] and m.calls == [("fr_sqrt_batch", 3)]
    m.calls.clear()
    pts = [BJ.Point(*BC.G), BJ.Point(*BC.neg(BC.G)), BJ.Point.identity()]
    recs = BJ.pack_batch(pts, engine=m)
    assert recs == [BJ.pack_host(p) for p in pts] and recs[0][:31] == recs[1][:31] and recs[0][31] ^ recs[1][31] == 0x80
    got, st = BJ.unpack_batch(recs + [b"\xff" * 32], engine=m)
    assert got == pts + [BJ.Point.identity()] and st.tolist() == [0, 0, 0, 1] and m.calls == [("bjj_pack_batch", 3), ("bjj_unpack_batch", 4)]
    m.calls.clear()
    secrets, msgs = [7, 11, BC.L - 2], [0, BC.R - 1, 5]
    sigs = eddsa.sign_batch(secrets, msgs, engine=m, packed=True)
    assert m.calls == [("bjj_mul_batch", 6), ("eddsa_poseidon_challenge_batch", 3), ("bjj_pack_batch", 3)] and all(len(s) == 64 for s in sigs)
    pks = BJ.pack_batch(eddsa.public_keys(secrets, engine=m), engine=m)
    m.calls.clear()
    assert eddsa.verify_packed_batch(pks, msgs, sigs, engine=m) == [True] * 3 and m.calls == [("eddsa_poseidon_verify_packed_batch", 3)]      # one call on the wire bytes
    assert [eddsa.verify_packed_status_host(p, mm, s) for p, mm, s in zip(pks, msgs, sigs)] == [0] * 3
    assert eddsa.verify_packed_status_batch(pks, msgs, [sigs[1], sigs[1], sigs[2]], engine=m).tolist() == [6, 0, 0]
    with pytest.raises(ValueError):
        eddsa.verify_packed_status_batch(pks, msgs[:2], sigs, engine=m)
    with pytest.raises(ValueError):
        BJ.unpack_batch([b"\x00" * 31], engine=m)


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


def test_argument_errors_answer_without_a_device(lib):
    for name in HOST:
        f, fd = getattr(lib, name), getattr(lib, name + "_dev")
        k = len(EXPECTED[name]) - 2                                  # pointer arguments behind ctx
        for null in set(range(k)) - OPTIONAL.get(name, set()):
            args = [None if j == null else DUMMY for j in range(k)]
            assert f(None, *args, 1) == BAD_ARG, (name, null)
            assert fd(None, *args, 1, None) == BAD_ARG, (name, null)
        assert f(None, *[DUMMY] * k, (1 << 40) + 1) == BAD_ARG and fd(None, *[DUMMY] * k, (1 << 40) + 1, None) == BAD_ARG, name


def test_no_work_is_ok(lib):
    for name in HOST:
        k = len(EXPECTED[name]) - 2
        assert getattr(lib, name)(None, *[None] * k, 0) == 0 and getattr(lib, name + "_dev")(None, *[None] * k, 0, None) == 0, name


def test_the_hooks_check_their_bounds(lib):
    try:
        for f in (lib.bn254_bjj_set_sqrt_form, lib.bn254_fr_set_sqrt_form):
            assert f(2) == BAD_ARG and f(-2) == BAD_ARG and f(0) == 0 and f(1) == 0
    finally:
        assert lib.bn254_bjj_set_sqrt_form(-1) == 0 and lib.bn254_fr_set_sqrt_form(-1) == 0


def test_the_status_numbers_are_as_documented():
    assert (PK.ST_OK, PK.ST_RANGE, PK.ST_SIGN, PK.ST_NO_POINT, PK.ST_EQUATION) == (0, 1, 3, 4, 6)
    ops = (ROOT / "bn_amd" / "csrc" / "babyjub_ops.hpp").read_text()
    assert "status[i] = !u.in_range ? 1 : !u.has_x ? 4 : !u.canonical ? 3 : 0;" in ops
    assert "status[i] = !in_range ? 1 : !has_x ? 4 : !canonical ? 3 : !eq ? 6 : 0;" in ops


def test_the_kernels_are_instances_of_bn254_fr_decode_k_without_spill_or_lds():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    for f in ("fr_sqrt_ops.hpp", "babyjub_ops.hpp"):
        text = (ROOT / "bn_amd" / "csrc" / f).read_text()
        assert "__shared__" not in text and "atomic" not in text.lower() and "__global__" not in text
    assert so.exists() and (isa_mix.LLVM / "llvm-readelf").exists()
    meta = kernel_meta.instances(so)
    for op, count in OPS.items():
        mine = [n for n in meta if re.search(r"\d+" + op + r"(E|I)", n)]
        assert len(mine) == count, (op, mine)
        for name in mine:
            assert kernel_meta.short_name(name) == "bn254_fr_decode_k", name
            assert meta[name]["spill"] == 0 == SPILL_CEILING["bn254_fr_decode_k"], (name, meta[name])
            assert meta[name]["lds"] == 0, (name, meta[name])
    old = [n for n in meta if re.search(r"\d+EddsaVerifyOp(E|I)", n)]
    assert len(old) == 1 and meta[old[0]]["spill"] == 0 and meta[old[0]]["vgpr"] <= 258, meta[old[0]]       # the unpacked verifier's instance did not grow
