"""Baby Jubjub and EdDSA-Poseidon (bn254_bjj_{validate,add,mul}_batch, bn254_eddsa_poseidon_{challenge,verify}_batch and their _dev twins) without a
GPU: the ten symbols and their declarations in every layer that mirrors the C header, the argument checks that answer before any device is
touched, the documented status numbers, the Python surface over a stand-in engine that answers from the integer model of babyjub_cases.py,
and the register budget of the kernels: template instances of bn254_fr_decode_k<Op> only."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import babyjub_cases as BC
import fr_cases as FC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, N, STATUS, FR_IN, FR_OUT, D_IN, D_OUT = ("void", MUT), ("usize", ()), ("i32", MUT), ("fr", CONST), ("fr", MUT), ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_bjj_validate_batch": [CTX, FR_IN, STATUS, N],
    "bn254_bjj_add_batch": [CTX, FR_IN, FR_IN, FR_OUT, N],
    "bn254_bjj_mul_batch": [CTX, FR_IN, FR_IN, FR_OUT, N],
    "bn254_eddsa_poseidon_challenge_batch": [CTX, FR_IN, FR_IN, FR_IN, FR_OUT, N],
    "bn254_eddsa_poseidon_verify_batch": [CTX, FR_IN, FR_IN, FR_IN, FR_IN, STATUS, N],
    "bn254_bjj_validate_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_bjj_add_batch_dev": [CTX, D_IN, D_IN, D_OUT, N, D_OUT],
    "bn254_bjj_mul_batch_dev": [CTX, D_IN, D_IN, D_OUT, N, D_OUT],
    "bn254_eddsa_poseidon_challenge_batch_dev": [CTX, D_IN, D_IN, D_IN, D_OUT, N, D_OUT],
    "bn254_eddsa_poseidon_verify_batch_dev": [CTX, D_IN, D_IN, D_IN, D_IN, D_OUT, N, D_OUT],
}
NAMES = tuple(EXPECTED)
HOST = NAMES[:5]
HOOKS = ("bn254_bjj_set_launch_max", "bn254_eddsa_window")
SCOPES = ("bjj_validate", "bjj_add", "bjj_mul", "eddsa_poseidon_challenge", "eddsa_poseidon_verify")
OPS = ("BjjValidateOp", "BjjAddOp", "BjjMulOp", "EddsaChallengeOp", "EddsaVerifyOp")
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_bjj_set_launch_max.argtypes = [C.c_size_t]
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
    assert any(s.name == "bn254_babyjub.hip" for s in _native.SOURCES)
    assert raw.bn254_eddsa_window() in (1, 2)


def test_header_declares_the_ten_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert hdr.index("int bn254_g2_validate_batch_dev(") < hdr.index("/* Baby Jubjub and EdDSA-Poseidon") < hdr.index("int bn254_bjj_validate_batch(") < hdr.index("/* ---- device-resident entry points")
    own = " ".join(hdr[hdr.index("/* Baby Jubjub and EdDSA-Poseidon"):hdr.index("int bn254_bjj_validate_batch(")].split())
    for word in ("a = 168700 and d = 168696", str(BC.L), str(BC.B8[0]), str(BC.B8[1]), "O = (0, 1)", "-(x, y) = (-x, y)", "complete", "two consecutive bn_fr, x then y",
                 "as they stand, before any field arithmetic", "[l]P != O", "O is one", "out may be p or q", "cofactor components included", "out may be p.",
                 "Poseidon5(r8[i].x, r8[i].y, a[i].x, a[i].y, msg[i])", "R_F = 8, R_P = 60", "NO curve check", "the integer of s is not below l", "R8 or A is not on the curve",
                 "[S]B8 != R8 + [8 hm]A", "INTEGER 8 hm", "NO subgroup check", "A = O", "n > 2^40", "BN254_E_BAD_ARG", "n == 0 succeeds", "at most 2^22 records", "d_status too",
                 "read nothing back"):
        assert word in own, word
    assert [int(x) for x in re.findall(r"(?:^| )(\d) (?=a coordinate is|a x\^2|on the curve but|otherwise: a valid|a word array|R8 or A is|\[S\]B8 !=|valid There)", own)] == [1, 4, 5, 0, 1, 4, 6, 0]
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for text in (semantics, threading):
        for name in NAMES:
            assert name in text, name
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"bjj_validate"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)                   # a line of its own
    src = (ROOT / "bn_amd" / "csrc" / "bn254_babyjub.hip").read_text()
    assert set(SCOPES) <= set(re.findall(r'"(\w+)"', src))


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn bjj_validate_batch(p: &[Fr]) -> Result<Vec<i32>, GpuError>", "pub fn bjj_add_batch(p: &[Fr], q: &[Fr]) -> Result<Vec<Fr>, GpuError>",
               "pub fn bjj_mul_batch(p: &[Fr], k: &[Fr]) -> Result<Vec<Fr>, GpuError>", "pub fn eddsa_poseidon_challenge_batch(a: &[Fr], r8: &[Fr], msg: &[Fr]) -> Result<Vec<Fr>, GpuError>",
               "pub fn eddsa_poseidon_verify_batch(a: &[Fr], r8: &[Fr], s: &[Fr], msg: &[Fr]) -> Result<Vec<i32>, GpuError>"):
        assert fn in txt, fn
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<int32_t> bjj_validate(", "std::vector<Fr> bjj_add(", "std::vector<Fr> bjj_mul(", "std::vector<Fr> eddsa_poseidon_challenge(", "std::vector<int32_t> eddsa_poseidon_verify(") + HOST:
        assert s + ("(" if s.startswith("bn254_") else "") in hpp, s
    variant = (ROOT / "tools" / "build_variant.sh").read_text()
    assert re.search(r"^for u in .*\bbn254_babyjub\b.*; do$", variant, re.M) and "-DBN254_EDDSA_WINDOW=1" in variant and "-DBN254_EDDSA_WINDOW=2" in variant
    ops = (ROOT / "bn_amd" / "csrc" / "babyjub_ops.hpp").read_text()
    assert re.search(r"^#ifndef BN254_EDDSA_WINDOW\n#define BN254_EDDSA_WINDOW [12]\b", ops, re.M)
    for doc in ("README.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        for name in HOST + ("Baby Jubjub", "EdDSA-Poseidon", "BLAKE-512"):
            assert name in text, (doc, name)
    readme = (ROOT / "README.md").read_text()
    assert "profiles/r25_babyjub.txt" in readme and "No speed is promised" in readme and (ROOT / "tools" / "time_babyjub.py").exists()


def test_python_surface():
    import bn_amd
    from bn_amd import babyjub, eddsa, engine
    E = engine.Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.bjj_validate_batch) == ["self", "p"] and sig(E.bjj_add_batch) == ["self", "p", "q"] and sig(E.bjj_mul_batch) == ["self", "p", "k"]
    assert sig(E.eddsa_poseidon_challenge_batch) == ["self", "a", "r8", "msg"] and sig(E.eddsa_poseidon_verify_batch) == ["self", "a", "r8", "s", "msg"]
    assert sig(E.bjj_validate_batch_dev) == ["self", "d_p", "d_status", "n", "stream"] and sig(E.bjj_mul_batch_dev) == ["self", "d_p", "d_k", "d_out", "n", "stream"]
    assert sig(E.bjj_add_batch_dev) == ["self", "d_p", "d_q", "d_out", "n", "stream"]
    assert sig(E.eddsa_poseidon_challenge_batch_dev) == ["self", "d_a", "d_r8", "d_msg", "d_out", "n", "stream"]
    assert sig(E.eddsa_poseidon_verify_batch_dev) == ["self", "d_a", "d_r8", "d_s", "d_msg", "d_status", "n", "stream"]
    for name in ("bjj_validate_batch", "bjj_add_batch", "bjj_mul_batch", "eddsa_poseidon_challenge_batch", "eddsa_poseidon_verify_batch"):
        assert getattr(bn_amd, name) is getattr(bn_amd.api, name) and "engine" in sig(getattr(bn_amd, name))
    for name in ("add_host", "mul_host", "on_curve_host", "Point", "mul_base", "A", "D", "L", "G", "B8"):
        assert hasattr(babyjub, name), name
    for name in ("public_keys", "sign", "sign_batch", "verify", "verify_batch", "verify_status_batch", "verify_host"):
        assert hasattr(eddsa, name), name
    assert inspect.signature(eddsa.sign).parameters["nonce"].default is None and "NOT circomlib's" in eddsa.__doc__
    assert bn_amd.poseidon.ARITY_MAX == 4 and engine.POSEIDON_ARITY_MAX == 4                     # the public Poseidon calls did not grow


# ------------------------------------------------------------------------------------------------------------------ a stand-in engine
class Model:
    """the five calls answered from the integer model; counts them"""
    def __init__(self):
        self.calls = []

    @staticmethod
    def _ints(a):
        a = np.asarray(a, np.uint64).reshape(-1, 4)
        inv = pow(FC.MONT, -1, BC.R)
        raw = [sum(int(x) << (64 * i) for i, x in enumerate(r)) for r in a]
        return [v * inv % BC.R if v < BC.R else v for v in raw]                  # words that are not below r stay what they are

    def _pts(self, p):
        v = self._ints(p)
        return list(zip(v[0::2], v[1::2]))

    def bjj_validate_batch(self, p):
        self.calls.append(("bjj_validate_batch", len(p)))
        return np.array([BC.validate_status(*q) for q in self._pts(p)], np.int32)

    def bjj_add_batch(self, p, q):
        self.calls.append(("bjj_add_batch", len(p)))
        return BC.point_rows([BC.add(a, b) for a, b in zip(self._pts(p), self._pts(q))])

    def bjj_mul_batch(self, p, k):
        self.calls.append(("bjj_mul_batch", len(p)))
        return BC.point_rows([BC.mul(a, b) for a, b in zip(self._pts(p), self._ints(k))])

    def eddsa_poseidon_challenge_batch(self, a, r8, msg):
        self.calls.append(("eddsa_poseidon_challenge_batch", len(msg)))
        return FC.rows([BC.challenge(x, y, m) for x, y, m in zip(self._pts(a), self._pts(r8), self._ints(msg))])

    def eddsa_poseidon_verify_batch(self, a, r8, s, msg):
        self.calls.append(("eddsa_poseidon_verify_batch", len(msg)))
        return np.array([BC.verify_status(x, y, k, m) for x, y, k, m in zip(self._pts(a), self._pts(r8), self._ints(s), self._ints(msg))], np.int32)


def test_the_package_over_the_model_makes_the_calls_it_promises():
    import bn_amd
    from bn_amd import Fr, babyjub as BJ, eddsa
    m = Model()
    assert BJ.mul_base([Fr(3), Fr(0)], engine=m) == [BJ.Point(*BC.mul(BC.B8, 3)), BJ.Point.identity()] and m.calls == [("bjj_mul_batch", 2)]
    m.calls.clear()
    secrets, msgs = [7, 11, BC.L - 2], [0, BC.R - 1, 5]
    pks = eddsa.public_keys(secrets, engine=m)
    assert m.calls == [("bjj_mul_batch", 3)] and pks == [BJ.Point(*BC.mul(BC.B8, s)) for s in secrets]
    m.calls.clear()
    sigs = eddsa.sign_batch(secrets, msgs, engine=m)
    assert m.calls == [("bjj_mul_batch", 6), ("eddsa_poseidon_challenge_batch", 3)]                 # keys and nonces share the one multiplication call
    m.calls.clear()
    assert eddsa.verify_batch(pks, msgs, sigs, engine=m) == [True] * 3 and m.calls == [("eddsa_poseidon_verify_batch", 3)]
    assert [eddsa.verify_host(p, mm, s) for p, mm, s in zip(pks, msgs, sigs)] == [True] * 3
    assert eddsa.sign(7, 5, nonce=99, engine=m) == (BJ.Point(*BC.sign(7, 5, 99)[1]), BC.sign(7, 5, 99)[2])
    assert eddsa.default_nonce(7, 5) == eddsa.default_nonce(7, 5) != eddsa.default_nonce(7, 6) and 0 <= eddsa.default_nonce(7, 5) < BC.L
    assert eddsa.verify_status_batch(pks, msgs, [(sigs[0][0], sigs[0][1] + BC.L), sigs[0], sigs[2]], engine=m).tolist() == [1, 6, 0]
    assert eddsa.sign_batch([], [], engine=m) == []
    with pytest.raises(ValueError):
        eddsa.sign_batch([1], [1, 2], engine=m)
    with pytest.raises(ValueError):
        bn_amd.bjj_mul_batch([BC.B8], [Fr(1), Fr(2)], engine=m)
    assert bn_amd.bjj_validate_batch(BC.point_rows([BC.B8, (BC.R, 1)]), engine=m).tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


def test_argument_errors_answer_without_a_device(lib):
    for name in HOST:
        f, fd = getattr(lib, name), getattr(lib, name + "_dev")
        k = len(EXPECTED[name]) - 2                                  # pointer arguments behind ctx
        for null in range(k):
            args = [None if j == null else DUMMY for j in range(k)]
            assert f(None, *args, 1) == BAD_ARG, (name, null)
            assert fd(None, *args, 1, None) == BAD_ARG, (name, null)
        assert f(None, *[DUMMY] * k, (1 << 40) + 1) == BAD_ARG and fd(None, *[DUMMY] * k, (1 << 40) + 1, None) == BAD_ARG, name


def test_no_work_is_ok(lib):
    for name in HOST:
        k = len(EXPECTED[name]) - 2
        assert getattr(lib, name)(None, *[None] * k, 0) == 0 and getattr(lib, name + "_dev")(None, *[None] * k, 0, None) == 0, name


def test_the_hook_checks_its_bounds(lib):
    try:
        assert lib.bn254_bjj_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_bjj_set_launch_max(64) == 0
    finally:
        assert lib.bn254_bjj_set_launch_max(0) == 0


def test_the_status_numbers_are_as_documented():
    from bn_amd import babyjub
    assert (BC.ST_OK, BC.ST_RANGE, BC.ST_CURVE, BC.ST_ORDER, BC.ST_EQUATION) == (0, 1, 4, 5, 6) and set(babyjub.STATUS) == {0, 1, 4, 5, 6}
    ops = (ROOT / "bn_amd" / "csrc" / "babyjub_ops.hpp").read_text()
    assert "status[i] = !in_range ? 1 : !on_curve ? 4 : !bjj_is_identity(lp) ? 5 : 0;" in ops and "status[i] = !in_range ? 1 : !on_curve ? 4 : !eq ? 6 : 0;" in ops
    wire = (ROOT / "bn_amd" / "csrc" / "io_wire.hpp").read_text()
    taken = {int(x) for x in re.findall(r"WIRE_\w+ = (\d+)", wire)}
    assert 6 not in taken and {1, 4, 5} <= taken, taken                                          # 6 is a new number; 1, 4, 5 keep their meaning


def test_the_kernels_are_instances_of_bn254_fr_decode_k_without_spill_or_lds():
    import isa_mix
    import kernel_meta
    import lane_shell
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    src = lane_shell.unit_source("bn254_babyjub.hip")    # the unit adds no kernel under a new name: the shell is lane_launch.hpp's
    assert "__global__" not in src
    for text in (src, (ROOT / "bn_amd" / "csrc" / "babyjub_ops.hpp").read_text()):
        assert "__shared__" not in text and "atomic" not in text.lower()
    assert so.exists() and (isa_mix.LLVM / "llvm-readelf").exists()
    meta = kernel_meta.instances(so)
    for op in OPS:
        mine = [n for n in meta if re.search(r"\d+" + op + r"(E|I)", n)]
        assert len(mine) == 1, (op, mine)
        assert kernel_meta.short_name(mine[0]) == "bn254_fr_decode_k", mine
        assert meta[mine[0]]["spill"] == 0 == SPILL_CEILING["bn254_fr_decode_k"], (mine[0], meta[mine[0]])
        assert meta[mine[0]]["lds"] == 0, (mine[0], meta[mine[0]])
