"""Point validation (bn254_g1_validate_batch, bn254_g2_validate_batch and their _dev twins) without a GPU: the four symbols and their declarations
in every layer that mirrors the C header, the argument checks that answer before any device is touched, the Python surface, bn_amd.api and
bls*.verify_batch(validate=...) over a stand-in engine that answers from the integer model of subgroup_cases.py - the numbers of engine calls they
promise - and the register budget of the kernels: template instances of bn254_fr_decode_k<Op> only."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import bn_model as M
import hash_g2_cases as HC
import subgroup_cases as S
import test_binding_signatures as B
import test_hash_abi as G1T
import test_hash_g2_abi as G2T

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, N, STATUS, D_IN, D_OUT = ("void", MUT), ("usize", ()), ("i32", MUT), ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_g1_validate_batch": [CTX, ("g1", CONST), STATUS, N],
    "bn254_g2_validate_batch": [CTX, ("g2", CONST), STATUS, N],
    "bn254_g1_validate_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_g2_validate_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
}
NAMES = tuple(EXPECTED)
HOOKS = ("bn254_validate_set_launch_max",)
SCOPES = ("g1_validate", "g2_validate")
OPS = ("G1ValidateOp", "G2ValidateOp")
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_validate_set_launch_max.argtypes = [C.c_size_t]
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
    assert any(s.name == "bn254_validate.hip" for s in _native.SOURCES)


def test_header_declares_the_four_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert hdr.index("bn254_g2_hash_to_curve_batch_dev(bn254_ctx") < hdr.index("/* Validation of raw points") < hdr.index("int bn254_g1_validate_batch(") < hdr.index("/* ---- device-resident entry points")
    own = " ".join(hdr[hdr.index("/* Validation of raw points"):hdr.index("int bn254_g1_validate_batch(")].split())
    for word in ("any z", "as they stand, before any field arithmetic", "z == 0: the point at infinity, whatever x and y hold", "Y^2 != X^3 + b Z^6", "(G2 only)",
                 "2q - r", "cofactor 1", "[u + 1]P + psi([u]P) + psi^2([u]P) == psi^3([2u]P)", "4965661367192848881", "gnark-crypto", "if and only if [r]P == 0",
                 "never the GLS multiplication", "bn254_g2_mul_batch by r is WRONG", "a record is never changed", "n > 2^40", "BN254_E_BAD_ARG", "n == 0 succeeds",
                 "at most 2^22 records", "d_status too"):
        assert word in own, word
    assert [int(x) for x in re.findall(r"(?:^| )(\d) (?=a coordinate|z == 0|Y\^2|\(G2 only\)|otherwise)", own)] == [1, 0, 4, 5, 0]       # the order of the checks
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for text in (semantics, threading):
        for name in NAMES:
            assert name in text, name
    for hook in HOOKS:                                                                          # the test hook is internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"g1_validate"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)                   # a line of its own
    src = (ROOT / "bn_amd" / "csrc" / "bn254_validate.hip").read_text()
    assert set(SCOPES) <= set(re.findall(r'"(\w+)"', src))


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn g1_validate_batch(p: &[G1]) -> Result<Vec<i32>, GpuError>", "pub fn g2_validate_batch(p: &[G2]) -> Result<Vec<i32>, GpuError>"):
        assert fn in txt, fn
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<int32_t> g1_validate(", "std::vector<int32_t> g2_validate(", "bn254_g1_validate_batch(", "bn254_g2_validate_batch("):
        assert s in hpp, s
    variant = (ROOT / "tools" / "build_variant.sh").read_text()
    assert re.search(r"^for u in .*\bbn254_validate\b.*; do$", variant, re.M) and "-DBN254_G2_SUBGROUP_ENDO=0" in variant
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        for name in NAMES[:2] + ("endomorphism subgroup test", "BN254_G2_SUBGROUP_ENDO", "validate=True"):
            assert name in text, (doc, name)
    readme = (ROOT / "README.md").read_text()
    assert "profiles/r24_validate.txt" in readme and (ROOT / "tools" / "time_validate.py").exists()


def test_the_decoders_switch_and_the_shared_chain():
    csrc = ROOT / "bn_amd" / "csrc"
    wire = (csrc / "io_wire.hpp").read_text()
    assert re.search(r"^#ifndef BN254_G2_SUBGROUP_ENDO\n#define BN254_G2_SUBGROUP_ENDO [01]\b", wire, re.M)
    assert "g2_in_subgroup_chain(" in wire and "g2_in_subgroup_endo(" in wire and "#if BN254_G2_SUBGROUP_ENDO" in wire
    ops = (csrc / "subgroup_ops.hpp").read_text()
    body = ops.split("#pragma once")[1]
    for s in ("BN_OUTER bool g2_in_subgroup_endo(const H2cJac2 &p)", "h2c_mul_u(p)", "h2c_psi(", "h2c_psi2(", "h2c_psi3(", "add_body<H2cF2>", "k::BN_U", "words_lt_q("):
        assert s in body, s
    assert "scalar_mul_gls(" not in body and "jac_add_flags(acc, p, false, false)" not in body   # never GLS, never an addition that assumes its operands differ
    g2 = (csrc / "hash_g2_ops.hpp").read_text()
    assert '#include "subgroup_ops.hpp"' in g2 and "BN_FN H2cJac2 h2c_mul_u(" not in g2 and "BN_FN H2cJac2 h2c_mul_u(" in ops                  # one copy of the chain
    import math
    assert S.N % S.R == 0 and math.gcd(S.N, S.COFACTOR) == 1 and S.COFACTOR == 2 * M.Q - M.R_ORD                                               # what the header's "if and only if" rests on


def test_python_surface():
    import bn_amd
    from bn_amd import bls, bls_minpk, engine
    E = engine.Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.g1_validate_batch) == ["self", "p"] and sig(E.g2_validate_batch) == ["self", "p"]
    assert sig(E.g1_validate_batch_dev) == ["self", "d_p", "d_status", "n", "stream"] and sig(E.g2_validate_batch_dev) == ["self", "d_p", "d_status", "n", "stream"]
    assert sig(bn_amd.g1_validate_batch) == ["points", "engine"] and sig(bn_amd.g2_validate_batch) == ["points", "engine"]
    assert sig(bn_amd.G1.is_valid) == ["self"] and sig(bn_amd.G2.is_valid) == ["self"]
    for mod in (bls, bls_minpk):
        p = inspect.signature(mod.verify_batch).parameters
        assert list(p)[:4] == ["pks", "msgs", "sigs", "dst"] and p["validate"].default is False and p["engine"].default is None


# ------------------------------------------------------------------------------------------------------------------ a stand-in engine
class _Validating:
    """the two validation calls answered from the integer model"""
    def g1_validate_batch(self, p):
        p = np.asarray(p, np.uint64).reshape(-1, 12)
        self.calls.append(("g1_validate_batch", p.shape[0]))
        return np.array([S.g1_status(r) for r in p], np.int32)

    def g2_validate_batch(self, p):
        p = np.asarray(p, np.uint64).reshape(-1, 24)
        self.calls.append(("g2_validate_batch", p.shape[0]))
        return np.array([S.g2_status(r) for r in p], np.int32)


class MinPkModel(_Validating, G2T.Model):
    def __init__(self):
        super().__init__()
        from bn_amd import G1
        self.g1_log[G1.one().limbs.tobytes()] = 1                                 # what a rejected row's key is replaced by


class MinSigModel(_Validating, G1T.Model):
    def __init__(self):
        super().__init__()
        from bn_amd import G2
        self.g2_log[G2.one().limbs.tobytes()] = 1


def test_the_api_is_one_engine_call():
    import bn_amd
    m = MinPkModel()
    rows, want = S.g2_batch(len(S.g2_cases()))
    got = bn_amd.g2_validate_batch(rows, engine=m)
    assert m.calls == [("g2_validate_batch", len(want))] and np.array_equal(got, want)
    m.calls.clear()
    pts = [bn_amd.G1(r) for r in S.g1_batch(5)[0]]
    assert np.array_equal(bn_amd.g1_validate_batch(pts, engine=m), S.g1_batch(5)[1]) and m.calls == [("g1_validate_batch", 5)]
    assert bn_amd.g2_validate_batch([], engine=m).shape == (0,)


def _mapped_g2():
    from bn_amd import G2
    return G2(HC.words(HC.map_to_curve((0, 1))))


def test_bls_minpk_validates_with_two_more_calls_and_only_when_asked():
    from bn_amd import Fr, G1, bls_minpk as bls
    m = MinPkModel()
    sks = [Fr(11 + 7 * i) for i in range(4)]
    pks = bls.public_keys(sks, engine=m)
    msgs = [bytes([i]) * 8 for i in range(4)]
    sigs = bls.sign_batch(sks, msgs, engine=m)
    today = [("g2_hash_to_curve_batch", (4, 8)), ("pairing_product_batch", 4, [2])]
    m.calls.clear()
    assert bls.verify_batch(pks, msgs, sigs, engine=m).all() and m.calls == today             # the default: exactly today's calls
    m.calls.clear()
    assert bls.verify_batch(pks, msgs, sigs, engine=m, validate=False).all() and m.calls == today
    m.calls.clear()
    ok = bls.verify_batch(pks, msgs, sigs, engine=m, validate=True)
    assert m.calls == [("g1_validate_batch", 4), ("g2_validate_batch", 4)] + today and ok.dtype == bool and ok.all()
    spoiled = list(sigs); spoiled[1] = _mapped_g2()                                            # on the twist, not in G2
    assert bls.verify_batch(pks, msgs, spoiled, engine=m, validate=True).tolist() == [True, False, True, True]
    wrong = list(sigs); wrong[3] = sigs[0]                                                     # valid points, wrong signature
    assert bls.verify_batch(pks, msgs, wrong, engine=m, validate=True).tolist() == [True, True, True, False]
    no_key = list(pks); no_key[2] = G1.zero()
    assert bls.verify_batch(no_key, msgs, sigs, engine=m, validate=True).tolist() == [True, True, False, True]
    off = pks[0].limbs.copy(); off[4] ^= np.uint64(1)
    bad_key = list(pks); bad_key[0] = G1(off)
    assert bls.verify_batch(bad_key, msgs, sigs, engine=m, validate=True).tolist() == [False, True, True, True]
    assert bls.verify_batch([], [], [], engine=G1T.NoDevice(), validate=True).shape == (0,)


def test_bls_validates_with_two_more_calls_and_only_when_asked():
    from bn_amd import Fr, G1, G2, bls
    m = MinSigModel()
    sks = [Fr(5 + 3 * i) for i in range(3)]
    pks = bls.public_keys(sks, engine=m)
    msgs = [bytes([i]) * 8 for i in range(3)]
    sigs = bls.sign_batch(sks, msgs, engine=m)
    m.calls.clear()
    assert bls.verify_batch(pks, msgs, sigs, engine=m).all()
    today = list(m.calls)
    assert not any("validate" in c[0] for c in today)
    m.calls.clear()
    assert bls.verify_batch(pks, msgs, sigs, engine=m, validate=True).all()
    assert m.calls == [("g1_validate_batch", 3), ("g2_validate_batch", 3)] + today
    bad_key = list(pks); bad_key[1] = _mapped_g2()
    assert bls.verify_batch(bad_key, msgs, sigs, engine=m, validate=True).tolist() == [True, False, True]
    no_key = list(pks); no_key[0] = G2.zero()
    assert bls.verify_batch(no_key, msgs, sigs, engine=m, validate=True).tolist() == [False, True, True]
    off = sigs[2].limbs.copy(); off[0] ^= np.uint64(1)
    bad_sig = list(sigs); bad_sig[2] = G1(off)
    assert bls.verify_batch(pks, msgs, bad_sig, engine=m, validate=True).tolist() == [True, True, False]


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


def test_argument_errors_answer_without_a_device(lib):
    for name in NAMES[:2]:
        f, fd = getattr(lib, name), getattr(lib, name + "_dev")
        assert f(None, None, DUMMY, 1) == BAD_ARG and f(None, DUMMY, None, 1) == BAD_ARG, name
        assert fd(None, None, DUMMY, 1, None) == BAD_ARG and fd(None, DUMMY, None, 1, None) == BAD_ARG, name
        assert f(None, DUMMY, DUMMY, (1 << 40) + 1) == BAD_ARG and fd(None, DUMMY, DUMMY, (1 << 40) + 1, None) == BAD_ARG, name


def test_no_work_is_ok(lib):
    for name in NAMES[:2]:
        assert getattr(lib, name)(None, None, None, 0) == 0 and getattr(lib, name + "_dev")(None, None, None, 0, None) == 0, name


def test_the_hook_checks_its_bounds(lib):
    try:
        assert lib.bn254_validate_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_validate_set_launch_max(64) == 0
    finally:
        assert lib.bn254_validate_set_launch_max(0) == 0


def test_the_kernels_are_instances_of_bn254_fr_decode_k_without_spill_or_lds():
    import isa_mix
    import kernel_meta
    import lane_shell
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    src = lane_shell.unit_source("bn254_validate.hip")  # the unit adds no kernel under a new name: the shell is lane_launch.hpp's
    assert "__global__" not in src
    for text in (src, (ROOT / "bn_amd" / "csrc" / "subgroup_ops.hpp").read_text()):
        assert "__shared__" not in text and "atomic" not in text.lower()
    assert so.exists() and (isa_mix.LLVM / "llvm-readelf").exists()
    meta = kernel_meta.instances(so)
    for op in OPS:
        mine = [n for n in meta if re.search(r"\d+" + op + r"(E|I)", n)]
        assert len(mine) == 1, (op, mine)
        assert kernel_meta.short_name(mine[0]) == "bn254_fr_decode_k", mine
        assert meta[mine[0]]["spill"] == 0 == SPILL_CEILING["bn254_fr_decode_k"], (mine[0], meta[mine[0]])
        assert meta[mine[0]]["lds"] == 0, (mine[0], meta[mine[0]])
    decoders = [n for n in meta if kernel_meta.short_name(n) == "bn254_g2_decode_k"]            # the wire decoder and G2DecompressOp: the first users of the test
    assert len(decoders) == 2 and all(meta[n]["spill"] <= SPILL_CEILING["bn254_g2_decode_k"] == 18 for n in decoders), [(n, meta[n]) for n in decoders]
