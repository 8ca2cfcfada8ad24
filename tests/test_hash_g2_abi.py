"""Hash-to-curve for G2 and cofactor clearing (bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch, bn254_g2_hash_to_curve_uniform_batch,
bn254_g2_hash_to_curve_batch and their _dev twins) without a GPU: the eight symbols and their declarations in every layer that mirrors the C
header, the argument checks that answer before any device is touched, the Python surface, bn_amd.api and bn_amd.bls_minpk over a stand-in engine
that answers from the integer model of hash_g2_cases.py - the numbers of engine calls they promise, their ValueError paths - the constants of the
device code re-derived from the formulas, and the register budget of the kernels: template instances of bn254_fr_decode_k<Op> only.  Neither the
constants nor the outputs are checked against gnark-crypto or any other library."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import bn_model as M
import hash_g2_cases as HC
import test_binding_signatures as B
import test_hash_abi as G1T

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, N, BYTES_IN, G2_IN, G2_OUT = ("void", MUT), ("usize", ()), ("u8", CONST), ("g2", CONST), ("g2", MUT)
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_g2_map_to_curve_batch": [CTX, BYTES_IN, G2_OUT, N],
    "bn254_g2_clear_cofactor_batch": [CTX, G2_IN, G2_OUT, N],
    "bn254_g2_hash_to_curve_uniform_batch": [CTX, BYTES_IN, G2_OUT, N],
    "bn254_g2_hash_to_curve_batch": [CTX, BYTES_IN, N, BYTES_IN, N, G2_OUT, N],
    "bn254_g2_map_to_curve_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_g2_clear_cofactor_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_g2_hash_to_curve_uniform_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_g2_hash_to_curve_batch_dev": [CTX, D_IN, N, BYTES_IN, N, D_OUT, N, D_OUT],
}
NAMES = tuple(EXPECTED)
HOOKS = ("bn254_hash_g2_set_launch_max",)
SCOPES = ("g2_map_to_curve", "g2_clear_cofactor", "g2_hash_to_curve", "g2_hash_to_curve_msg")
OPS = ("G2MapToCurveOp", "G2ClearCofactorOp", "G2HashUniformOp", "G2HashMsgOp")
NOT_CHECKED = "checked against gnark-crypto or any other library"
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_hash_g2_set_launch_max.argtypes = [C.c_size_t]
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
    assert any(s.name == "bn254_hash_g2.hip" for s in _native.SOURCES)


def test_header_declares_the_eight_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    for d in ("BN254_H2C_G2_FIELD_BYTES 96", "BN254_H2C_G2_UNIFORM_BYTES 192"):
        assert re.search(r"^#define " + d + "$", hdr, re.M), d
    assert hdr.index("bn254_g1_hash_to_curve_batch_dev(bn254_ctx") < hdr.index("/* Hash to G2") < hdr.index("#define BN254_H2C_G2_FIELD_BYTES") < hdr.index("/* ---- device-resident entry points")
    own = " ".join(hdr[hdr.index("/* Hash to G2"):hdr.index("#define BN254_H2C_G2_FIELD_BYTES")].split())
    for word in ("CHECKED AGAINST gnark-crypto OR ANY OTHER LIBRARY", "find_z_svdw", "Z = 1", "sign_0 | (zero_0 & sign_1)", "inv0(0) = 0", "zero counts as a square",
                 "48 big-endian bytes", "below 2^384", "NOT IN G2", "2q - r", "[u]P + psi([3u]P) + psi^2([u]P) + psi^3(P)", "4965661367192848881", "NOT [2q - r]P",
                 "never the GLS multiplication", "CALLER's responsibility", "Z = 0 counts as infinity", "G2::zero() = (0, 1, 0)", "out may be exactly p",
                 "u0.c0 | u0.c1 | u1.c0 | u1.c1", "expand_message_xmd(msg, dst, 192)", "SHA-256", "msg_len == 0 is allowed", "HOST pointer", "BN254_E_BAD_ARG",
                 "dst_len == 0", "msg_len > 2^20", "n * msg_len > 2^40", "n == 0 succeeds"):
        assert word in own, word
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for text in (semantics, threading):
        for name in NAMES:
            assert name in text, name
    for hook in HOOKS:                                                                          # the test hook is internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"g2_map_to_curve"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)                   # a line of its own
    src = (ROOT / "bn_amd" / "csrc" / "bn254_hash_g2.hip").read_text()
    assert set(SCOPES) <= set(re.findall(r'"(\w+)"', src))


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn g2_map_to_curve_batch(u: &[u8]) -> Result<Vec<G2>, GpuError>",
               "pub fn g2_clear_cofactor_batch(p: &[G2]) -> Result<Vec<G2>, GpuError>",
               "pub fn g2_hash_to_curve_uniform_batch(uniform: &[u8]) -> Result<Vec<G2>, GpuError>",
               "pub fn g2_hash_to_curve_batch(msgs: &[u8], msg_len: usize, n: usize, dst: &[u8]) -> Result<Vec<G2>, GpuError>"):
        assert fn in txt, fn
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<G2> g2_map_to_curve(", "std::vector<G2> g2_clear_cofactor(", "std::vector<G2> g2_hash_to_curve_uniform(", "std::vector<G2> g2_hash_to_curve(",
              "bn254_g2_map_to_curve_batch(", "bn254_g2_clear_cofactor_batch(", "bn254_g2_hash_to_curve_uniform_batch(", "bn254_g2_hash_to_curve_batch("):
        assert s in hpp, s
    variant = (ROOT / "tools" / "build_variant.sh").read_text()
    assert re.search(r"^for u in .*\bbn254_hash_g2\b.*; do$", variant, re.M)
    csrc = ROOT / "bn_amd" / "csrc"
    for text in (hpp, txt, (ROOT / "bn_amd" / "hash_to_curve.py").read_text(), (ROOT / "bn_amd" / "bls_minpk.py").read_text(), (csrc / "hash_g2_ops.hpp").read_text(),
                 (csrc / "bn254_hash_g2.hip").read_text(), (ROOT / "bn_amd" / "engine.py").read_text(), (ROOT / "bn_amd" / "api.py").read_text()):
        flat = " ".join(text.replace("///", " ").replace("//", " ").split())
        assert NOT_CHECKED in flat
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        flat = " ".join(text.split())
        assert "Neither the constants nor the outputs are checked against gnark-crypto or any other library" in flat, doc
        for name in NAMES[:4] + ("bn_amd.bls_minpk", "hash to G2"):
            assert name in text, (doc, name)
        for word in ("`encode_to_curve`", "mixed lengths on the device", "endomorphism subgroup test", "shorter addition chain for `u`", "multi-GPU"):      # the "not built" list
            assert word in flat, (doc, word)
    readme = (ROOT / "README.md").read_text()
    assert "profiles/r23_hash_g2.txt" in readme and (ROOT / "tools" / "time_hash_g2.py").exists()
    assert "bls_minpk" in " ".join((ROOT / "bn_amd" / "bls.py").read_text().split("\n")[:12])


def test_the_device_constants_are_the_formulas():
    """Z by the RFC's search over Fq2 and c1 .. c4 from it (hash_g2_cases.py derives them), against what tools/gen_device_constants.py wrote -
    Montgomery radix 2^261 in 29-bit limbs - and against the literals the generator asserts"""
    txt = (ROOT / "bn_amd" / "csrc" / "bn254_constants.hpp").read_text()
    for name, want in (("H2C_G2_C1", HC.C1), ("H2C_G2_C3", HC.C3), ("H2C_G2_C4", HC.C4)):
        m = re.search(r"uint32_t %s\[2\]\[9\] = \{\{([^}]*)\}, \{([^}]*)\}\}" % name, txt)
        for half, w in zip(m.groups(), want):
            limbs = [int(x.strip().rstrip("u"), 16) for x in half.split(",")]
            assert len(limbs) == 9 and all(l < 1 << 29 for l in limbs)
            assert sum(l << (29 * i) for i, l in enumerate(limbs)) == w * (1 << 261) % M.Q, name
    assert HC.Z == (1, 0) and HC.C1 == M.f2_add((1, 0), M.G2_B) and HC.C2 == ((M.Q - 1) // 2, 0) and HC.sgn0(HC.C3) == 0
    assert M.f2_sqr(HC.C3) == M.f2_scale(HC.C1, -3 % M.Q) and M.f2_scale(HC.C4, 3) == M.f2_scale(HC.C1, -4 % M.Q)
    gen = (ROOT / "tools" / "gen_device_constants.py").read_text()
    for v in HC.C3 + HC.C4:
        assert str(v) in gen
    assert "find_z_svdw_g2" in gen
    ops = (ROOT / "bn_amd" / "csrc" / "hash_g2_ops.hpp").read_text()
    for s in ("k::H2C_G2_C1", "k::H2C_C2", "k::H2C_G2_C3", "k::H2C_G2_C4", "k::TWIST_MUL_BY_Q_X", "k::TWIST_MUL_BY_Q_Y", "k::GLS_W", "k::GLS_WGX", "k::BN_U", "add_body<H2cF2>"):
        assert s in ops, s
    assert "scalar_mul_gls(" not in ops.split("#pragma once")[1]                                # the clearing never takes the GLS multiplication
    assert M.U == 4965661367192848881 and HC.CLEAR_K == (M.U + 3 * M.U * HC.LAMBDA + M.U * HC.LAMBDA ** 2 + HC.LAMBDA ** 3) % M.R_ORD != 0


def test_python_surface():
    import bn_amd
    from bn_amd import bls, bls_minpk, engine, hash_to_curve
    E = engine.Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.g2_map_to_curve_batch) == ["self", "u"] and sig(E.g2_clear_cofactor_batch) == ["self", "p"] and sig(E.g2_hash_to_curve_uniform_batch) == ["self", "uniform"]
    assert sig(E.g2_hash_to_curve_batch) == ["self", "msgs", "dst"]
    assert sig(E.g2_map_to_curve_batch_dev) == ["self", "d_u", "d_out", "n", "stream"] and sig(E.g2_clear_cofactor_batch_dev) == ["self", "d_p", "d_out", "n", "stream"]
    assert sig(E.g2_hash_to_curve_uniform_batch_dev) == ["self", "d_uniform", "d_out", "n", "stream"]
    assert sig(E.g2_hash_to_curve_batch_dev) == ["self", "d_msgs", "msg_len", "dst", "d_out", "n", "stream"]
    assert sig(bn_amd.g2_map_to_curve_batch) == ["us", "engine"] and sig(bn_amd.g2_clear_cofactor_batch) == ["points", "engine"]
    assert sig(bn_amd.g2_hash_to_curve_batch) == ["msgs", "dst", "engine"] and sig(bn_amd.G2.hash) == ["msg", "dst"]
    assert (engine.H2C_G2_FIELD_BYTES, engine.H2C_G2_UNIFORM_BYTES) == (96, 192)
    assert sig(hash_to_curve.hash_to_field) == ["msg", "dst", "count", "m"]
    p = inspect.signature(hash_to_curve.hash_to_field).parameters
    assert (p["count"].default, p["m"].default) == (2, 1)
    assert bls_minpk.DST == hash_to_curve.BLS_G2_DST == b"BLS_SIG_BN254G2_XMD:SHA-256_SVDW_RO_NUL_" == HC.BLS_G2_DST
    assert bls.DST == hash_to_curve.BLS_DST == b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"             # bls keeps its tag
    for mod in (bls, bls_minpk):
        assert sig(mod.keygen) == ["rng"] and sig(mod.public_keys)[:1] == ["sks"]
        assert sig(mod.sign_batch)[:3] == ["sks", "msgs", "dst"] and sig(mod.sign)[:3] == ["sk", "msg", "dst"]
        assert sig(mod.verify_batch)[:4] == ["pks", "msgs", "sigs", "dst"] and sig(mod.verify)[:4] == ["pk", "msg", "sig", "dst"]
        assert sig(mod.aggregate)[:1] == ["sigs"] and sig(mod.verify_aggregate)[:4] == ["pks", "msgs", "sig", "dst"]
        assert sig(mod.fast_aggregate_verify)[:4] == ["pks", "msg", "sig", "dst"]
        assert "proofs of possession" in " ".join(mod.fast_aggregate_verify.__doc__.split())
        for f in (mod.sign_batch, mod.verify_batch, mod.verify_aggregate, mod.fast_aggregate_verify):
            assert inspect.signature(f).parameters["dst"].default == mod.DST


def test_the_host_expansion_is_the_model():
    from bn_amd import hash_to_curve as H
    import hash_cases as G1C
    for dl in HC.DST_LENS:
        for ml in HC.msg_lens(dl):
            msg = HC.messages(1, ml, dl)[0].tobytes()
            assert H.hash_to_field(msg, HC.dst_of(dl), 2, 2) == HC.hash_to_field(msg, HC.dst_of(dl))
            assert H.hash_to_field(msg, HC.dst_of(dl), m=1) == G1C.hash_to_field(msg, HC.dst_of(dl))           # m = 1 is what it was
            assert H.uniform_bytes_g2([msg], HC.dst_of(dl))[0].tobytes() == HC.expand_message_xmd(msg, HC.dst_of(dl), 192)
    assert H.uniform_bytes_g2([], b"tag").shape == (0, 192) and H.uniform_bytes([], b"tag").shape == (0, 96)
    with pytest.raises(ValueError):
        H.hash_to_field(b"m", b"tag", 2, 3)


# ------------------------------------------------------------------------------------------------------------------ a stand-in engine
O1, O2, R = M.FQ_OPS, M.FQ2_OPS, M.R_ORD
NoDevice, _g1, _g2, _g1_words, _g2_words, _scalar = G1T.NoDevice, G1T._g1, G1T._g2, G1T._g1_words, G1T._g2_words, G1T._scalar


class Model:
    """answers from the integer model and records what was asked.  Pairings are answered in the exponent: every G1 point it meets is a
    multiple k of G1::one() that it handed out itself (or the constant -G1::one()), so e(k G1, Q) = e(G1, k Q) and a product is one iff the sum
    of k_i Q_i is zero in G2."""
    def __init__(self):
        self.calls = []
        self.g1_log = {}

    def _k(self, row):
        return self.g1_log[np.asarray(row, np.uint64).tobytes()]

    def g2_hash_to_curve_batch(self, msgs, dst):
        msgs = np.asarray(msgs, np.uint8)
        self.calls.append(("g2_hash_to_curve_batch", msgs.shape))
        return np.stack([HC.words(HC.hash_to_curve(m.tobytes(), dst)) for m in msgs])

    def g2_hash_to_curve_uniform_batch(self, uniform):
        uniform = np.asarray(uniform, np.uint8).reshape(-1, 192)
        self.calls.append(("g2_hash_to_curve_uniform_batch", uniform.shape[0]))
        return np.stack([HC.words(HC.hash_uniform(u.tobytes())) for u in uniform])

    def g2_map_to_curve_batch(self, u):
        u = np.asarray(u, np.uint8).reshape(-1, 96)
        self.calls.append(("g2_map_to_curve_batch", u.shape[0]))
        rows = [HC.words(HC.map_to_curve((int.from_bytes(r[:48].tobytes(), "big"), int.from_bytes(r[48:].tobytes(), "big")))) for r in u]
        return np.stack(rows) if rows else np.zeros((0, 24), np.uint64)

    def g2_clear_cofactor_batch(self, p):
        p = np.asarray(p, np.uint64).reshape(-1, 24)
        self.calls.append(("g2_clear_cofactor_batch", p.shape[0]))
        return np.stack([HC.words(HC.aff(HC.clear_jac(_g2(r)))) for r in p])

    def g1_mul_base_batch(self, base, k):
        from bn_amd import G1
        assert np.array_equal(np.asarray(base).reshape(-1), G1.one().limbs)
        self.calls.append(("g1_mul_base_batch", len(k)))
        out = []
        for row in np.asarray(k, np.uint64).reshape(-1, 4):
            w = _g1_words(M.g_normalize(O1, M.g_mul(O1, M.G1_ONE, _scalar(row))))
            self.g1_log[w.tobytes()] = _scalar(row)
            out.append(w)
        return np.stack(out)

    def g2_mul_batch(self, p, k):
        self.calls.append(("g2_mul_batch", len(p)))
        return np.stack([_g2_words(M.g_normalize(O2, M.g_mul(O2, _g2(a), _scalar(b)))) for a, b in zip(np.asarray(p), np.asarray(k))])

    def g2_msm(self, p, k):
        self.calls.append(("g2_msm", len(p)))
        acc = M.g_zero(O2)
        for a, b in zip(np.asarray(p), np.asarray(k)):
            acc = M.g_add(O2, acc, M.g_mul(O2, _g2(a), _scalar(b)))
        return _g2_words(M.g_normalize(O2, acc))

    def g1_msm(self, p, k):
        self.calls.append(("g1_msm", len(p)))
        assert all(_scalar(b) == 1 for b in np.asarray(k))
        total = sum(self._k(a) for a in np.asarray(p)) % R
        w = _g1_words(M.g_normalize(O1, M.g_mul(O1, M.G1_ONE, total)))
        self.g1_log[w.tobytes()] = total
        return w

    def _product_is_one(self, P, Q):
        from bn_amd import bls_minpk
        self.g1_log.setdefault(bls_minpk._neg_g1_one().tobytes(), R - 1)
        acc = M.g_zero(O2)
        for a, b in zip(P, Q):
            acc = M.g_add(O2, acc, M.g_mul(O2, _g2(b), self._k(a)))
        return M.g_is_zero(O2, acc)

    def _gt(self, one):
        from bn_amd import Gt
        out = Gt.one().limbs.copy()
        if not one:
            out[5] = 7
        return out

    def pairing_product(self, p, q):
        self.calls.append(("pairing_product", len(p)))
        return self._gt(self._product_is_one(np.asarray(p), np.asarray(q)))

    def pairing_product_batch(self, p, q, offsets):
        offs = [int(x) for x in offsets]
        self.calls.append(("pairing_product_batch", len(offs) - 1, sorted({b - a for a, b in zip(offs, offs[1:])})))
        return np.stack([self._gt(self._product_is_one(np.asarray(p)[a:b], np.asarray(q)[a:b])) for a, b in zip(offs, offs[1:])])


def test_the_negated_generator_is_a_constant():
    from bn_amd import bls_minpk
    assert _g1(bls_minpk._neg_g1_one()) == M.g_neg(O1, M.G1_ONE)


def test_api_routes_equal_and_mixed_lengths_to_the_same_bytes():
    import bn_amd
    m = Model()
    same = [b"abcd", b"efgh"]
    got = bn_amd.g2_hash_to_curve_batch(same, b"tag", engine=m)
    assert m.calls == [("g2_hash_to_curve_batch", (2, 4))]                       # one length: the device's SHA-256
    assert all(isinstance(p, bn_amd.G2) and np.array_equal(p.limbs, HC.words(HC.hash_to_curve(s, b"tag"))) for p, s in zip(got, same))
    m.calls.clear()
    mixed = [b"", b"a", b"abcd"]
    got = bn_amd.g2_hash_to_curve_batch(mixed, b"tag", engine=m)
    assert m.calls == [("g2_hash_to_curve_uniform_batch", 3)]                    # mixed lengths: hashlib, then the uniform call
    assert all(np.array_equal(p.limbs, HC.words(HC.hash_to_curve(s, b"tag"))) for p, s in zip(got, mixed))
    m.calls.clear()
    pts = bn_amd.g2_map_to_curve_batch([(0, 0), (0, 1), ((1 << 384) - 1, 5)], engine=m)
    assert m.calls == [("g2_map_to_curve_batch", 3)] and np.array_equal(pts[2].limbs, HC.words(HC.map_to_curve(((1 << 384) - 1, 5))))
    assert bn_amd.g2_map_to_curve_batch([], engine=m) == []
    m.calls.clear()
    cl = bn_amd.g2_clear_cofactor_batch(pts, engine=m)
    assert m.calls == [("g2_clear_cofactor_batch", 3)] and np.array_equal(cl[1].limbs, HC.words(HC.clear(HC.map_to_curve((0, 1)))))


def test_errors_raise_before_any_device_call():
    import bn_amd
    from bn_amd import bls_minpk as bls
    nd = NoDevice()
    for dst in (b"", b"x" * 256):
        with pytest.raises(ValueError, match="1 .. 255 bytes"):
            bn_amd.g2_hash_to_curve_batch([b"m"], dst, engine=nd)
    with pytest.raises(ValueError, match=r"\(n, msg_len\) uint8"):
        bn_amd.g2_hash_to_curve_batch(np.zeros(5, np.uint8), b"tag", engine=nd)
    with pytest.raises(OverflowError):
        bn_amd.g2_map_to_curve_batch([(0, 1 << 384)], engine=nd)
    one = bn_amd.G1.one(); two = bn_amd.G2.one()
    with pytest.raises(ValueError, match="distinct messages"):
        bls.verify_aggregate([one, one, one], [b"a", b"b", b"a"], two, engine=nd)
    with pytest.raises(ValueError, match="distinct messages"):
        bls.verify_aggregate([one, one], np.zeros((2, 8), np.uint8), two, engine=nd)
    with pytest.raises(ValueError, match="as many public keys as messages"):
        bls.verify_aggregate([one], [b"a", b"b"], two, engine=nd)
    with pytest.raises(ValueError, match="as many messages as secret keys"):
        bls.sign_batch([bn_amd.Fr(1)], [b"a", b"b"], engine=nd)
    with pytest.raises(ValueError, match="as many public keys and signatures as messages"):
        bls.verify_batch([one], [b"a"], [two, two], engine=nd)
    assert bls.sign_batch([], [], engine=nd) == [] and bls.verify_batch([], [], [], engine=nd).shape == (0,)
    assert bls.verify_aggregate([], [], two, engine=nd) is False and bls.fast_aggregate_verify([], b"m", two, engine=nd) is False


def test_bls_minpk_over_the_stand_in_engine_makes_the_calls_it_promises():
    from bn_amd import Fr, G2, bls_minpk as bls
    m = Model()
    sks = [Fr(11 + 7 * i) for i in range(4)]
    pks = bls.public_keys(sks, engine=m)
    assert m.calls == [("g1_mul_base_batch", 4)]
    msgs = [bytes([i]) * 8 for i in range(4)]
    m.calls.clear()
    sigs = bls.sign_batch(sks, msgs, engine=m)
    assert m.calls == [("g2_hash_to_curve_batch", (4, 8)), ("g2_mul_batch", 4)]
    for sk, msg, sig in zip(sks, msgs, sigs):
        h = HC.hash_to_curve(msg, bls.DST)
        assert np.array_equal(sig.limbs, _g2_words(M.g_normalize(O2, M.g_mul(O2, HC.jac(h), sk.v))))
    assert np.array_equal(bls.sign(sks[2], msgs[2], engine=m).limbs, sigs[2].limbs)
    m.calls.clear()
    ok = bls.verify_batch(pks, msgs, sigs, engine=m)
    assert m.calls == [("g2_hash_to_curve_batch", (4, 8)), ("pairing_product_batch", 4, [2])]             # no addition call: -G1::one() is a constant
    assert ok.dtype == bool and ok.all()
    spoiled = list(sigs); spoiled[3] = sigs[1]
    assert bls.verify_batch(pks, msgs, spoiled, engine=m).tolist() == [True, True, True, False]
    assert bls.verify(pks[0], msgs[0], sigs[0], engine=m) is True and bls.verify(pks[1], msgs[0], sigs[0], engine=m) is False
    assert bls.verify(pks[0], msgs[0], sigs[0], dst=b"another tag", engine=m) is False
    m.calls.clear()
    mixed = [b"", b"a", b"bb", b"ccc"]
    assert bls.verify_batch(pks, mixed, bls.sign_batch(sks, mixed, engine=m), engine=m).all()
    assert [c[0] for c in m.calls] == ["g2_hash_to_curve_uniform_batch", "g2_mul_batch", "g2_hash_to_curve_uniform_batch", "pairing_product_batch"]
    m.calls.clear()
    agg = bls.aggregate(sigs, engine=m)
    assert m.calls == [("g2_msm", 4)]
    m.calls.clear()
    assert bls.verify_aggregate(pks, msgs, agg, engine=m) is True
    assert m.calls == [("g2_hash_to_curve_batch", (4, 8)), ("pairing_product", 5)]
    assert bls.verify_aggregate(pks, msgs[1:] + msgs[:1], agg, engine=m) is False
    assert bls.verify_aggregate(pks[:3], msgs[:3], agg, engine=m) is False
    one = b"one message"
    same = bls.aggregate(bls.sign_batch(sks, [one] * 4, engine=m), engine=m)
    m.calls.clear()
    assert bls.fast_aggregate_verify(pks, one, same, engine=m) is True
    assert m.calls == [("g1_msm", 4), ("g2_hash_to_curve_batch", (1, len(one))), ("pairing_product", 2)]
    assert bls.fast_aggregate_verify(pks[:3], one, same, engine=m) is False
    assert bls.fast_aggregate_verify(pks, one, G2.zero(), engine=m) is False


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read
TAG = b"tag"


def test_argument_errors_answer_without_a_device(lib):
    for name in ("bn254_g2_map_to_curve_batch", "bn254_g2_clear_cofactor_batch", "bn254_g2_hash_to_curve_uniform_batch"):
        f, fd = getattr(lib, name), getattr(lib, name + "_dev")
        assert f(None, None, DUMMY, 1) == BAD_ARG and f(None, DUMMY, None, 1) == BAD_ARG, name
        assert fd(None, None, DUMMY, 1, None) == BAD_ARG and fd(None, DUMMY, None, 1, None) == BAD_ARG, name
        assert f(None, DUMMY, DUMMY, (1 << 40) + 1) == BAD_ARG and fd(None, DUMMY, DUMMY, (1 << 40) + 1, None) == BAD_ARG, name
    cases = [("a NULL tag", DUMMY, 4, None, 3, DUMMY, 1), ("an empty tag", DUMMY, 4, TAG, 0, DUMMY, 1), ("a tag of 256 bytes", DUMMY, 4, b"x" * 256, 256, DUMMY, 1),
             ("an empty tag without work", DUMMY, 4, TAG, 0, DUMMY, 0), ("NULL messages of 4 bytes", None, 4, TAG, 3, DUMMY, 1), ("a NULL output", DUMMY, 4, TAG, 3, None, 1),
             ("a NULL output for empty messages", None, 0, TAG, 3, None, 1), ("messages above 2^20 bytes", DUMMY, (1 << 20) + 1, TAG, 3, DUMMY, 1),
             ("n above 2^40", DUMMY, 0, TAG, 3, DUMMY, (1 << 40) + 1), ("n * msg_len above 2^40", DUMMY, 1 << 20, TAG, 3, DUMMY, (1 << 20) + 1)]
    for what, msgs, ml, dst, dl, out, n in cases:
        assert lib.bn254_g2_hash_to_curve_batch(None, msgs, ml, dst, dl, out, n) == BAD_ARG, what
        assert lib.bn254_g2_hash_to_curve_batch_dev(None, msgs, ml, dst, dl, out, n, None) == BAD_ARG, what


def test_no_work_is_ok(lib):
    for name in ("bn254_g2_map_to_curve_batch", "bn254_g2_clear_cofactor_batch", "bn254_g2_hash_to_curve_uniform_batch"):
        assert getattr(lib, name)(None, None, None, 0) == 0 and getattr(lib, name + "_dev")(None, None, None, 0, None) == 0, name
    assert lib.bn254_g2_hash_to_curve_batch(None, None, 32, TAG, 3, None, 0) == 0 and lib.bn254_g2_hash_to_curve_batch_dev(None, None, 32, TAG, 3, None, 0, None) == 0
    assert lib.bn254_g2_hash_to_curve_batch(None, None, 0, None, 3, None, 0) == 0


def test_the_hook_checks_its_bounds(lib):
    try:
        assert lib.bn254_hash_g2_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_hash_g2_set_launch_max(64) == 0
    finally:
        assert lib.bn254_hash_g2_set_launch_max(0) == 0


def test_the_kernels_are_instances_of_bn254_fr_decode_k_without_spill_or_lds():
    import isa_mix
    import kernel_meta
    import lane_shell
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    src = lane_shell.unit_source("bn254_hash_g2.hip")  # the unit adds no kernel under a new name: the shell is lane_launch.hpp's
    assert "__global__" not in src
    for text in (src, (ROOT / "bn_amd" / "csrc" / "hash_g2_ops.hpp").read_text()):
        assert "__shared__" not in text and "atomic" not in text.lower()
    assert so.exists() and (isa_mix.LLVM / "llvm-readelf").exists()
    meta = kernel_meta.instances(so)
    for op in OPS:
        mine = [n for n in meta if re.search(r"\d+" + op + r"(E|I)", n)]
        assert len(mine) == 1, (op, mine)
        assert kernel_meta.short_name(mine[0]) == "bn254_fr_decode_k", mine
        assert meta[mine[0]]["spill"] == 0 == SPILL_CEILING["bn254_fr_decode_k"], (mine[0], meta[mine[0]])
        assert meta[mine[0]]["lds"] == 0, (mine[0], meta[mine[0]])
