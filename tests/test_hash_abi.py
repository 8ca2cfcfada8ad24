"""Hash-to-curve for G1 (bn254_g1_map_to_curve_batch, bn254_g1_hash_to_curve_uniform_batch, bn254_g1_hash_to_curve_batch and their _dev twins)
without a GPU: the six symbols and their declarations in every layer that mirrors the C header, the argument checks that answer before any
device is touched, the Python surface, bn_amd.api and bn_amd.bls over a stand-in engine that answers from the integer model of hash_cases.py
- the numbers of engine calls they promise, their ValueError paths, the routes of equal-length and mixed-length messages - the constants of
the device code re-derived from the formulas, and the register budget of the kernels: template instances of bn254_fr_decode_k<Op> only."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import bn_model as M
import hash_cases as HC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, N, BYTES_IN, G1_OUT = ("void", MUT), ("usize", ()), ("u8", CONST), ("g1", MUT)
D_IN, D_OUT = ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_g1_map_to_curve_batch": [CTX, BYTES_IN, G1_OUT, N],
    "bn254_g1_hash_to_curve_uniform_batch": [CTX, BYTES_IN, G1_OUT, N],
    "bn254_g1_hash_to_curve_batch": [CTX, BYTES_IN, N, BYTES_IN, N, G1_OUT, N],
    "bn254_g1_map_to_curve_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_g1_hash_to_curve_uniform_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_g1_hash_to_curve_batch_dev": [CTX, D_IN, N, BYTES_IN, N, D_OUT, N, D_OUT],
}
NAMES = tuple(EXPECTED)
HOOKS = ("bn254_hash_set_launch_max", "bn254_hash_inv0_form")
SCOPES = ("g1_map_to_curve", "g1_hash_to_curve", "g1_hash_to_curve_msg")
OPS = ("G1MapToCurveOp", "G1HashUniformOp", "G1HashMsgOp")
NOT_CHECKED = "not checked against gnark-crypto or any other library"
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_hash_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_hash_inv0_form.argtypes = []
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
    assert any(s.name == "bn254_hash.hip" for s in _native.SOURCES)


def test_header_declares_the_six_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    for d in ("BN254_H2C_FIELD_BYTES 48", "BN254_H2C_UNIFORM_BYTES 96", "BN254_H2C_DST_MAX 255"):
        assert re.search(r"^#define " + d + "$", hdr, re.M), d
    assert hdr.index("bn254_g2_decompress_batch_dev(bn254_ctx") < hdr.index("/* Hash to G1") < hdr.index("#define BN254_H2C_FIELD_BYTES") < hdr.index("/* ---- device-resident entry points")
    own = " ".join(hdr[hdr.index("/* Hash to G1"):hdr.index("#define BN254_H2C_FIELD_BYTES")].split())
    for word in (NOT_CHECKED, "find_z_svdw", "Z = 1", "sgn0", "inv0(0) = 0", "zero counts as a square", "48 big-endian bytes", "below 2^384", "never gives the point at infinity",
                 "equal points double", "G::zero() = (0, 1, 0)", "cofactor is 1", "expand_message_xmd", "SHA-256", "msg_len == 0 is allowed", "HOST pointer", "BN254_E_BAD_ARG",
                 "dst_len == 0", "msg_len > 2^20", "n * msg_len > 2^40", "n == 0 succeeds"):
        assert word in own, word
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for text in (semantics, threading):
        for name in NAMES:
            assert name in text, name
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"g1_map_to_curve"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)
    assert not [l for l in block.split("\n") if '"g1_compress"' in l and '"g1_map_to_curve"' in l]          # a line of its own
    src = (ROOT / "bn_amd" / "csrc" / "bn254_hash.hip").read_text()
    assert set(SCOPES) <= set(re.findall(r'"(\w+)"', src))


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn g1_map_to_curve_batch(u: &[u8]) -> Result<Vec<G1>, GpuError>",
               "pub fn g1_hash_to_curve_uniform_batch(uniform: &[u8]) -> Result<Vec<G1>, GpuError>",
               "pub fn g1_hash_to_curve_batch(msgs: &[u8], msg_len: usize, n: usize, dst: &[u8]) -> Result<Vec<G1>, GpuError>"):
        assert fn in txt, fn
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<G1> g1_map_to_curve(", "std::vector<G1> g1_hash_to_curve_uniform(", "std::vector<G1> g1_hash_to_curve(",
              "bn254_g1_map_to_curve_batch(", "bn254_g1_hash_to_curve_uniform_batch(", "bn254_g1_hash_to_curve_batch("):
        assert s in hpp, s
    variant = (ROOT / "tools" / "build_variant.sh").read_text()
    assert re.search(r"^for u in .*\bbn254_hash\b.*; do$", variant, re.M) and "-DBN254_H2C_INV0=0" in variant
    for text in (hpp, txt, (ROOT / "bn_amd" / "hash_to_curve.py").read_text(), (ROOT / "bn_amd" / "bls.py").read_text(), (ROOT / "bn_amd" / "csrc" / "hash_ops.hpp").read_text()):
        assert NOT_CHECKED in " ".join(text.replace("///", " ").replace("//", " ").split())
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        assert NOT_CHECKED in " ".join(text.split()), doc
        for name in ("bn254_g1_map_to_curve_batch", "bn254_g1_hash_to_curve_uniform_batch", "bn254_g1_hash_to_curve_batch", "bn_amd.bls"):
            assert name in text, (doc, name)
        for word in ("hash to G2", "`encode_to_curve`", "`expand_message_xof`", "mixed length on the device", "three chains instead of four", "multi-GPU"):      # the "not built" list
            assert word in text, (doc, word)
    readme = (ROOT / "README.md").read_text()
    assert "one launch per call" in readme and "profiles/r22_hash.txt" in readme
    assert (ROOT / "tools" / "time_hash.py").exists()


def test_the_device_constants_are_the_formulas():
    """Z by the RFC's search and c2 .. c4 from it (hash_cases.py derives them), against what tools/gen_device_constants.py wrote - Montgomery
    radix 2^261 in 29-bit limbs - and against the literals the generator asserts"""
    txt = (ROOT / "bn_amd" / "csrc" / "bn254_constants.hpp").read_text()
    for name, want in (("H2C_C2", HC.C2), ("H2C_C3", HC.C3), ("H2C_C4", HC.C4)):
        m = re.search(r"uint32_t %s\[9\] = \{([^}]*)\}" % name, txt)
        limbs = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
        assert len(limbs) == 9 and all(l < 1 << 29 for l in limbs)
        v = sum(l << (29 * i) for i, l in enumerate(limbs))
        assert v == want * (1 << 261) % M.Q, name
    assert (HC.Z, HC.C1) == (1, 4) and HC.C3 * HC.C3 % M.Q == -12 % M.Q and HC.C4 * 3 % M.Q == -16 % M.Q and 2 * HC.C2 % M.Q == M.Q - 1
    gen = (ROOT / "tools" / "gen_device_constants.py").read_text()
    assert hex(HC.C3) in gen and hex(HC.C4) in gen and "find_z_svdw" in gen
    ops = (ROOT / "bn_amd" / "csrc" / "hash_ops.hpp").read_text()
    assert "fe_lc3<4, 0, 0>" in ops and "k::H2C_C2" in ops and "k::H2C_C3" in ops and "k::H2C_C4" in ops


def test_python_surface():
    import bn_amd
    from bn_amd import bls, engine, hash_to_curve
    E = engine.Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.g1_map_to_curve_batch) == ["self", "u"] and sig(E.g1_hash_to_curve_uniform_batch) == ["self", "uniform"]
    assert sig(E.g1_hash_to_curve_batch) == ["self", "msgs", "dst"]
    assert sig(E.g1_map_to_curve_batch_dev) == ["self", "d_u", "d_out", "n", "stream"]
    assert sig(E.g1_hash_to_curve_uniform_batch_dev) == ["self", "d_uniform", "d_out", "n", "stream"]
    assert sig(E.g1_hash_to_curve_batch_dev) == ["self", "d_msgs", "msg_len", "dst", "d_out", "n", "stream"]
    assert sig(bn_amd.g1_map_to_curve_batch) == ["us", "engine"] and sig(bn_amd.g1_hash_to_curve_batch) == ["msgs", "dst", "engine"]
    assert sig(bn_amd.G1.hash) == ["msg", "dst"]
    assert (engine.H2C_FIELD_BYTES, engine.H2C_UNIFORM_BYTES, engine.H2C_DST_MAX) == (48, 96, 255)
    assert sig(hash_to_curve.expand_message_xmd) == ["msg", "dst", "length"] and sig(hash_to_curve.hash_to_field)[:2] == ["msg", "dst"]
    assert bls.DST == hash_to_curve.BLS_DST == b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_" == HC.BLS_DST
    assert sig(bls.keygen) == ["rng"] and sig(bls.public_keys)[:1] == ["sks"]
    assert sig(bls.sign_batch)[:3] == ["sks", "msgs", "dst"] and sig(bls.sign)[:3] == ["sk", "msg", "dst"]
    assert sig(bls.verify_batch)[:4] == ["pks", "msgs", "sigs", "dst"] and sig(bls.verify)[:4] == ["pk", "msg", "sig", "dst"]
    assert sig(bls.aggregate)[:1] == ["sigs"] and sig(bls.verify_aggregate)[:4] == ["pks", "msgs", "sig", "dst"]
    assert sig(bls.fast_aggregate_verify)[:4] == ["pks", "msg", "sig", "dst"]
    assert "proofs of possession" in " ".join(bls.fast_aggregate_verify.__doc__.split())
    for f in (bls.sign_batch, bls.verify_batch, bls.verify_aggregate, bls.fast_aggregate_verify):
        assert inspect.signature(f).parameters["dst"].default == bls.DST


def test_the_host_expansion_is_the_model():
    from bn_amd import hash_to_curve as H
    quux = b"QUUX-V01-CS02-with-expander-SHA256-128"
    assert H.expand_message_xmd(b"", quux, 32).hex() == "68a985b87eb6b46952128911f2a4412bbc302a9d759667f87f7a21d803f07235"
    assert H.expand_message_xmd(b"abc", quux, 32).hex() == "d8ccab23b5985ccea865c6c97b6e5b8350e794e603b4b97902f53a8a0d605615"
    for dl in HC.DST_LENS:
        for ml in HC.msg_lens(dl):
            msg = HC.messages(1, ml, dl)[0].tobytes()
            assert H.expand_message_xmd(msg, HC.dst_of(dl), 96) == HC.expand_message_xmd(msg, HC.dst_of(dl), 96)
            assert H.hash_to_field(msg, HC.dst_of(dl)) == HC.hash_to_field(msg, HC.dst_of(dl))
    for dst in (b"", b"x" * 256):
        with pytest.raises(ValueError, match="1 .. 255 bytes"):
            H.expand_message_xmd(b"m", dst, 96)
    with pytest.raises(ValueError):
        H.expand_message_xmd(b"m", b"tag", 255 * 32 + 1)


# ------------------------------------------------------------------------------------------------------------------ a stand-in engine
class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


O = M.FQ_OPS
R = M.R_ORD


def _g1(row):
    return tuple(M.from_mont_limbs(row[4 * i:4 * i + 4]) for i in range(3))


def _g2(row):
    v = [M.from_mont_limbs(row[4 * i:4 * i + 4]) for i in range(6)]
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def _g1_words(p):
    return np.array([l for c in p for l in M.to_mont_limbs(c)], np.uint64)


def _g2_words(p):
    return np.array([l for two in p for c in two for l in M.to_mont_limbs(c)], np.uint64)


def _scalar(row):
    return M.from_mont_limbs(row, R)


class Model:
    """answers from the integer model and records what was asked.  Pairings are answered in the exponent: every G2 point it meets is a
    multiple k of G2::one() it handed out itself, so e(P, k G2) = e(k P, G2) and a product is one iff the sum of k_i P_i is zero."""
    def __init__(self):
        self.calls = []
        self.g2_log = {}

    def _k(self, row):
        return self.g2_log[np.asarray(row, np.uint64).tobytes()]

    def g1_hash_to_curve_batch(self, msgs, dst):
        msgs = np.asarray(msgs, np.uint8)
        self.calls.append(("g1_hash_to_curve_batch", msgs.shape))
        return np.stack([HC.words(HC.hash_to_curve(m.tobytes(), dst)) for m in msgs])

    def g1_hash_to_curve_uniform_batch(self, uniform):
        uniform = np.asarray(uniform, np.uint8).reshape(-1, 96)
        self.calls.append(("g1_hash_to_curve_uniform_batch", uniform.shape[0]))
        return np.stack([HC.words(HC.hash_uniform(u.tobytes())) for u in uniform])

    def g1_map_to_curve_batch(self, u):
        u = np.asarray(u, np.uint8).reshape(-1, 48)
        self.calls.append(("g1_map_to_curve_batch", u.shape[0]))
        return np.stack([HC.words(HC.map_to_curve(int.from_bytes(r.tobytes(), "big"))) for r in u]) if u.shape[0] else np.zeros((0, 12), np.uint64)

    def g2_mul_base_batch(self, base, k):
        from bn_amd import G2
        assert np.array_equal(np.asarray(base).reshape(-1), G2.one().limbs)
        self.calls.append(("g2_mul_base_batch", len(k)))
        out = []
        for row in np.asarray(k, np.uint64).reshape(-1, 4):
            w = _g2_words(M.g_normalize(M.FQ2_OPS, M.g_mul(M.FQ2_OPS, M.G2_ONE, _scalar(row))))
            self.g2_log[w.tobytes()] = _scalar(row)
            out.append(w)
        return np.stack(out)

    def g1_mul_batch(self, p, k):
        self.calls.append(("g1_mul_batch", len(p)))
        return np.stack([_g1_words(M.g_normalize(O, M.g_mul(O, _g1(a), _scalar(b)))) for a, b in zip(np.asarray(p), np.asarray(k))])

    def g1_add_batch(self, a, b, negate_b=False):
        self.calls.append(("g1_add_batch", len(a), bool(negate_b)))
        return np.stack([_g1_words(M.g_add(O, _g1(x), M.g_neg(O, _g1(y)) if negate_b else _g1(y))) for x, y in zip(np.asarray(a), np.asarray(b))])

    def g1_msm(self, p, k):
        self.calls.append(("g1_msm", len(p)))
        acc = M.g_zero(O)
        for a, b in zip(np.asarray(p), np.asarray(k)):
            acc = M.g_add(O, acc, M.g_mul(O, _g1(a), _scalar(b)))
        return _g1_words(M.g_normalize(O, acc))

    def g2_msm(self, p, k):
        self.calls.append(("g2_msm", len(p)))
        assert all(_scalar(b) == 1 for b in np.asarray(k))
        total = sum(self._k(a) for a in np.asarray(p)) % R
        w = _g2_words(M.g_normalize(M.FQ2_OPS, M.g_mul(M.FQ2_OPS, M.G2_ONE, total)))
        self.g2_log[w.tobytes()] = total
        return w

    def _product_is_one(self, P, Q):
        from bn_amd import G2
        self.g2_log.setdefault(G2.one().limbs.tobytes(), 1)
        acc = M.g_zero(O)
        for a, b in zip(P, Q):
            acc = M.g_add(O, acc, M.g_mul(O, _g1(a), self._k(b)))
        return M.g_is_zero(O, acc)

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


def test_api_routes_equal_and_mixed_lengths_to_the_same_bytes():
    import bn_amd
    m = Model()
    same = [b"abcd", b"efgh", b"ijkl"]
    got = bn_amd.g1_hash_to_curve_batch(same, b"tag", engine=m)
    assert m.calls == [("g1_hash_to_curve_batch", (3, 4))]                       # one length: the device's SHA-256
    assert all(isinstance(p, bn_amd.G1) and np.array_equal(p.limbs, HC.words(HC.hash_to_curve(s, b"tag"))) for p, s in zip(got, same))
    m.calls.clear()
    mixed = [b"", b"a", b"abcd"]
    got = bn_amd.g1_hash_to_curve_batch(mixed, b"tag", engine=m)
    assert m.calls == [("g1_hash_to_curve_uniform_batch", 3)]                    # mixed lengths: hashlib, then the uniform call
    assert all(np.array_equal(p.limbs, HC.words(HC.hash_to_curve(s, b"tag"))) for p, s in zip(got, mixed))
    assert np.array_equal(got[2].limbs, bn_amd.g1_hash_to_curve_batch([b"abcd"], b"tag", engine=m)[0].limbs)          # the same bytes either way
    m.calls.clear()
    arr = HC.messages(2, 0)
    assert len(bn_amd.g1_hash_to_curve_batch(arr, b"tag", engine=m)) == 2 and m.calls == [("g1_hash_to_curve_batch", (2, 0))]
    m.calls.clear()
    pts = bn_amd.g1_map_to_curve_batch([0, 2, 3, (1 << 384) - 1], engine=m)
    assert m.calls == [("g1_map_to_curve_batch", 4)] and np.array_equal(pts[3].limbs, HC.words(HC.map_to_curve((1 << 384) - 1)))
    assert bn_amd.g1_map_to_curve_batch([], engine=m) == []


def test_errors_raise_before_any_device_call():
    import bn_amd
    from bn_amd import bls
    nd = NoDevice()
    for dst in (b"", b"x" * 256):
        with pytest.raises(ValueError, match="1 .. 255 bytes"):
            bn_amd.g1_hash_to_curve_batch([b"m"], dst, engine=nd)
    with pytest.raises(ValueError, match=r"\(n, msg_len\) uint8"):
        bn_amd.g1_hash_to_curve_batch(np.zeros(5, np.uint8), b"tag", engine=nd)
    with pytest.raises(OverflowError):
        bn_amd.g1_map_to_curve_batch([1 << 384], engine=nd)
    one = bn_amd.G1.one(); two = bn_amd.G2.one()
    with pytest.raises(ValueError, match="distinct messages"):
        bls.verify_aggregate([two, two, two], [b"a", b"b", b"a"], one, engine=nd)
    with pytest.raises(ValueError, match="distinct messages"):
        bls.verify_aggregate([two, two], np.zeros((2, 8), np.uint8), one, engine=nd)
    with pytest.raises(ValueError, match="as many public keys as messages"):
        bls.verify_aggregate([two], [b"a", b"b"], one, engine=nd)
    with pytest.raises(ValueError, match="as many messages as secret keys"):
        bls.sign_batch([bn_amd.Fr(1)], [b"a", b"b"], engine=nd)
    with pytest.raises(ValueError, match="as many public keys and signatures as messages"):
        bls.verify_batch([two], [b"a"], [one, one], engine=nd)
    assert bls.sign_batch([], [], engine=nd) == [] and bls.verify_batch([], [], [], engine=nd).shape == (0,)
    assert bls.verify_aggregate([], [], one, engine=nd) is False and bls.fast_aggregate_verify([], b"m", one, engine=nd) is False


def test_bls_over_the_stand_in_engine_makes_the_calls_it_promises():
    from bn_amd import Fr, G1, bls
    m = Model()
    sks = [Fr(11 + 7 * i) for i in range(5)]
    pks = bls.public_keys(sks, engine=m)
    assert m.calls == [("g2_mul_base_batch", 5)]
    msgs = [bytes([i]) * 8 for i in range(5)]
    m.calls.clear()
    sigs = bls.sign_batch(sks, msgs, engine=m)
    assert m.calls == [("g1_hash_to_curve_batch", (5, 8)), ("g1_mul_batch", 5)]
    for sk, msg, sig in zip(sks, msgs, sigs):
        h = HC.hash_to_curve(msg, bls.DST)
        assert np.array_equal(sig.limbs, _g1_words(M.g_normalize(O, M.g_mul(O, (h[0], h[1], 1), sk.v))))
    assert np.array_equal(bls.sign(sks[2], msgs[2], engine=m).limbs, sigs[2].limbs)
    m.calls.clear()
    ok = bls.verify_batch(pks, msgs, sigs, engine=m)
    assert m.calls == [("g1_hash_to_curve_batch", (5, 8)), ("g1_add_batch", 5, True), ("pairing_product_batch", 5, [2])]
    assert ok.dtype == bool and ok.all()
    spoiled = list(sigs); spoiled[3] = sigs[1]
    assert bls.verify_batch(pks, msgs, spoiled, engine=m).tolist() == [True, True, True, False, True]
    assert bls.verify(pks[0], msgs[0], sigs[0], engine=m) is True and bls.verify(pks[1], msgs[0], sigs[0], engine=m) is False
    assert bls.verify(pks[0], msgs[0], sigs[0], dst=b"another tag", engine=m) is False
    m.calls.clear()
    mixed = [b"", b"a", b"bb", b"ccc", b"dddd"]
    assert bls.verify_batch(pks, mixed, bls.sign_batch(sks, mixed, engine=m), engine=m).all()
    assert [c[0] for c in m.calls] == ["g1_hash_to_curve_uniform_batch", "g1_mul_batch", "g1_hash_to_curve_uniform_batch", "g1_add_batch", "pairing_product_batch"]
    m.calls.clear()
    agg = bls.aggregate(sigs, engine=m)
    assert m.calls == [("g1_msm", 5)]
    m.calls.clear()
    assert bls.verify_aggregate(pks, msgs, agg, engine=m) is True
    assert m.calls == [("g1_hash_to_curve_batch", (5, 8)), ("pairing_product", 6)]
    assert bls.verify_aggregate(pks, msgs[1:] + msgs[:1], agg, engine=m) is False
    assert bls.verify_aggregate(pks[:4], msgs[:4], agg, engine=m) is False
    one = b"one message"
    same = bls.aggregate(bls.sign_batch(sks, [one] * 5, engine=m), engine=m)
    m.calls.clear()
    assert bls.fast_aggregate_verify(pks, one, same, engine=m) is True
    assert m.calls == [("g2_msm", 5), ("g1_hash_to_curve_batch", (1, len(one))), ("pairing_product", 2)]
    assert bls.fast_aggregate_verify(pks[:4], one, same, engine=m) is False
    assert bls.fast_aggregate_verify(pks, one, G1.zero(), engine=m) is False


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read
TAG = b"tag"


def test_argument_errors_answer_without_a_device(lib):
    assert lib.bn254_g1_map_to_curve_batch(None, None, DUMMY, 1) == BAD_ARG and lib.bn254_g1_map_to_curve_batch(None, DUMMY, None, 1) == BAD_ARG
    assert lib.bn254_g1_hash_to_curve_uniform_batch(None, None, DUMMY, 1) == BAD_ARG and lib.bn254_g1_hash_to_curve_uniform_batch(None, DUMMY, None, 1) == BAD_ARG
    assert lib.bn254_g1_map_to_curve_batch_dev(None, None, DUMMY, 1, None) == BAD_ARG and lib.bn254_g1_map_to_curve_batch_dev(None, DUMMY, None, 1, None) == BAD_ARG
    assert lib.bn254_g1_hash_to_curve_uniform_batch_dev(None, None, DUMMY, 1, None) == BAD_ARG and lib.bn254_g1_hash_to_curve_uniform_batch_dev(None, DUMMY, None, 1, None) == BAD_ARG
    for n in ((1 << 40) + 1,):
        assert lib.bn254_g1_map_to_curve_batch(None, DUMMY, DUMMY, n) == BAD_ARG and lib.bn254_g1_hash_to_curve_uniform_batch_dev(None, DUMMY, DUMMY, n, None) == BAD_ARG
    cases = [("a NULL tag", DUMMY, 4, None, 3, DUMMY, 1), ("an empty tag", DUMMY, 4, TAG, 0, DUMMY, 1), ("a tag of 256 bytes", DUMMY, 4, b"x" * 256, 256, DUMMY, 1),
             ("an empty tag without work", DUMMY, 4, TAG, 0, DUMMY, 0), ("NULL messages of 4 bytes", None, 4, TAG, 3, DUMMY, 1), ("a NULL output", DUMMY, 4, TAG, 3, None, 1),
             ("a NULL output for empty messages", None, 0, TAG, 3, None, 1), ("messages above 2^20 bytes", DUMMY, (1 << 20) + 1, TAG, 3, DUMMY, 1),
             ("n above 2^40", DUMMY, 0, TAG, 3, DUMMY, (1 << 40) + 1), ("n * msg_len above 2^40", DUMMY, 1 << 20, TAG, 3, DUMMY, (1 << 20) + 1)]
    for what, msgs, ml, dst, dl, out, n in cases:
        assert lib.bn254_g1_hash_to_curve_batch(None, msgs, ml, dst, dl, out, n) == BAD_ARG, what
        assert lib.bn254_g1_hash_to_curve_batch_dev(None, msgs, ml, dst, dl, out, n, None) == BAD_ARG, what


def test_no_work_is_ok(lib):
    assert lib.bn254_g1_map_to_curve_batch(None, None, None, 0) == 0 and lib.bn254_g1_map_to_curve_batch_dev(None, None, None, 0, None) == 0
    assert lib.bn254_g1_hash_to_curve_uniform_batch(None, None, None, 0) == 0 and lib.bn254_g1_hash_to_curve_uniform_batch_dev(None, None, None, 0, None) == 0
    assert lib.bn254_g1_hash_to_curve_batch(None, None, 32, TAG, 3, None, 0) == 0 and lib.bn254_g1_hash_to_curve_batch_dev(None, None, 32, TAG, 3, None, 0, None) == 0
    assert lib.bn254_g1_hash_to_curve_batch(None, None, 0, None, 3, None, 0) == 0


def test_the_hooks_check_their_bounds(lib):
    try:
        assert lib.bn254_hash_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_hash_set_launch_max(64) == 0
    finally:
        assert lib.bn254_hash_set_launch_max(0) == 0
    assert lib.bn254_hash_inv0_form() in (0, 1)
    ops = (ROOT / "bn_amd" / "csrc" / "hash_ops.hpp").read_text()
    assert re.search(r"^#define BN254_H2C_INV0 %d\b" % lib.bn254_hash_inv0_form(), ops, re.M)            # the default of the source is what was built


def test_the_kernels_are_instances_of_bn254_fr_decode_k_without_spill_or_lds():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    import lane_shell
    src = lane_shell.unit_source("bn254_hash.hip")  # the unit adds no kernel under a new name: the shell is lane_launch.hpp's
    assert "__shared__" not in src and "__shared__" not in (ROOT / "bn_amd" / "csrc" / "hash_ops.hpp").read_text()
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    meta = kernel_meta.instances(so)
    for op in OPS:
        mine = [n for n in meta if re.search(r"\d+" + op + r"(E|I)", n)]
        assert len(mine) == 1, (op, mine)
        assert kernel_meta.short_name(mine[0]) == "bn254_fr_decode_k", mine
        assert meta[mine[0]]["spill"] == 0 == SPILL_CEILING["bn254_fr_decode_k"], (mine[0], meta[mine[0]])
        assert meta[mine[0]]["lds"] == 0, (mine[0], meta[mine[0]])
