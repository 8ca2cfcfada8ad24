"""Grumpkin (bn254_grumpkin_{validate,add,mul,msm}_batch and their _dev twins) without a GPU: the eight symbols and their declarations in every
layer that mirrors the C header, the argument checks that answer before any device is touched, the documented status numbers, the Python
surface - bn_amd.grumpkin, bn_amd.pedersen and bn_amd.ipa - over a stand-in engine that answers from the integer model of grumpkin_cases.py,
and the register budget of the kernels: template instances of bn254_fr_decode_k<Op> only."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import fr_cases as FC
import grumpkin_cases as GC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST, MUT = ("const",), ("mut",)
CTX, N, STATUS, FR_IN, FR_OUT, K_IN, OFFS, D_IN, D_OUT = ("void", MUT), ("usize", ()), ("i32", MUT), ("fr", CONST), ("fr", MUT), ("u8", CONST), ("usize", CONST), ("void", CONST), ("void", MUT)
EXPECTED = {
    "bn254_grumpkin_validate_batch": [CTX, FR_IN, STATUS, N],
    "bn254_grumpkin_add_batch": [CTX, FR_IN, FR_IN, FR_OUT, N],
    "bn254_grumpkin_mul_batch": [CTX, FR_IN, K_IN, FR_OUT, N],
    "bn254_grumpkin_msm_batch": [CTX, FR_IN, K_IN, OFFS, N, FR_OUT],
    "bn254_grumpkin_validate_batch_dev": [CTX, D_IN, D_OUT, N, D_OUT],
    "bn254_grumpkin_add_batch_dev": [CTX, D_IN, D_IN, D_OUT, N, D_OUT],
    "bn254_grumpkin_mul_batch_dev": [CTX, D_IN, D_IN, D_OUT, N, D_OUT],
    "bn254_grumpkin_msm_batch_dev": [CTX, D_IN, D_IN, OFFS, N, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
LANE = NAMES[:3]                                     # one record per lane: (ctx, pointers.., n)
HOOKS = ("bn254_grumpkin_set_launch_max", "bn254_grumpkin_window")
SCOPES = ("grumpkin_validate", "grumpkin_add", "grumpkin_mul", "grumpkin_msm", "grumpkin_msm_fold")
OPS = ("GrkValidateOp", "GrkAddOp", "GrkMulOp", "GrkMsmOp", "GrkMsmFoldOp")
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_grumpkin_set_launch_max.argtypes = [C.c_size_t]
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
    assert any(s.name == "bn254_grumpkin.hip" for s in _native.SOURCES)
    assert raw.bn254_grumpkin_window() == 4


def test_header_declares_the_eight_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
    hdr = B.HEADER.read_text()
    assert hdr.index("int bn254_eddsa_poseidon_verify_packed_batch_dev(") < hdr.index("/* Grumpkin, one record per lane") < hdr.index("int bn254_grumpkin_validate_batch(") < hdr.index("/* ---- device-resident entry points")
    own = " ".join(hdr[hdr.index("/* Grumpkin, one record per lane"):hdr.index("int bn254_grumpkin_validate_batch(")].split())
    for word in ("y^2 = x^3 - 17", "whose order is q", "cofactor is 1", str(GC.G[1]), "two consecutive bn_fr, x then y", "Infinity is (0, 0)", "non-residue",
                 "little-endian integer k", "Any value below 2^256", "[k mod q]P", "NOT a Montgomery image", "no Fq type", "as they stand, before any field arithmetic",
                 "O = (0, 0) is one", "no subgroup status", "Renes-Costello-Batina", "out may be p or q", "never a fault", "out may be p.", "all 256 bits",
                 "HOST array of m + 1 size_t", "An empty segment", "must not overlap", "at most 16 partial sums", "n > 2^40", "BN254_E_BAD_ARG", "do not start at 0",
                 "n == 0 (m == 0) succeeds", "at most 2^22 records", "read nothing back"):
        assert word in own, word
    assert [int(x) for x in re.findall(r"(?:^| )(\d) (?=a coordinate is|y\^2 != x\^3|otherwise: a point)", own)] == [1, 4, 0]
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for text in (semantics, threading):
        for name in NAMES:
            assert name in text, name
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    mine = [l for l in block.split("\n") if '"grumpkin_validate"' in l]
    assert len(mine) == 1 and re.findall(r'"(\w+)"', mine[0]) == list(SCOPES)                   # a line of its own
    src = (ROOT / "bn_amd" / "csrc" / "bn254_grumpkin.hip").read_text()
    assert set(SCOPES) <= set(re.findall(r'"(\w+)"', src))


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(_native.SIGNATURES) == set(B.c_declarations())
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    for fn in ("pub fn grumpkin_validate_batch(p: &[Fr]) -> Result<Vec<i32>, GpuError>", "pub fn grumpkin_add_batch(p: &[Fr], q: &[Fr]) -> Result<Vec<Fr>, GpuError>",
               "pub fn grumpkin_mul_batch(p: &[Fr], k32: &[u8]) -> Result<Vec<Fr>, GpuError>",
               "pub fn grumpkin_msm_batch(p: &[Fr], k32: &[u8], offsets: &[usize]) -> Result<Vec<Fr>, GpuError>"):
        assert fn in txt, fn
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<int32_t> grumpkin_validate(", "std::vector<Fr> grumpkin_add(", "std::vector<Fr> grumpkin_mul(", "std::vector<Fr> grumpkin_msm(") + NAMES[:4]:
        assert s + ("(" if s.startswith("bn254_") else "") in hpp, s
    variant = (ROOT / "tools" / "build_variant.sh").read_text()
    assert re.search(r"^for u in .*\bbn254_grumpkin\b.*; do$", variant, re.M)
    switches = set()
    for f in ("grumpkin_ops.hpp", "grumpkin_constants.hpp", "bn254_grumpkin.hip"):
        switches |= set(re.findall(r"^#\s*if(?:n?def|\s+!?defined\()\s*(\w+)", (ROOT / "bn_amd" / "csrc" / f).read_text(), re.M))
    assert all(s.startswith("BN254_") for s in switches), switches                              # BN_* is a pinned set (test_build_quality.py)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        for name in NAMES[:4] + ("Grumpkin", "NOT Barretenberg's"):
            assert name in text, (doc, name)
    readme = (ROOT / "README.md").read_text()
    assert "profiles/r30_grumpkin.txt" in readme and "No speed is promised" in readme and (ROOT / "tools" / "time_grumpkin.py").exists()
    section = " ".join(readme[readme.index("**Grumpkin, BN254's cycle curve"):].split())
    for word in ("GLV", "signed digits", "bucket-method MSM", "fixed-base", "compressed points", "`Fq` type", "Barretenberg-compatible generators", "multi-GPU"):
        assert word in section, word


def test_python_surface():
    import bn_amd
    from bn_amd import engine, grumpkin, ipa, pedersen
    E = engine.Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.grumpkin_validate_batch) == ["self", "p"] and sig(E.grumpkin_add_batch) == ["self", "p", "q"] and sig(E.grumpkin_mul_batch) == ["self", "p", "k"]
    assert sig(E.grumpkin_msm_batch) == ["self", "p", "k", "offsets"]
    assert sig(E.grumpkin_validate_batch_dev) == ["self", "d_p", "d_status", "n", "stream"] and sig(E.grumpkin_mul_batch_dev) == ["self", "d_p", "d_k", "d_out", "n", "stream"]
    assert sig(E.grumpkin_add_batch_dev) == ["self", "d_p", "d_q", "d_out", "n", "stream"]
    assert sig(E.grumpkin_msm_batch_dev) == ["self", "d_p", "d_k", "offsets", "m", "d_out", "stream"]
    for name in ("grumpkin_validate_batch", "grumpkin_add_batch", "grumpkin_mul_batch", "grumpkin_msm_batch"):
        assert getattr(bn_amd, name) is getattr(bn_amd.api, name) and "engine" in sig(getattr(bn_amd, name))
    for name in ("Q", "R", "B", "G", "on_curve_host", "add_host", "neg_host", "mul_host", "Point", "msm", "point_limbs", "scalar_rows"):
        assert hasattr(grumpkin, name), name
    assert grumpkin.B == -17 and grumpkin.Q == GC.Q and grumpkin.R == GC.R
    for name in ("generators", "commit", "commit_batch"):
        assert hasattr(pedersen, name), name
    assert sig(pedersen.commit)[:4] == ["gens", "values", "blind", "h"] and sig(ipa.prove)[:5] == ["gens", "u", "a", "b", "transcript"]
    assert sig(ipa.verify)[:5] == ["gens", "u", "commitment", "proof", "transcript"] and ipa.Proof._fields == ("L", "R", "a_final", "b_final")
    assert "NOT Barretenberg's" in pedersen.__doc__ and "THIS PROJECT'S OWN" in ipa.__doc__
    from bn_amd import sumcheck
    assert issubclass(ipa.Transcript, sumcheck.Transcript)


# ------------------------------------------------------------------------------------------------------------------ a stand-in engine
class Model:
    """the four calls answered from the integer model; counts them"""
    def __init__(self):
        self.calls = []

    @staticmethod
    def _ints(a):
        a = np.asarray(a, np.uint64).reshape(-1, 4)
        return [sum(int(x) << (64 * i) for i, x in enumerate(r)) for r in a]

    def _pts(self, p):
        inv = pow(FC.MONT, -1, GC.R)
        v = [w * inv % GC.R if w < GC.R else w for w in self._ints(p)]           # words that are not below r stay what they are
        return list(zip(v[0::2], v[1::2]))

    def grumpkin_validate_batch(self, p):
        self.calls.append(("validate", len(p)))
        return np.array([GC.validate_status(*q) for q in self._pts(p)], np.int32)

    def grumpkin_add_batch(self, p, q):
        self.calls.append(("add", len(p)))
        return GC.point_rows([GC.add(a, b) for a, b in zip(self._pts(p), self._pts(q))])

    def grumpkin_mul_batch(self, p, k):
        self.calls.append(("mul", len(p)))
        return GC.point_rows([GC.mul(a, b) for a, b in zip(self._pts(p), self._ints(k))])

    def grumpkin_msm_batch(self, p, k, offsets):
        o = [int(x) for x in offsets]
        self.calls.append(("msm", len(p), len(o) - 1))
        pts, ks = self._pts(p), self._ints(k)
        return GC.point_rows([GC.msm(pts[a:b], ks[a:b]) for a, b in zip(o, o[1:])]).reshape(len(o) - 1, 2, 4)


def test_the_package_over_the_model_makes_the_calls_it_promises():
    import bn_amd
    from bn_amd import grumpkin as GK, ipa, pedersen
    m = Model()
    G = GK.Point.generator()
    assert bn_amd.grumpkin_mul_batch([G, G], [3, GC.Q + 3], engine=m) == [GK.Point(*GC.mul(GC.G, 3))] * 2 and m.calls == [("mul", 2)]
    assert bn_amd.grumpkin_add_batch([G], [GK.Point.identity()], engine=m) == [G]
    assert bn_amd.grumpkin_validate_batch(GC.point_rows([GC.G, (GC.R, 1), GC.OFF_CURVE, GC.O]), engine=m).tolist() == [0, 1, 4, 0]
    m.calls.clear()
    assert GK.msm([G, G], [2, 3], engine=m) == GK.Point(*GC.mul(GC.G, 5)) and m.calls == [("msm", 2, 1)]
    with pytest.raises(ValueError):
        bn_amd.grumpkin_mul_batch([G], [1, 2], engine=m)
    with pytest.raises(ValueError):
        bn_amd.grumpkin_mul_batch([G], [-1], engine=m)
    # Pedersen: one call each
    gens = pedersen.generators(4, "abi")
    m.calls.clear()
    c = pedersen.commit(gens, [1, 2, 3], blind=4, engine=m)
    assert c == pedersen.commit_host(gens, [1, 2, 3], blind=4) and m.calls == [("msm", 4, 1)]
    m.calls.clear()
    cs = pedersen.commit_batch(gens, [[1, 2], [3, 4], [5, 6]], engine=m)
    assert cs == [pedersen.commit_host(gens, v) for v in ([1, 2], [3, 4], [5, 6])] and m.calls == [("msm", 6, 3)]
    # the inner-product argument at n = 4 and n = 1: accepted; tampered: rejected; the calls per round as documented
    u = pedersen.generators(1, "abi.u")[0]
    for n in (4, 1):
        a, b = [5, GC.Q - 1, 7, 11][:n], [2, 3, GC.Q - 5, 1][:n]
        m.calls.clear()
        proof = ipa.prove(gens[:n], u, a, b, ipa.Transcript("abi"), engine=m)
        k = n.bit_length() - 1
        want = [("msm", n + 1, 1)]
        for j in range(k):
            h = n >> (j + 1)
            want += [("msm", 2 * h + 2, 2), ("msm", 2 * h, h)]
        assert m.calls == want
        C_ = ipa.commitment(gens[:n], u, a, b, engine=m)
        m.calls.clear()
        assert ipa.verify(gens[:n], u, C_, proof, ipa.Transcript("abi"), engine=m) is True and m.calls == [("msm", n, 1), ("msm", 2 * k + 3, 2)]
        assert ipa.verify(gens[:n], u, C_, proof, ipa.Transcript("abi"), b=b, engine=m) is True
        assert ipa.verify(gens[:n], u, C_, proof._replace(a_final=(proof.a_final + 1) % GC.Q), ipa.Transcript("abi"), engine=m) is False
        if k:
            assert ipa.verify(gens[:n], u, C_, proof._replace(L=[G] + proof.L[1:]), ipa.Transcript("abi"), engine=m) is False
            assert ipa.verify(gens[:n], u, C_, proof, ipa.Transcript("abi2"), engine=m) is False


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


def test_argument_errors_answer_without_a_device(lib):
    for name in LANE:
        f, fd = getattr(lib, name), getattr(lib, name + "_dev")
        k = len(EXPECTED[name]) - 2                                  # pointer arguments behind ctx
        for null in range(k):
            args = [None if j == null else DUMMY for j in range(k)]
            assert f(None, *args, 1) == BAD_ARG, (name, null)
            assert fd(None, *args, 1, None) == BAD_ARG, (name, null)
        assert f(None, *[DUMMY] * k, (1 << 40) + 1) == BAD_ARG and fd(None, *[DUMMY] * k, (1 << 40) + 1, None) == BAD_ARG, name
    f, fd = lib.bn254_grumpkin_msm_batch, lib.bn254_grumpkin_msm_batch_dev
    offs = lambda *v: np.array(v, np.uint64)
    ok, not0, down, big = offs(0, 2, 3), offs(1, 2, 3), offs(0, 3, 2), offs(0, (1 << 40) + 1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for g, tail in ((f, ()), (fd, (None,))):
        assert g(None, None, DUMMY, p(ok), 2, DUMMY, *tail) == BAD_ARG and g(None, DUMMY, None, p(ok), 2, DUMMY, *tail) == BAD_ARG
        assert g(None, DUMMY, DUMMY, None, 2, DUMMY, *tail) == BAD_ARG and g(None, DUMMY, DUMMY, p(ok), 2, None, *tail) == BAD_ARG
        assert g(None, DUMMY, DUMMY, p(not0), 2, DUMMY, *tail) == BAD_ARG                          # offsets[0] != 0
        assert g(None, DUMMY, DUMMY, p(down), 2, DUMMY, *tail) == BAD_ARG                          # decreasing
        assert g(None, DUMMY, DUMMY, p(big), 1, DUMMY, *tail) == BAD_ARG                           # more than 2^40 terms


def test_no_work_is_ok(lib):
    for name in LANE:
        k = len(EXPECTED[name]) - 2
        assert getattr(lib, name)(None, *[None] * k, 0) == 0 and getattr(lib, name + "_dev")(None, *[None] * k, 0, None) == 0, name
    assert lib.bn254_grumpkin_msm_batch(None, None, None, None, 0, None) == 0 and lib.bn254_grumpkin_msm_batch_dev(None, None, None, None, 0, None, None) == 0


def test_the_hook_checks_its_bounds(lib):
    try:
        assert lib.bn254_grumpkin_set_launch_max((1 << 22) + 1) == BAD_ARG and lib.bn254_grumpkin_set_launch_max(64) == 0
    finally:
        assert lib.bn254_grumpkin_set_launch_max(0) == 0


def test_the_status_numbers_are_as_documented():
    from bn_amd import grumpkin
    assert (GC.ST_OK, GC.ST_RANGE, GC.ST_CURVE) == (0, 1, 4) and set(grumpkin.STATUS) == {0, 1, 4}
    ops = (ROOT / "bn_amd" / "csrc" / "grumpkin_ops.hpp").read_text()
    assert "status[i] = !in_range ? 1 : !on_curve ? 4 : 0;" in ops
    wire = (ROOT / "bn_amd" / "csrc" / "io_wire.hpp").read_text()
    taken = {int(x) for x in re.findall(r"WIRE_\w+ = (\d+)", wire)}
    assert {1, 4} <= taken, taken                                                                # 1 and 4 keep the wire format's meaning


def test_the_kernels_are_instances_of_bn254_fr_decode_k_without_spill_or_lds():
    import isa_mix
    import kernel_meta
    import lane_shell
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    src = lane_shell.unit_source("bn254_grumpkin.hip")    # the unit adds no kernel under a new name: the shell is lane_launch.hpp's
    assert "__global__" not in src
    for text in (src, (ROOT / "bn_amd" / "csrc" / "grumpkin_ops.hpp").read_text()):
        assert "__shared__" not in text and "atomic" not in text.lower()
    assert so.exists() and (isa_mix.LLVM / "llvm-readelf").exists()
    meta = kernel_meta.instances(so)
    for op in OPS:
        mine = [n for n in meta if re.search(r"\d+" + op + r"(E|I)", n)]
        assert len(mine) == 1, (op, mine)
        assert kernel_meta.short_name(mine[0]) == "bn254_fr_decode_k", mine
        assert meta[mine[0]]["spill"] == 0 == SPILL_CEILING["bn254_fr_decode_k"], (mine[0], meta[mine[0]])
        assert meta[mine[0]]["lds"] == 0, (mine[0], meta[mine[0]])
