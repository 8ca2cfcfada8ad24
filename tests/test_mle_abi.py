"""Multilinear tables and sumcheck rounds over Fr (bn254_fr_mle_eq, bn254_fr_mle_fold, bn254_fr_sumcheck_round and their _dev twins), bn_amd.mle
and bn_amd.sumcheck, without a GPU: the six declarations in every layer that mirrors the C header, the argument checks that answer before
any device is touched, the profiling scopes, the Python surface and its errors, the test hooks, the two first users over a stand-in engine
that answers from the integer model, and the register budget of the device code - the kernels are template instances of an existing kernel
name (bn254_fr_decode_k<Op>)."""
import ctypes as C
import inspect
import pathlib
import re
import sys

import numpy as np
import pytest

import fr_cases as FC
import mle_cases as MC
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

CONST = ("const",)
MUT = ("mut",)
CTX, FR_IN, FR_OUT, N, INT = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ()), ("int", ())
D_IN, D_OUT, OFF, U64 = ("void", CONST), ("void", MUT), ("usize", CONST), ("u64", CONST)
EXPECTED = {
    "bn254_fr_mle_eq": [CTX, FR_IN, INT, FR_OUT],
    "bn254_fr_mle_eq_dev": [CTX, D_IN, INT, D_OUT, D_OUT],
    "bn254_fr_mle_fold": [CTX, FR_IN, N, FR_IN, FR_OUT],
    "bn254_fr_mle_fold_dev": [CTX, D_IN, N, FR_IN, D_OUT, D_OUT],
    "bn254_fr_sumcheck_round": [CTX, FR_IN, N, N, OFF, U64, FR_IN, N, INT, FR_OUT],
    "bn254_fr_sumcheck_round_dev": [CTX, D_IN, N, N, OFF, U64, FR_IN, N, INT, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPES = ("fr_mle_eq", "fr_mle_fold", "fr_sumcheck_round", "fr_sumcheck_sum")
HOOKS = ("bn254_fr_sumcheck_piece", "bn254_fr_sumcheck_fan", "bn254_fr_mle_set_launch_max", "bn254_fr_sumcheck_set_piece")
LIMITS = {"MLE_VARS_MAX": 30, "SUMCHECK_DEGREE_MAX": 4, "SUMCHECK_TABLES_MAX": 16, "SUMCHECK_GROUPS_MAX": 16}
BAD_ARG = -2
R = FC.R


def test_header_declares_the_six_entry_points_and_the_limits():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
        assert decls[name]["params"][-1][0] == ("stream" if name.endswith("_dev") else "out")
    hdr = B.HEADER.read_text()
    for name, value in LIMITS.items():
        assert re.search(r"^#define BN254_%s %d$" % (name, value), hdr, re.M), name
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    for name in NAMES:
        assert name in semantics, name
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    assert "bn254_fr_mle_eq, bn254_fr_mle_fold and bn254_fr_sumcheck_round serialise on the context" in threading
    for name in NAMES:
        if name.endswith("_dev"):
            assert name in threading, name
    own = " ".join(hdr[hdr.index("Multilinear tables and sumcheck rounds over Fr"):hdr.index("#define BN254_MLE_VARS_MAX")].split())
    for word in ("bit j of i", "MOST significant", "index-major", "tables[i * k + j]", "point[j] = challenge[nv - 1 - j]", "out[i] = in[i] + r * (in[i + len/2] - in[i])",
                 "Fr::one()", "HOST", "`out` may be exactly `in`", "an odd len", "t * (T_j[i + h] - T_j[i])", "degree + 1", "need not be a power of two", "canonical",
                 "BN254_E_BAD_ARG", "n k > 2^40", "No atomics", "Threading"):
        assert word in own, word
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook


def test_the_scope_names_are_documented_and_used():
    hdr = B.HEADER.read_text()
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    lines = block.split("\n")
    mine = [i for i, l in enumerate(lines) if '"fr_mle_eq"' in l]
    ntt = [i for i, l in enumerate(lines) if '"ntt"' in l]
    assert len(mine) == 1 and len(ntt) == 1 and 0 < mine[0] < ntt[0]
    assert re.findall(r'"(\w+)"', lines[mine[0]]) == list(SCOPES)                               # a line of their own
    names = re.findall(r'"(\w+)"', block)
    assert tuple(names[-2:]) == ("ntt", "ntt_table") and len(names) == len(set(names))
    src = (ROOT / "bn_amd" / "csrc" / "bn254_mle.hip").read_text()
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
    for fn in ("pub fn fr_mle_eq(z: &[Fr]) -> Result<Vec<Fr>, GpuError>", "pub fn fr_mle_fold(a: &[Fr], r: &Fr) -> Result<Vec<Fr>, GpuError>",
               "pub fn fr_sumcheck_round(tables: &[Fr], k: usize, group_offsets: &[usize], group_tables: &[u64], group_coeff: &[Fr], degree: usize) -> Result<Vec<Fr>, GpuError>"):
        assert fn in txt, fn
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    assert B.compare(B.c_declarations(), md, "INTEGRATION.md") == []
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    for s in ("std::vector<Fr> fr_mle_eq(", "std::vector<Fr> fr_mle_fold(", "std::vector<Fr> fr_sumcheck_round(", "bn254_fr_mle_eq(", "bn254_fr_mle_fold(", "bn254_fr_sumcheck_round("):
        assert s in hpp, s
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        for name in ("bn254_fr_mle_eq", "bn254_fr_mle_fold", "bn254_fr_sumcheck_round"):
            assert name in text, (doc, name)
    assert "bn254_mle.hip" in [s.name for s in _native.SOURCES]
    assert (ROOT / "bn_amd" / "csrc" / "mle_ops.hpp").exists()
    assert " bn254_mle" in (ROOT / "tools" / "build_variant.sh").read_text()
    readme = (ROOT / "README.md").read_text()
    assert "profiles/r17_mle.txt" in readme and (ROOT / "profiles" / "r17_mle.txt").exists() and (ROOT / "tools" / "time_mle.py").exists()
    for doc in (readme, inspect.getdoc(__import__("bn_amd").sumcheck)):
        assert "fused fold-then-round" in doc and "factored" in doc                            # the "not built" list


def test_python_surface():
    import bn_amd
    from bn_amd import engine, mle, sumcheck
    assert list(inspect.signature(bn_amd.fr_mle_eq).parameters) == ["z", "engine"]
    assert list(inspect.signature(bn_amd.fr_mle_fold).parameters) == ["a", "r", "engine"]
    sig = inspect.signature(bn_amd.fr_sumcheck_round)
    assert list(sig.parameters) == ["tables", "groups", "degree", "engine"] and sig.parameters["degree"].default is None
    E = engine.Engine
    assert list(inspect.signature(E.fr_mle_eq).parameters) == ["self", "z"]
    assert list(inspect.signature(E.fr_mle_fold).parameters) == ["self", "a", "r"]
    sig = inspect.signature(E.fr_sumcheck_round)
    assert list(sig.parameters) == ["self", "tables", "groups", "degree"] and sig.parameters["degree"].default is None
    assert list(inspect.signature(E.fr_mle_eq_dev).parameters) == ["self", "d_z", "nv", "d_out", "stream"]
    assert list(inspect.signature(E.fr_mle_fold_dev).parameters) == ["self", "d_in", "length", "r", "d_out", "stream"]
    assert list(inspect.signature(E.fr_sumcheck_round_dev).parameters) == ["self", "d_tables", "n", "k", "groups", "d_out", "degree", "stream"]
    assert (engine.MLE_VARS_MAX, engine.SUMCHECK_DEGREE_MAX, engine.SUMCHECK_TABLES_MAX, engine.SUMCHECK_GROUPS_MAX) == tuple(LIMITS.values())
    assert list(inspect.signature(mle.eq_table).parameters)[:2] == ["point", "limbs"] and inspect.signature(mle.eq_table).parameters["limbs"].default is False
    assert list(inspect.signature(mle.fold).parameters)[:2] == ["table", "r"] and list(inspect.signature(mle.evaluate).parameters)[:2] == ["table", "point"]
    assert list(inspect.signature(sumcheck.prove).parameters)[:3] == ["tables", "groups", "transcript"]
    assert list(inspect.signature(sumcheck.verify).parameters) == ["proof", "nv", "groups", "transcript"]
    assert sumcheck.Proof._fields == ("claim", "rounds", "finals")
    src = inspect.getsource(mle.evaluate)
    assert src.count("fr_mle_eq(") == 1 and src.count("fr_dot_batch(") == 1 and "fr_mle_fold" not in src
    src = inspect.getsource(sumcheck.prove)
    assert src.count("fr_sumcheck_round(") == 1 and src.count("fr_mle_fold(") == 1
    src = inspect.getsource(sumcheck.verify) + inspect.getsource(sumcheck._at)
    assert "engine" not in src and "fr_" not in src                                             # host integer arithmetic only
    doc = inspect.getdoc(sumcheck)
    for word in ("host-buffer", "once per round", "resident prover", "_dev", "Not built"):
        assert word in doc, word
    for word in ("SHA256(label)", "32 bytes, big endian", "0x00", "0x01", "0x02", "Fr.interpret"):
        assert word in inspect.getdoc(sumcheck.Transcript), word


class NoDevice:
    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def test_bad_arguments_raise_before_any_device_call_and_name_the_operand():
    import bn_amd
    from bn_amd import mle, sumcheck
    one = bn_amd.Fr.one()
    nd = NoDevice()
    with pytest.raises(ValueError, match="^z holds 31 variables"):
        bn_amd.fr_mle_eq([one] * 31, engine=nd)
    with pytest.raises(ValueError, match="^a holds 3 rows"):
        bn_amd.fr_mle_fold([one] * 3, one, engine=nd)
    with pytest.raises(ValueError, match="^r must be ONE scalar"):
        bn_amd.fr_mle_fold([one] * 4, np.zeros(8, np.uint64), engine=nd)
    rnd = lambda tables, groups, degree=None: bn_amd.fr_sumcheck_round(tables, groups, degree, engine=nd)
    two = [[one] * 4, [one] * 4]
    with pytest.raises(ValueError, match="^tables hold 3 indices"):
        rnd([[one] * 3], [(one, [0])])
    with pytest.raises(ValueError, match="^tables hold 0 indices"):
        rnd([[]], [(one, [0])])
    with pytest.raises(ValueError, match="^tables differ in length"):
        rnd([[one] * 4, [one] * 2], [(one, [0])])
    with pytest.raises(ValueError, match="^tables hold 17 tables"):
        rnd([[one] * 2] * 17, [(one, [0])])
    with pytest.raises(ValueError, match="^tables must have shape"):
        rnd(np.zeros((4, 2, 3), np.uint64), [(one, [0])])
    with pytest.raises(ValueError, match="^groups holds 0 products"):
        rnd(two, [])
    with pytest.raises(ValueError, match="^groups holds 17 products"):
        rnd(two, [(one, [0])] * 17)
    with pytest.raises(ValueError, match=r"^groups\[1\] holds 0 tables"):
        rnd(two, [(one, [0]), (one, [])])
    with pytest.raises(ValueError, match=r"^groups\[0\] holds 2 tables, 1..1"):
        rnd(two, [(one, [0, 1])], 1)
    with pytest.raises(ValueError, match=r"^groups\[0\] names table 2 but tables holds 2"):
        rnd(two, [(one, [0, 2])])
    with pytest.raises(ValueError, match=r"^groups\[0\] names table -1"):
        rnd(two, [(one, [-1])])
    with pytest.raises(ValueError, match="^degree must be 1..4, got 5"):
        rnd(two, [(one, [0] * 5)])
    with pytest.raises(ValueError, match=r"^the coefficient of groups\[0\] must be ONE scalar"):
        rnd(two, [(np.zeros(3, np.uint64), [0])])
    with pytest.raises(ValueError, match="^table holds 3 values but point has 2 variables"):
        mle.evaluate([one] * 3, [one] * 2, engine=nd)
    with pytest.raises(ValueError, match="a power of two"):
        sumcheck.prove([[one] * 6], [(one, [0])], engine=nd)
    with pytest.raises(ValueError, match="^tables hold 1 indices"):
        sumcheck.prove([[one]], [(one, [0])], engine=nd)
    with pytest.raises(ValueError, match="at least one product"):
        sumcheck.prove([[one] * 2], [], engine=nd)


class Model:
    """a stand-in engine that answers from the integer model and records what was asked"""
    def __init__(self): self.calls = []

    @staticmethod
    def _ints(a):
        from bn_amd import Fr
        a = np.asarray(a, np.uint64)
        return [Fr.from_limbs(r).v for r in a.reshape(-1, 4)]

    def fr_mle_eq(self, z):
        self.calls.append("fr_mle_eq")
        return FC.rows(MC.eq_table(self._ints(z)))

    def fr_mle_fold(self, a, r):
        self.calls.append("fr_mle_fold")
        a = np.asarray(a, np.uint64)
        flat = self._ints(a)
        return FC.rows(MC.fold(flat, self._ints(r)[0])).reshape((a.shape[0] // 2,) + a.shape[1:])

    def fr_sumcheck_round(self, tables, groups, degree=None):
        self.calls.append("fr_sumcheck_round")
        t = np.asarray(tables, np.uint64)
        n, k = t.shape[0], t.shape[1]
        flat = self._ints(t)
        rows = [flat[i * k:(i + 1) * k] for i in range(n)]
        gs = [(self._ints(c)[0], list(m)) for c, m in groups]
        return FC.rows(MC.round_sums(rows, gs, degree or MC.degree_of(gs)))

    def fr_dot_batch(self, coeff, x, offsets, index=None):
        self.calls.append("fr_dot_batch")
        assert index is None and [int(o) for o in offsets] == [0, len(coeff)]
        return FC.rows([sum(a * b for a, b in zip(self._ints(coeff), self._ints(x))) % R])


def test_mle_over_a_stand_in_engine_that_answers_from_the_model():
    """evaluate is ONE eq table and ONE inner product, and equals nv folds from the top variable down"""
    from bn_amd import Fr, mle
    m = Model()
    t = [Fr(v) for v in MC.values(16, 61)]
    point = [Fr(v) for v in MC.values(4, 62)]
    y = mle.evaluate(t, point, engine=m)
    assert m.calls == ["fr_mle_eq", "fr_dot_batch"]
    assert y == Fr(MC.evaluate([x.v for x in t], [p.v for p in point]))
    cur = t
    for r in point[::-1]:
        cur = mle.fold(cur, r, engine=m)
    assert cur == [y]
    assert mle.eq_table(point, engine=m) == [Fr(v) for v in MC.eq_table([p.v for p in point])]
    assert mle.eq_table([], engine=m) == [Fr.one()] and mle.eq_table(point, limbs=True, engine=m).shape == (16, 4)
    assert mle.evaluate([Fr(9)], [], engine=m) == Fr(9)
    both = np.stack([FC.rows(MC.values(8, 63)), FC.rows(MC.values(8, 64))], axis=1)            # (8, 2, 4): two tables index-major
    out = mle.fold(both, Fr(5), engine=m)
    assert out.shape == (4, 2, 4) and out[:, 1].tobytes() == FC.rows(MC.fold(MC.values(8, 64), 5)).tobytes()


@pytest.fixture(scope="module")
def statement():
    """eq_tau * (A B - C) with C = A o B: tables (as lists of Fr) and groups; the sum over the hypercube is zero"""
    from bn_amd import Fr
    nv = 4
    tau = MC.values(nv, 71)
    a, b = MC.values(1 << nv, 72), MC.values(1 << nv, 73)
    c = [x * y % R for x, y in zip(a, b)]
    tables = [[Fr(v) for v in t] for t in (MC.eq_table(tau), a, b, c)]
    return nv, tables, [(Fr(1), [0, 1, 2]), (Fr(R - 1), [0, 3])]


def test_sumcheck_over_a_stand_in_engine_that_answers_from_the_model(statement):
    from bn_amd import Fr, mle, sumcheck
    nv, tables, groups = statement
    m = Model()
    proof, point = sumcheck.prove(tables, groups, engine=m)
    assert m.calls == ["fr_sumcheck_round", "fr_mle_fold"] * nv
    assert proof.claim == Fr.zero() and len(proof.rounds) == nv and all(len(g) == 4 for g in proof.rounds) and len(proof.finals) == 4 and len(point) == nv
    ok, vpoint = sumcheck.verify(proof, nv, groups)
    assert ok and vpoint == point
    assert proof.finals == [mle.evaluate(t, point, engine=m) for t in tables]
    # the same proof from the model prover over the same transcript
    tr = sumcheck.Transcript("bn_amd.sumcheck")
    sumcheck._absorb_statement(tr, nv, 4, 3, groups, Fr.zero())
    def challenge(s, g):
        tr.absorb([Fr(v) for v in g])
        return tr.challenge().v
    rows = [[t[i].v for t in tables] for i in range(1 << nv)]
    claim, rounds, finals, mpoint = MC.prove(rows, [(c.v, j) for c, j in groups], challenge)
    assert claim == 0 and [[x.v for x in g] for g in proof.rounds] == rounds and [x.v for x in proof.finals] == finals and [p.v for p in point] == mpoint
    # another label, another proof; it verifies under its own label only
    other, _ = sumcheck.prove(tables, groups, transcript=sumcheck.Transcript("other"), engine=m)
    assert other.rounds[1] != proof.rounds[1]
    assert sumcheck.verify(other, nv, groups, transcript=sumcheck.Transcript("other"))[0] and not sumcheck.verify(other, nv, groups)[0]


def test_a_spoiled_proof_is_rejected(statement):
    from bn_amd import Fr, sumcheck
    nv, tables, groups = statement
    proof, _ = sumcheck.prove(tables, groups, engine=Model())
    one = Fr.one()
    for s in (0, nv - 1):
        for t in (0, 3):
            rounds = [list(g) for g in proof.rounds]
            rounds[s][t] = rounds[s][t] + one
            assert not sumcheck.verify(proof._replace(rounds=rounds), nv, groups)[0], (s, t)
    for j in range(4):
        finals = list(proof.finals); finals[j] = finals[j] + one
        assert not sumcheck.verify(proof._replace(finals=finals), nv, groups)[0], j
    assert not sumcheck.verify(proof._replace(claim=one), nv, groups)[0]
    assert sumcheck.verify(proof._replace(rounds=proof.rounds[:-1]), nv, groups) == (False, None)
    assert not sumcheck.verify(proof, nv, [(Fr(2), [0, 1, 2]), groups[1]])[0]                   # another statement
    # a sum that is not zero is proved as what it is
    wrong = [tables[0], tables[1], tables[2], [x + one for x in tables[3]]]
    p2, _ = sumcheck.prove(wrong, groups, engine=Model())
    assert p2.claim != Fr.zero() and sumcheck.verify(p2, nv, groups)[0] and not sumcheck.verify(p2._replace(claim=Fr.zero()), nv, groups)[0]


def test_the_transcript_is_the_documented_hash_chain():
    import hashlib
    from bn_amd import Fr, sumcheck
    h = lambda b: hashlib.sha256(b).digest()
    tr = sumcheck.Transcript("label")
    xs = [Fr(0), Fr(R - 1), Fr(1 << 200)]
    tr.absorb(xs)
    state = h(h(b"label") + b"".join(x.v.to_bytes(32, "big") for x in xs))
    assert tr.state == state
    r = tr.challenge()
    assert r.v == int.from_bytes(h(state + b"\x00") + h(state + b"\x01"), "big") % R and tr.state == h(state + b"\x02")
    assert tr.challenge() != r
    assert sumcheck.Transcript(b"label").state == h(b"label")


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_sumcheck_piece.argtypes = []; l.bn254_fr_sumcheck_piece.restype = C.c_uint
    l.bn254_fr_sumcheck_fan.argtypes = []; l.bn254_fr_sumcheck_fan.restype = C.c_uint
    l.bn254_fr_mle_set_launch_max.argtypes = [C.c_size_t]
    l.bn254_fr_sumcheck_set_piece.argtypes = [C.c_uint]
    return l


DUMMY = C.c_void_p(0x1000)       # never dereferenced: every case below is answered before the data is read


def _sz(*v):
    return (C.c_size_t * len(v))(*v)


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


COEFF = (C.c_uint64 * 64)()


@pytest.mark.parametrize("case, z, nv, out", [
    ("nv below zero", DUMMY, -1, DUMMY),
    ("nv above the limit", DUMMY, 31, DUMMY),
    ("a NULL out", DUMMY, 3, None),
    ("a NULL out without variables", None, 0, None),
    ("a NULL z with variables", None, 1, DUMMY),
])
def test_eq_argument_errors_answer_without_a_device(lib, case, z, nv, out):
    assert [lib.bn254_fr_mle_eq(None, z, nv, out), lib.bn254_fr_mle_eq_dev(None, z, nv, out, None)] == [BAD_ARG] * 2, case


@pytest.mark.parametrize("case, a, length, r, out", [
    ("an odd length", DUMMY, 3, DUMMY, DUMMY),
    ("one record", DUMMY, 1, DUMMY, DUMMY),
    ("len > 2^40", DUMMY, (1 << 40) + 2, DUMMY, DUMMY),
    ("a NULL in", None, 4, DUMMY, DUMMY),
    ("a NULL r", DUMMY, 4, None, DUMMY),
    ("a NULL out", DUMMY, 4, DUMMY, None),
])
def test_fold_argument_errors_answer_without_a_device(lib, case, a, length, r, out):
    assert [lib.bn254_fr_mle_fold(None, a, length, r, out), lib.bn254_fr_mle_fold_dev(None, a, length, r, out, None)] == [BAD_ARG] * 2, case


def test_an_empty_fold_is_ok_and_writes_nothing(lib):
    out = (C.c_uint64 * 8)(*([7] * 8))
    for p in (None, DUMMY):
        assert [lib.bn254_fr_mle_fold(None, p, 0, p, out), lib.bn254_fr_mle_fold_dev(None, p, 0, p, out, None)] == [0, 0]
        assert [lib.bn254_fr_mle_fold(None, p, 0, p, None), lib.bn254_fr_mle_fold_dev(None, p, 0, p, None, None)] == [0, 0]
    assert list(out) == [7] * 8


GOOD = dict(tables=DUMMY, n=8, k=3, off=_sz(0, 2, 3), members=_u64(0, 2, 1), coeff=COEFF, g=2, degree=2, out=DUMMY)


@pytest.mark.parametrize("case, change", [
    ("n odd", dict(n=7)),
    ("n below 2", dict(n=0)),
    ("n is one", dict(n=1)),
    ("no table", dict(k=0)),
    ("17 tables", dict(k=17)),
    ("no group", dict(g=0)),
    ("17 groups", dict(g=17, off=_sz(*range(18)), members=_u64(*([0] * 17)))),
    ("degree zero", dict(degree=0)),
    ("degree negative", dict(degree=-1)),
    ("degree five", dict(degree=5)),
    ("an empty group", dict(off=_sz(0, 2, 2))),
    ("a group longer than the degree", dict(off=_sz(0, 3, 4), members=_u64(0, 1, 2, 0))),
    ("a table number that is k", dict(members=_u64(0, 3, 1))),
    ("a table number far outside", dict(members=_u64(0, 2, 1 << 40))),
    ("offsets[0] != 0", dict(off=_sz(1, 2, 3))),
    ("decreasing offsets", dict(off=_sz(0, 2, 1))),
    ("NULL tables", dict(tables=None)),
    ("NULL offsets", dict(off=None)),
    ("NULL table numbers", dict(members=None)),
    ("NULL coefficients", dict(coeff=None)),
    ("NULL out", dict(out=None)),
    ("n k > 2^40", dict(n=(1 << 39) + 2, k=2, members=_u64(0, 1, 1))),
])
def test_round_argument_errors_answer_without_a_device(lib, case, change):
    a = dict(GOOD, **change)
    args = (a["tables"], a["n"], a["k"], a["off"], a["members"], a["coeff"], a["g"], a["degree"], a["out"])
    assert [lib.bn254_fr_sumcheck_round(None, *args), lib.bn254_fr_sumcheck_round_dev(None, *args, None)] == [BAD_ARG] * 2, case


def test_the_hooks_check_their_bounds(lib):
    P, F = lib.bn254_fr_sumcheck_piece(), lib.bn254_fr_sumcheck_fan()
    assert P in (4, 8, 16, 32) and F == 16                                                      # the ones the host simulation runs
    try:
        assert lib.bn254_fr_sumcheck_set_piece(65) == BAD_ARG and lib.bn254_fr_sumcheck_set_piece(4) == 0 and lib.bn254_fr_sumcheck_set_piece(64) == 0
        assert lib.bn254_fr_mle_set_launch_max((1 << 22) + 1) == BAD_ARG
        assert lib.bn254_fr_mle_set_launch_max(20) == 0
    finally:
        assert lib.bn254_fr_sumcheck_set_piece(0) == 0 and lib.bn254_fr_mle_set_launch_max(0) == 0
    assert lib.bn254_fr_sumcheck_piece() == P


def test_the_kernels_are_instances_of_fr_decode_k_and_spill_nothing():
    import isa_mix
    import kernel_meta
    from test_build_quality import SPILL_CEILING
    so = ROOT / "bn_amd" / "libbn254_hip.so"
    import lane_shell
    src = lane_shell.unit_source("bn254_mle.hip")  # the unit adds no kernel under any other name: the shell is lane_launch.hpp's
    assert "bn_lane_launch<MLE_BLOCK>(" in src and "MLE_BLOCK = 256" in src
    if not so.exists() or not (isa_mix.LLVM / "llvm-readelf").exists():
        pytest.skip("library or llvm-readelf not present")
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0
    meta = kernel_meta.instances(so)
    for op, count in (("FrSumcheckRoundOp", 4), ("FrSumcheckSumOp", 1), ("FrMleEqOp", 1), ("FrMleFoldOp", 1)):
        mine = [n for n in meta if kernel_meta.short_name(n) == "bn254_fr_decode_k" and re.search(r"\d+" + op + "(E|I)", n)]
        assert len(mine) == count, (op, mine)                                                   # the round: one instance per degree
        for n in mine:
            assert meta[n]["spill"] == 0 and meta[n]["private"] == 0 and meta[n]["lds"] == 0, (n, meta[n])
