"""The fused fold-then-round call (bn254_fr_sumcheck_fold_round and its _dev twin) and bn_amd.sumcheck.prove_resident without a GPU: the two
declarations in every layer that mirrors the C header, the argument checks that answer before any device is touched - overlaps among them -,
the profiling scope, the Python surface and its errors, the test hooks, and that the four new kernels are template instances of an existing
kernel name (bn254_fr_decode_k<Op>), whose spill ceiling tests/test_build_quality.py enforces."""
import ctypes as C
import inspect
import pathlib
import re

import numpy as np
import pytest

import hostsim_fold_round_lib as HF
import test_binding_signatures as B

ROOT = pathlib.Path(__file__).resolve().parents[1]

CONST = ("const",)
MUT = ("mut",)
CTX, FR_IN, FR_OUT, N, INT = ("void", MUT), ("fr", CONST), ("fr", MUT), ("usize", ()), ("int", ())
D_IN, D_OUT, OFF, U64 = ("void", CONST), ("void", MUT), ("usize", CONST), ("u64", CONST)
EXPECTED = {
    "bn254_fr_sumcheck_fold_round": [CTX, FR_IN, N, N, FR_IN, OFF, U64, FR_IN, N, INT, FR_OUT, FR_OUT],
    "bn254_fr_sumcheck_fold_round_dev": [CTX, D_IN, N, N, FR_IN, OFF, U64, FR_IN, N, INT, D_OUT, D_OUT, D_OUT],
}
NAMES = tuple(EXPECTED)
SCOPE = "fr_sumcheck_fold_round"
HOOKS = ("bn254_fr_sumcheck_fold_piece", "bn254_fr_sumcheck_fold_set_piece", "bn254_fr_sumcheck_fold_piece_for")
BAD_ARG = -2


def test_header_declares_the_two_entry_points():
    decls = B.c_declarations()
    for name, params in EXPECTED.items():
        assert name in decls, name
        assert [t for _, t in decls[name]["params"]] == params, (name, decls[name]["params"])
        assert decls[name]["ret"] == ("int", ())
        assert decls[name]["params"][-1][0] == ("stream" if name.endswith("_dev") else "out")
    hdr = B.HEADER.read_text()
    semantics = hdr[hdr.index("Semantics replaced"):hdr.index("Error behaviour")]
    threading = hdr[hdr.index("Threading"):hdr.index("#ifndef BN254_HIP_H")]
    for name in NAMES:
        assert name in semantics and name in threading, name
    assert "bn254_fr_sumcheck_fold_round serialises on the context" in threading
    own = " ".join(hdr[hdr.index("The fold of one sumcheck round and the round polynomial of the next"):hdr.index("int bn254_fr_sumcheck_fold_round(")].split())
    for word in ("index-major", "MOST significant", "HOST", "bn254_fr_mle_fold(tables, n k, r)", "bn254_fr_sumcheck_round(folded, n / 2, k", "canonical", "one that no group names",
                 "`folded` may be exactly `tables`", "rows [n/2, n) are then left as they were", "BN254_E_BAD_ARG", "h2 = n / 4", "a0 + r (a2 - a0)", "a1 + r (a3 - a1)",
                 "belong to that lane alone", "No LDS, no atomics", "compute units * 4 * 64 * 2", "profiles/r20_fold_round.txt", "n not a multiple of 4 or below 4", "n k > 2^40",
                 "Threading"):
        assert word in own, word
    for hook in HOOKS:                                                                          # the test hooks are internal
        assert hook + "(" not in hdr, hook


def test_the_scope_name_is_documented_and_used():
    hdr = B.HEADER.read_text()
    block = hdr[hdr.index("/* kernel: "):hdr.index("int bn254_kernel_stats(")]
    names = re.findall(r'"(\w+)"', block)
    assert names.count(SCOPE) == 1 and len(names) == len(set(names))
    unit = (ROOT / "bn_amd" / "csrc" / "bn254_mle.hip").read_text() + (ROOT / "bn_amd" / "csrc" / "mle_ops.hpp").read_text()
    assert '"%s"' % SCOPE in unit and "FR_SUMCHECK_FOLD_ROUND_SCOPE" in unit


def test_every_mirror_of_the_header_has_them():
    from bn_amd import _native
    assert set(NAMES) <= set(_native.SIGNATURES)
    for name in NAMES:
        assert len(_native.SIGNATURES[name]) == len(EXPECTED[name]), name
    txt = B.RUST_LIB.read_text()
    rust = B.rust_declarations(txt)
    assert set(NAMES) <= set(rust)
    assert B.compare(B.c_declarations(), {k: rust[k] for k in NAMES}, "bindings/rust/src/lib.rs") == []
    assert ("pub fn fr_sumcheck_fold_round(tables: &[Fr], k: usize, r: &Fr, group_offsets: &[usize], group_tables: &[u64], group_coeff: &[Fr], degree: usize) "
            "-> Result<(Vec<Fr>, Vec<Fr>), GpuError>") in txt
    md = B.rust_declarations(B.rust_blocks_of_markdown(B.INTEGRATION.read_text()))
    assert set(NAMES) <= set(md)
    hpp = (ROOT / "include" / "bn254.hpp").read_text()
    assert "fr_sumcheck_fold_round(" in hpp and "bn254_fr_sumcheck_fold_round(" in hpp
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        assert "bn254_fr_sumcheck_fold_round" in text and "prove_resident" in text and "profiles/r20_fold_round.txt" in text, doc
    assert (ROOT / "tools" / "time_fold_round.py").exists() and (ROOT / "profiles" / "r20_fold_round.txt").exists()


def test_python_surface():
    import bn_amd
    from bn_amd import engine, sumcheck
    sig = inspect.signature(bn_amd.fr_sumcheck_fold_round)
    assert list(sig.parameters) == ["tables", "r", "groups", "degree", "engine"] and sig.parameters["degree"].default is None
    E = engine.Engine
    sig = inspect.signature(E.fr_sumcheck_fold_round)
    assert list(sig.parameters) == ["self", "tables", "r", "groups", "degree"] and sig.parameters["degree"].default is None
    assert list(inspect.signature(E.fr_sumcheck_fold_round_dev).parameters) == ["self", "d_tables", "n", "k", "r", "groups", "d_folded", "d_out", "degree", "stream"]
    assert list(inspect.signature(sumcheck.prove_resident).parameters) == list(inspect.signature(sumcheck.prove).parameters) == ["tables", "groups", "transcript", "engine"]
    assert isinstance(sumcheck.FUSED, bool)
    doc = inspect.getdoc(sumcheck)
    for word in ("prove_resident", "ONE device buffer", "fr_sumcheck_fold_round_dev", "profiles/r20_fold_round.txt", "Not built"):
        assert word in doc, word


class NoDevice:
    device = 0

    def __getattr__(self, name): raise AssertionError("a device call was made: " + name)


def test_bad_arguments_raise_before_any_device_call_and_name_the_operand():
    import bn_amd
    from bn_amd import sumcheck
    one = bn_amd.Fr.one()
    nd = NoDevice()
    call = lambda tables, groups, degree=None, r=one: bn_amd.fr_sumcheck_fold_round(tables, r, groups, degree, engine=nd)
    two = [[one] * 4, [one] * 4]
    for n in (2, 6):
        with pytest.raises(ValueError, match="^tables hold %d indices: a fold and a round need a multiple of 4" % n):
            call([[one] * n], [(one, [0])])
    with pytest.raises(ValueError, match="^tables hold 0 indices"):
        call([[]], [(one, [0])])
    with pytest.raises(ValueError, match="^tables hold 3 indices"):
        call([[one] * 3], [(one, [0])])
    with pytest.raises(ValueError, match="^tables hold 17 tables"):
        call([[one] * 4] * 17, [(one, [0])])
    with pytest.raises(ValueError, match=r"^groups\[0\] holds 2 tables, 1..1"):
        call(two, [(one, [0, 1])], 1)
    with pytest.raises(ValueError, match=r"^groups\[0\] names table 2 but tables holds 2"):
        call(two, [(one, [0, 2])])
    with pytest.raises(ValueError, match="^r must be ONE scalar"):
        call(two, [(one, [0])], r=np.zeros(8, np.uint64))
    with pytest.raises(ValueError, match="a power of two"):
        sumcheck.prove_resident([[one] * 6], [(one, [0])], engine=nd)
    with pytest.raises(ValueError, match="at least one product"):
        sumcheck.prove_resident([[one] * 2], [], engine=nd)


@pytest.fixture(scope="module")
def lib():
    from bn_amd import _native
    l = _native.lib()
    l.bn254_fr_sumcheck_fold_piece.argtypes = []; l.bn254_fr_sumcheck_fold_piece.restype = C.c_uint
    l.bn254_fr_sumcheck_fold_set_piece.argtypes = [C.c_uint]
    return l


def _sz(*v):
    return (C.c_size_t * len(v))(*v)


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


# never dereferenced: every case below is answered before the data is read.  n = 8 rows of k = 3 tables are 768 bytes, folded 384, out 96
TABLES = 0x100000
COEFF = (C.c_uint64 * 64)()
GOOD = dict(tables=TABLES, n=8, k=3, r=0x1000, off=_sz(0, 2, 3), members=_u64(0, 2, 1), coeff=COEFF, g=2, degree=2, folded=0x200000, out=0x300000)
BAD = [
    ("n is zero", dict(n=0)),
    ("n is two", dict(n=2)),
    ("n is six", dict(n=6)),
    ("a NULL r", dict(r=None)),
    ("a NULL folded", dict(folded=None)),
    ("a NULL out", dict(out=None)),
    ("a NULL tables", dict(tables=None)),
    ("no table", dict(k=0)),
    ("17 tables", dict(k=17)),
    ("no group", dict(g=0)),
    ("degree five", dict(degree=5)),
    ("a group longer than the degree", dict(off=_sz(0, 3, 4), members=_u64(0, 1, 2, 0))),
    ("a table number that is k", dict(members=_u64(0, 3, 1))),
    ("offsets[0] != 0", dict(off=_sz(1, 2, 3))),
    ("n k > 2^40", dict(n=(1 << 39) + 4, k=2, members=_u64(0, 1, 1))),
    ("folded overlaps the first record of tables from below", dict(folded=TABLES - 384 + 32)),
    ("folded overlaps the last record of tables", dict(folded=TABLES + 768 - 32)),
    ("folded one record into tables", dict(folded=TABLES + 32)),
    ("out inside tables", dict(out=TABLES + 512)),
    ("out is tables", dict(out=TABLES)),
    ("out overlaps the last record of folded", dict(out=0x200000 + 384 - 32)),
    ("out's last record is the first of folded", dict(out=0x200000 - 64)),
    ("in place, out inside the upper half", dict(folded=TABLES, out=TABLES + 700)),
]


def _args(a):
    return (a["tables"], a["n"], a["k"], a["r"], a["off"], a["members"], a["coeff"], a["g"], a["degree"], a["folded"], a["out"])


@pytest.mark.parametrize("case, change", BAD, ids=[c for c, _ in BAD])
def test_argument_errors_answer_without_a_device(lib, case, change):
    args = _args(dict(GOOD, **change))
    assert [lib.bn254_fr_sumcheck_fold_round(None, *args), lib.bn254_fr_sumcheck_fold_round_dev(None, *args, None)] == [BAD_ARG] * 2, case
    assert HF.lib().hfr_check(*args) == BAD_ARG


@pytest.mark.parametrize("case, change", [
    ("apart", {}),
    ("the exact alias", dict(folded=TABLES)),
    ("folded right behind tables", dict(folded=TABLES + 768)),
    ("folded right in front of tables", dict(folded=TABLES - 384)),
    ("out right behind tables, in place", dict(folded=TABLES, out=TABLES + 768)),
    ("out right in front of folded", dict(out=0x200000 - 96)),
    ("the smallest call", dict(n=4)),
])
def test_the_check_accepts(case, change):
    """through the host simulation's copy of the check alone: the library would go on to a device"""
    assert HF.lib().hfr_check(*_args(dict(GOOD, **change))) == 0, case


def test_the_hooks_check_their_bounds(lib):
    P = lib.bn254_fr_sumcheck_fold_piece()
    assert P in (4, 8, 16)
    try:
        assert lib.bn254_fr_sumcheck_fold_set_piece(65) == BAD_ARG and lib.bn254_fr_sumcheck_fold_set_piece(4) == 0 and lib.bn254_fr_sumcheck_fold_set_piece(64) == 0
    finally:
        assert lib.bn254_fr_sumcheck_fold_set_piece(0) == 0
    assert lib.bn254_fr_sumcheck_fold_piece() == P


def test_the_unit_adds_no_kernel_name():
    """the four new kernels are instances of bn254_fr_decode_k, which tests/test_build_quality.py holds to a spill count of 0"""
    from test_build_quality import SPILL_CEILING
    import lane_shell
    lane_shell.unit_source("bn254_mle.hip")  # the unit adds no kernel under any other name: the shell is lane_launch.hpp's
    assert SPILL_CEILING["bn254_fr_decode_k"] == 0                                              # test_build_quality holds every instance to it
