"""Every leaf the GPU runs as an inline-asm chain (bn_amd/csrc/fe_asm.hpp, BN_LC_CHAIN in fe.hpp), through its bounds-checked C++ twin on RAW limbs
(tests/hostsim/hostsim_leaf.cpp) at the operand bounds the leaf states - every case of tests/leaf_cases.py - against the integer model there.
The twin aborts the process on a contract violation, so a green run also proves every case to be inside the contract: tests/test_gpu_leaf.py sends
the same cases to the asm leaves and expects the twin's limbs.  Also here: the committed fe_asm.hpp is what tools/gen_asm_leaf.py writes."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import hostsim_leaf_lib as H
import leaf_cases as L

ROOT = pathlib.Path(__file__).resolve().parents[1]
NAMES = [l[0] for l in L.LEAVES]


def test_the_list_of_leaves_is_the_compiled_one():
    assert H.leaf_table() == [(name, kinds, outw) for name, kinds, outw, _ in L.LEAVES]


@pytest.mark.parametrize("name", NAMES)
def test_twin_against_the_integer_model(name):
    _, kinds, outw, d = L.LEAVES[L.LEAF_ID[name]]
    cs = L.cases(name)
    classes = {c[0].split()[0] for c in cs}
    assert {"ceiling", "all", "random"} <= classes and ("hot" in classes or not any(d.get("C", (1,)))), classes
    assert sum(1 for c in cs if c[0].startswith("random")) == 256
    if d.get("flag") or d["family"] == "wred":
        assert {c[3] for c in cs} == {0, 1}
    ops, bounds, flags = L.pack(name)
    before = ops.copy()
    got = H.run(L.LEAF_ID[name], ops, bounds, flags, outw)
    assert np.array_equal(ops, before)
    count, first = L.failures(name, got)
    assert count == 0, (name, count, first)


def test_the_reductions_reach_every_chain():
    """every branch of BN_LC_CHAIN that can be instantiated - (terms on their own in the 64-bit chain, a narrow sum exists) - has an entry; the
    forms with a per-lane sign and with every term wide are among them"""
    reached = {L.lc_branch(d)[:2] for _, _, _, d in L.LEAVES if d["family"] == "lc"}
    assert reached == {(n, narrow) for n in range(5) for narrow in (False, True)} - {(4, True)}
    assert any(d["family"] == "lc" and d["SIGN2"] for *_, d in L.LEAVES) and any(d["family"] == "lc" and d["WIDE"] for *_, d in L.LEAVES)


def test_the_model_rejects_a_wrong_limb():
    """the model is not vacuous: the twin's result with one bit of one limb flipped fails it, for every leaf"""
    for name in NAMES:
        _, kinds, outw, d = L.LEAVES[L.LEAF_ID[name]]
        ops, bounds, flags = L.pack(name)
        got = H.run(L.LEAF_ID[name], ops[-8:], bounds[-8:], flags[-8:], outw)
        for k, case in enumerate(L.cases(name)[-8:]):
            bad = got[k].copy(); bad[k % outw] ^= 1 << (k % 29)
            assert L.check(name, case, got[k]) is None and L.check(name, case, bad) is not None, (name, case[0])


def test_the_probe_builds_and_stays_out_of_the_product():
    """tests/leafprobe/: cross-compiles for gfx950, holds one kernel per leaf in each of its two build contexts and the entry points of both -
    and the PRODUCT library holds none of them, and nothing under bn_amd/ refers to the probe"""
    import ctypes
    import leafprobe
    lib = ctypes.CDLL(str(leafprobe.build()))
    for ctx in leafprobe.CONTEXTS:
        for sym in ("run", "leaf_count", "leaf_info"):
            assert hasattr(lib, "bnlp_%s_%s" % (ctx, sym))
    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_meta
    from bn_amd import _native
    assert set(kernel_meta.kernel_meta(leafprobe.LIB)) == {p + name for p in ("lpi_", "lpf_") for name in NAMES}
    assert not [k for k in kernel_meta.kernel_meta(_native.build()) if k.startswith(("lpi_", "lpf_", "bnlp_"))]
    for f in (ROOT / "bn_amd").rglob("*.py"):
        assert "leafprobe" not in f.read_text(), f
    for f in (ROOT / "bn_amd" / "csrc").glob("*.hip"):
        assert "leafprobe" not in f.read_text() and "leaf_list" not in f.read_text(), f


def test_the_committed_asm_header_is_current():
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_asm_leaf.py"), "--check"], capture_output=True, text=True)
    assert p.returncode == 0 and "up to date" in p.stdout, p.stdout + p.stderr
    other = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_asm_leaf.py"), "--check", str(ROOT / "README.md")], capture_output=True, text=True)
    assert other.returncode == 1 and "stale" in other.stdout                                    # the check does tell a difference, and writes nothing
