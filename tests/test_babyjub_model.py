"""Baby Jubjub and EdDSA-Poseidon without a GPU: the facts the interface rests on, in integers; the published Poseidon5 answers and circomlibjs'
signature from both the model of tests/babyjub_cases.py and the package's host functions; the package against the model on the edge sets; and
the generated constants."""
import pathlib
import subprocess
import sys

import babyjub_cases as BC
import poseidon_cases as PC

ROOT = pathlib.Path(__file__).resolve().parents[1]
R = BC.R


def test_the_curve_facts():
    from bn_amd import babyjub as BJ
    assert (BJ.A, BJ.D, BJ.L, BJ.ORDER, BJ.G, BJ.B8, BJ.IDENTITY) == (BC.A_COEFF, BC.D_COEFF, BC.L, BC.ORDER, BC.G, BC.B8, BC.O) and BJ.A == 168700 and BJ.D == 168696
    assert pow(BC.A_COEFF, (R - 1) // 2, R) == 1 and pow(BC.D_COEFF, (R - 1) // 2, R) == R - 1          # a is a square, d is not: the law is complete
    assert BC.L.bit_length() == 251 and BC.ORDER == 8 * BC.L == 21888242871839275222246405745257275088614511777268538073601725287587578984328
    assert BC.ORDER > R and abs(BC.ORDER - (R + 1)) <= 2 * int(R ** 0.5) + 2                             # Hasse; 8 l is not an element of Fr
    assert all(pow(w, BC.L - 1, BC.L) == 1 for w in (2, 3, 5, 7))                                         # l is (a probable) prime
    for p in (BC.O, BC.G, BC.B8):
        assert BC.on_curve(p) and BJ.on_curve_host(p)
    assert BC.add(BC.O, BC.G) == BC.G and BC.add(BC.G, BC.neg(BC.G)) == BC.O and BC.neg(BC.G) == ((-BC.G[0]) % R, BC.G[1])
    assert BC.mul(BC.G, 8) == BC.B8 and BC.mul(BC.B8, BC.L) == BC.O and BC.mul(BC.G, BC.ORDER) == BC.O
    assert BC.mul(BC.G, BC.L) != BC.O and BC.mul(BC.G, 4 * BC.L) != BC.O                                  # G has the full order 8 l
    sm = BC.small_order_points()
    assert sm["order2"] == (0, R - 1) and BC.add(sm["order2"], sm["order2"]) == BC.O
    assert sm["order4"][1] == 0 and BC.A_COEFF * sm["order4"][0] ** 2 % R == 1 and BC.mul(sm["order4"], 2) == sm["order2"] and sm["order4neg"] == BC.neg(sm["order4"])
    assert BC.mul(sm["order8"], 4) == sm["order2"]
    assert BC.add(BC.B8, BC.B8) == BC.mul(BC.B8, 2)                                                      # doubling is the same formula
    assert not BC.on_curve(BC.OFF_CURVE)
    names = [n for n, _ in BC.edge_points()]
    assert len(set(names)) == len(names) and all(BC.on_curve(p) for _, p in BC.edge_points())
    assert [BC.validate_status(*p) for n, p in BC.edge_points() if n.startswith("B8+")] == [5] * 4


def test_the_width_6_instance_comes_out_of_the_grain_derivation():
    from bn_amd import poseidon
    assert PC.PARTIAL[6] == 60 == poseidon.R_P[6] and poseidon.R_F == PC.FULL == 8
    C, M = poseidon.constants(6)
    mC, mM, xs, ys = PC.constants(6)
    assert list(C) == mC and len(C) == 68 * 6 and [list(r) for r in M] == mM
    assert len(set(xs + ys)) == 12 and all((x + y) % R for x in xs for y in ys)                           # the first Cauchy draw: distinct, no zero sum
    for s in PC.states(6, 12, 5):
        assert poseidon.permute_host(s) == PC.permute(s)
    # the public hash stays at arity four
    assert poseidon.ARITY_MAX == 4
    try:
        poseidon.hash_host([1, 2, 3, 4, 5])
    except ValueError:
        pass
    else:
        raise AssertionError("arity five must stay out of the public hash")


def test_the_published_poseidon5_answers():
    from bn_amd import eddsa, poseidon
    for ins, want in BC.KNOWN_POSEIDON5.items():
        assert BC.poseidon5(list(ins)) == want == poseidon.permute_host([0] + list(ins))[0]
        assert eddsa.challenge_host((ins[2], ins[3]), (ins[0], ins[1]), ins[4]) == want


def test_the_circomlibjs_signature():
    from bn_amd import babyjub as BJ, eddsa
    assert BC.KAT_M == int.from_bytes(bytes(range(10)) + b"\0\0", "little")
    assert BC.on_curve(BC.KAT_A) and BC.on_curve(BC.KAT_R8) and BC.KAT_S < BC.L
    assert BC.verify_status(BC.KAT_A, BC.KAT_R8, BC.KAT_S, BC.KAT_M) == 0
    assert eddsa.verify_host(BC.KAT_A, BC.KAT_M, (BC.KAT_R8, BC.KAT_S)) is True
    assert eddsa.verify_host(BJ.Point(*BC.KAT_A), BC.KAT_M + 1, (BJ.Point(*BC.KAT_R8), BC.KAT_S)) is False
    # the scalar of A is the integer 8 hm: reduced mod l it is another scalar, and here the same point only because A has order l
    hm = BC.challenge(BC.KAT_A, BC.KAT_R8, BC.KAT_M)
    assert BC.mul(BC.B8, BC.KAT_S) == BC.add(BC.KAT_R8, BC.mul(BC.KAT_A, 8 * hm)) == BC.add(BC.KAT_R8, BC.mul(BC.mul(BC.KAT_A, 8), hm))


def test_signing_gives_the_same_equation_as_circomlib():
    """A = [s]B8, S = rho + 8 hm s is circomlib's A = [key >> 3]B8, S = rho + hm key with key = 8 s"""
    s, m, rho = 123456789123456789, 77, 424242
    a, r8, S = BC.sign(s, m, rho)
    key = 8 * s
    assert a == BC.mul(BC.B8, key >> 3) and S == (rho + BC.challenge(a, r8, m) * key) % BC.L and BC.verify_status(a, r8, S, m) == 0


def test_the_failing_classes_and_the_small_order_keys():
    from bn_amd import eddsa
    for name, (a, r8, s, m), want in BC.failing_rows():
        assert eddsa.verify_status_host(a, m, (r8, s)) == want, name
    st = {name: want for name, _, want in BC.failing_rows()}
    assert st["A = O"] == st["A of order 2"] == st["A of order 8"] == 0                                   # no subgroup check, as in circomlib


def test_the_package_host_functions_against_the_model():
    from bn_amd import babyjub as BJ
    pts = [p for _, p in BC.edge_points()]
    for p in pts:
        assert BJ.on_curve_host(p) and BJ.neg_host(p) == BC.neg(p)
        for q in pts:
            assert BJ.add_host(p, q) == BC.add(p, q)
    for p in pts[:6]:
        for k in BC.EDGE_SCALARS + [BC.ORDER, 8 * BC.L + 1]:
            assert BJ.mul_host(p, k) == BC.mul(p, k)
    assert not BJ.on_curve_host(BC.OFF_CURVE) and not BJ.on_curve_host((R, 1)) and not BJ.on_curve_host((0, R + 1))
    assert BJ.Point(*BC.B8) == BJ.Point.base() and -BJ.Point.base() == BJ.Point(*BC.neg(BC.B8)) and BJ.Point.identity() == BJ.Point(0, 1)
    assert (BJ.point_limbs(BC.B8) == BC.point_rows([BC.B8])[0]).all() and BJ.Point.from_limbs(BC.point_rows([BC.G])[0]) == BJ.Point.generator()
    assert (BJ.raw_limbs(R, 1) == BC.point_rows([(R, 1)])[0]).all()


def test_the_committed_constants_are_current():
    tool = str(ROOT / "tools" / "gen_babyjub_constants.py")
    p = subprocess.run([sys.executable, tool, "--check"], capture_output=True, text=True)
    assert p.returncode == 0 and "up to date" in p.stdout, p.stdout + p.stderr
    other = subprocess.run([sys.executable, tool, "--check", str(ROOT / "README.md")], capture_output=True, text=True)
    assert other.returncode == 1 and "stale" in other.stdout                                             # the check does tell a difference, and writes nothing
    txt = (ROOT / "bn_amd" / "csrc" / "babyjub_constants.hpp").read_text()
    mont = lambda v: "{" + ", ".join("0x%08xu" % ((v * (1 << 256) % R >> (32 * i)) & 0xffffffff) for i in range(8)) + "}"
    for v in (BC.A_COEFF, BC.D_COEFF, BC.B8[0], BC.B8[1], BC.mul(BC.B8, 3)[0], BC.mul(BC.B8, 2)[0] * BC.mul(BC.B8, 2)[1] % R):
        assert mont(v) in txt
    assert "{" + ", ".join("0x%08xu" % ((BC.L >> (32 * i)) & 0xffffffff) for i in range(8)) + "}" in txt
