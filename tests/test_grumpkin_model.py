"""Grumpkin in Python integers, no GPU and no library: the curve facts the device code rests on, the projective formulas of
bn_amd/csrc/grumpkin_ops.hpp (written out again in tests/grumpkin_cases.py) against chord and tangent on every pair of edge points, the host
model of bn_amd/grumpkin.py against the independent one, the generated constants, and the Pedersen generators."""
import pathlib
import subprocess
import sys

import grumpkin_cases as GC

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_the_curve_facts():
    assert GC.on_curve(GC.G) and GC.G[1] ** 2 % GC.R == GC.R - 16 and GC.G[1] <= (GC.R - 1) // 2
    assert pow(GC.B_COEFF, (GC.R - 1) // 2, GC.R) == GC.R - 1                  # -17 is a non-residue: no point has x = 0, (0, 0) is free for O
    assert GC.mul(GC.G, GC.R) != GC.O and GC.R % 3 == 1 and GC.Q % 3 == 1
    names = [n for n, _ in GC.edge_points()]
    assert names[:5] == ["O", "G", "negG", "2G", "(q-1)G"]


def test_q_times_every_edge_point_is_the_identity():
    for name, p in GC.edge_points():
        assert GC.mul(p, GC.Q) == GC.O, name
        assert GC.mul(p, GC.Q + 1) == p, name


def test_the_projective_addition_agrees_with_chord_and_tangent_on_every_edge_pair():
    pts = [p for _, p in GC.edge_points()]
    for p in pts:
        for q in pts:                                                        # P + P, P + O, O + O and P + (-P) are among them
            S = GC.proj_add(GC.to_proj(p), GC.to_proj(q))
            assert S != (0, 0, 0) and GC.from_proj(S) == GC.add(p, q), (p, q)
    # and on projective inputs with Z != 1
    P3 = GC.proj_add(GC.to_proj(GC.G), GC.to_proj(GC.mul(GC.G, 2)))
    assert P3[2] != 1 and GC.from_proj(GC.proj_add(P3, P3)) == GC.mul(GC.G, 6) and GC.from_proj(GC.proj_add(P3, (0, 1, 0))) == GC.mul(GC.G, 3)


def test_the_projective_doubling_agrees_with_add_p_p():
    for name, p in GC.edge_points():
        P = GC.to_proj(p)
        D, S = GC.proj_double(P), GC.proj_add(P, P)
        assert GC.proj_eq(D, S) and GC.from_proj(D) == GC.add(p, p), name
        D2 = GC.proj_double(S)                                               # Z != 1
        assert GC.proj_eq(D2, GC.proj_add(S, S)) and GC.from_proj(D2) == GC.mul(p, 4), name


def test_the_package_model_agrees_with_the_independent_one():
    from bn_amd import grumpkin as GK
    assert (GK.Q, GK.R, GK.B % GK.R, GK.G, GK.IDENTITY) == (GC.Q, GC.R, GC.B_COEFF, GC.G, GC.O)
    pts = [p for _, p in GC.edge_points()]
    for p in pts:
        assert GK.on_curve_host(p) and GK.neg_host(p) == GC.neg(p)
        for q in pts:
            assert GK.add_host(p, q) == GC.add(p, q)
        for k in (0, 1, 2, 15, 16, GC.Q - 1, GC.Q, (1 << 256) - 1):
            assert GK.mul_host(p, k) == GC.mul(p, k)
    assert not GK.on_curve_host(GC.OFF_CURVE) and not GK.on_curve_host((GC.R, 1))
    assert GK.scalar_rows([1, (1 << 256) - 1]).tolist() == [[1, 0, 0, 0], [2**64 - 1] * 4]
    assert GK.point_limbs((0, 0)).tolist() == [[0] * 4] * 2 and (GK.point_limbs(GC.G) == GC.point_rows([GC.G])[0]).all()


def test_the_generated_constants_are_up_to_date():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_grumpkin_constants.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "up to date" in r.stdout, r.stdout + r.stderr


def test_the_pedersen_generators_are_on_the_curve_and_distinct():
    from bn_amd import pedersen
    gens = pedersen.generators(16, "test")
    pts = [(g.x, g.y) for g in gens]
    assert all(GC.on_curve(p) and p != GC.O and p[1] <= (GC.R - 1) // 2 for p in pts) and len(set(pts)) == 16
    assert pedersen.generators(4, "test") == gens[:4] and pedersen.generators(4, b"other")[0] != gens[0]
    h = pedersen.blind_generator()
    assert GC.on_curve((h.x, h.y)) and (h.x, h.y) not in pts
    assert "NOT Barretenberg's" in pedersen.__doc__
    # the host model of a commitment is the model's sum
    want = GC.msm(pts[:3] + [(h.x, h.y)], [5, GC.Q - 1, 0, 9])
    c = pedersen.commit_host(gens, [5, GC.Q - 1, 0], blind=9)
    assert (c.x, c.y) == want
