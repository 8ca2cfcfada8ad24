"""Pedersen commitments and the inner-product argument over Grumpkin on an MI355X (run with -m gpu): bn_amd.pedersen against the integer model
of tests/grumpkin_cases.py, and bn_amd.ipa's proofs accepted, tampered proofs rejected, with the number of device calls it promises."""
import numpy as np
import pytest

import grumpkin_cases as GC

pytestmark = pytest.mark.gpu


class Counting:
    """an engine that counts the segmented sums it is asked for: (terms, segments) per call"""
    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def grumpkin_msm_batch(self, p, k, offsets):
        self.calls.append((len(p), len(offsets) - 1))
        return self.eng.grumpkin_msm_batch(p, k, offsets)


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own, destroyed when the module is done: the process keeps none of its streams"""
    import bn_amd
    e = bn_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gens():
    from bn_amd import pedersen
    return pedersen.generators(8, "bn_amd.test")


def _model(points, ks):
    from bn_amd import grumpkin as GK
    return GK.Point(*GC.msm([(p.x, p.y) for p in points], ks))


def test_commit_against_the_model(eng, gens):
    from bn_amd import pedersen
    rng = np.random.default_rng(5)
    vals = [0, 1, GC.Q - 1] + [GC.rand256(rng) % GC.Q for _ in range(5)]
    c = Counting(eng)
    assert pedersen.commit(gens, vals, engine=c) == _model(gens, vals) == pedersen.commit_host(gens, vals) and c.calls == [(8, 1)]
    h = pedersen.blind_generator()
    assert pedersen.commit(gens, vals, blind=77, engine=c) == _model(gens + [h], vals + [77]) and c.calls[-1] == (9, 1)
    assert pedersen.commit(gens, vals, blind=77, h=gens[0], engine=c) == _model(gens + [gens[0]], vals + [77])
    assert pedersen.commit(gens, [], engine=c) == _model([], [])                                     # no values: O
    with pytest.raises(ValueError):
        pedersen.commit(gens, [1] * 9, engine=c)


def test_commit_batch_is_one_call(eng, gens):
    from bn_amd import pedersen
    rng = np.random.default_rng(6)
    vecs = [[GC.rand256(rng) % GC.Q for _ in range(5)] for _ in range(3)]
    c = Counting(eng)
    got = pedersen.commit_batch(gens, vecs, engine=c)
    assert got == [_model(gens[:5], v) for v in vecs] and c.calls == [(15, 3)]
    got = pedersen.commit_batch(gens, vecs, blinds=[1, 2, 3], engine=c)
    h = pedersen.blind_generator()
    assert got == [_model(gens[:5] + [h], v + [b]) for v, b in zip(vecs, (1, 2, 3))] and c.calls[-1] == (18, 3)


@pytest.mark.parametrize("n", [8, 1])
def test_the_inner_product_argument(eng, gens, n):
    from bn_amd import grumpkin as GK, ipa, pedersen
    rng = np.random.default_rng(7 + n)
    a = [GC.rand256(rng) % GC.Q for _ in range(n)]; b = [GC.rand256(rng) % GC.Q for _ in range(n)]
    g, u = gens[:n], pedersen.generators(1, "bn_amd.test.u")[0]
    c = Counting(eng)
    proof = ipa.prove(g, u, a, b, ipa.Transcript("t"), engine=c)
    k = n.bit_length() - 1
    assert len(proof.L) == len(proof.R) == k
    # the statement's commitment, then per round ONE call of two segments for L and R and ONE of n / 2 two-term segments for the generators
    want_calls = [(n + 1, 1)]
    for j in range(k):
        h = n >> (j + 1)
        want_calls += [(2 * h + 2, 2), (2 * h, h)]
    assert c.calls == want_calls
    C = ipa.commitment(g, u, a, b, engine=eng)
    assert C == _model(g + [u], a + [sum(x * y for x, y in zip(a, b)) % GC.Q])
    c.calls.clear()
    assert ipa.verify(g, u, C, proof, ipa.Transcript("t"), engine=c) is True
    assert c.calls == [(n, 1), (2 * k + 3, 2)]                                                        # the folded generator over s, then the two sides
    assert ipa.verify(g, u, C, proof, ipa.Transcript("t"), b=b, engine=eng) is True
    assert ipa.verify(g, u, C, proof, ipa.Transcript("t"), b=[(b[0] + 1) % GC.Q] + b[1:], engine=eng) is False
    # rejected: another transcript, a_final + 1, b_final + 1, another commitment, an L replaced by G
    assert ipa.verify(g, u, C, proof, ipa.Transcript("other"), engine=eng) is (k == 0)                # without rounds no challenge is drawn
    assert ipa.verify(g, u, C, proof._replace(a_final=(proof.a_final + 1) % GC.Q), ipa.Transcript("t"), engine=eng) is False
    assert ipa.verify(g, u, C, proof._replace(b_final=(proof.b_final + 1) % GC.Q), ipa.Transcript("t"), engine=eng) is False
    assert ipa.verify(g, u, C + GK.Point.generator(), proof, ipa.Transcript("t"), engine=eng) is False
    if k:
        bad = proof._replace(L=[GK.Point.generator()] + proof.L[1:])
        assert ipa.verify(g, u, C, bad, ipa.Transcript("t"), engine=eng) is False
        assert ipa.verify(g, u, C, proof._replace(R=proof.R[:-1]), ipa.Transcript("t"), engine=eng) is False
    with pytest.raises(ValueError):
        ipa.prove(gens[:3], u, [1, 2, 3], [1, 2, 3], ipa.Transcript("t"), engine=eng)
