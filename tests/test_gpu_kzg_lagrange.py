"""The first users of the transforms over G1 on an MI355X (run with -m gpu): bn_amd.kzg.lagrange_srs (the reference string in the
Lagrange basis, without the trapdoor), commit_evals and open_all (every opening over the domain: FK20).  The Lagrange points are checked
against host integers with the trapdoor redrawn from the same seed, the commitments against commit() of the interpolated polynomial, every
proof of open_all against open() at the same point, byte for byte, and all of them against the verifier.  Beside the small sizes every
user runs once at a size whose transforms over G1 are of 2^13 points, where their twiddles and shift powers first take both table halves."""
import numpy as np
import pytest

import fr_cases as FC
import ntt_cases as NC

pytestmark = pytest.mark.gpu
N = 8
SIZES = ((3, 8), (2, 4))                                    # (log_n, n)
LENGTHS = (0, 1, 2, 5, 8)


def _draws(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(64), "little") % FC.R for _ in range(count)]


@pytest.fixture(scope="module")
def srs():
    from bn_amd import kzg
    tau = _draws(950, 1)[0]
    assert tau != 0                                                                             # then setup keeps the first draw
    return kzg.setup(N, np.random.default_rng(950)), tau


def _lagrange_at(log_n, tau):
    """L_j(tau) for the domain {w^j} by the product formula, host integers"""
    n, R = 1 << log_n, FC.R
    xs = [pow(NC.root(log_n), j, R) for j in range(n)]
    out = []
    for j in range(n):
        num = den = 1
        for k in range(n):
            if k != j:
                num = num * (tau - xs[k]) % R
                den = den * (xs[j] - xs[k]) % R
        out.append(num * pow(den, -1, R) % R)
    return out


@pytest.mark.parametrize("log_n, n", SIZES)
def test_the_lagrange_points_are_the_multiples_of_the_host_integers(srs, log_n, n):
    from bn_amd import G1, kzg
    from bn_amd.api import default_engine
    s, tau = srs
    l = kzg.lagrange_srs(s, log_n)
    assert l.log_n == log_n and l.g2_one == s.g2_one and l.tau_g2 == s.tau_g2
    assert l.g1_lagrange.shape == (n, 12) and l.g1_lagrange.dtype == np.uint64
    want = default_engine().g1_mul_base_batch(G1.one().limbs, FC.rows(_lagrange_at(log_n, tau)))
    assert l.g1_lagrange.tobytes() == want.tobytes()
    assert sum(_lagrange_at(log_n, tau)) % FC.R == 1
    with pytest.raises(ValueError, match="powers"):
        kzg.lagrange_srs(s, 4)


BIG_LOG = 13                                                # the smallest transform over G1 that takes twiddles and shift powers from both table halves
OPEN_LOG = 12                                               # open_all over this domain runs its transforms at 2^13
OPEN_AT = (0, 1, 2047, 2048, 4095)


@pytest.fixture(scope="module")
def srs_big():
    from bn_amd import kzg
    tau = _draws(951, 1)[0]
    assert tau != 0
    return kzg.setup(1 << BIG_LOG, np.random.default_rng(951)), tau


def _lagrange_closed(log_n, tau):
    """L_j(tau) = (tau^n - 1) / n * w^j / (tau - w^j), host integers"""
    n, R = 1 << log_n, FC.R
    c = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    w, out, x = NC.root(log_n), [], 1
    for _ in range(n):
        out.append(c * x % R * pow(tau - x, -1, R) % R)
        x = x * w % R
    return out


def test_the_8192_lagrange_points_are_the_multiples_of_the_closed_form(srs_big):
    from bn_amd import G1, kzg
    from bn_amd.api import default_engine
    s, tau = srs_big
    assert _lagrange_closed(3, tau) == _lagrange_at(3, tau)                                     # the closed form is the product formula
    L = _lagrange_closed(BIG_LOG, tau)
    assert sum(L) % FC.R == 1
    l = kzg.lagrange_srs(s, BIG_LOG)
    assert l.log_n == BIG_LOG and l.g1_lagrange.shape == (1 << BIG_LOG, 12)
    want = default_engine().g1_mul_base_batch(G1.one().limbs, FC.rows(L))
    assert l.g1_lagrange.tobytes() == want.tobytes(), np.nonzero((l.g1_lagrange != want).any(axis=1))[0][:8]


def test_commit_evals_of_8192_evaluations_is_commit_of_the_interpolated_polynomial(srs_big):
    from bn_amd import kzg
    s, _ = srs_big
    l = kzg.lagrange_srs(s, BIG_LOG)
    evals = _draws(961, 1 << BIG_LOG)
    coeffs = FC.rows(NC.ntt(evals, True))                                                       # interpolated on Python integers
    got, want = kzg.commit_evals(l, FC.rows(evals)), kzg.commit(s, coeffs)
    assert got == want
    assert got.normalize().limbs.tobytes() == want.normalize().limbs.tobytes()


@pytest.mark.parametrize("length", (4096, 2049))
def test_open_all_over_4096_points_gives_the_proofs_of_open_and_they_verify(srs_big, length):
    """the transforms inside open_all are of size 2^13 here: the values against the Python-integer transform, thirteen and more proofs
    against open() byte for byte, all 4096 against the verifier"""
    from bn_amd import Fr, kzg
    s, _ = srs_big
    n, R = 1 << OPEN_LOG, FC.R
    w = NC.root(OPEN_LOG)
    coeffs = _draws(980 + length, length)
    p = FC.rows(coeffs)
    ys, proofs = kzg.open_all(s, p, OPEN_LOG)
    assert len(ys) == len(proofs) == n
    assert [y.v for y in ys] == NC.ntt(coeffs + [0] * (n - length))
    rng = np.random.default_rng(990 + length)
    ms = sorted(set(OPEN_AT) | {int(m) for m in rng.choice(np.setdiff1d(np.arange(n), OPEN_AT), 8, replace=False)})
    assert len(ms) == len(OPEN_AT) + 8
    zs = [Fr(pow(w, m, R)) for m in range(n)]
    for m in ms:
        y, proof = kzg.open(s, p, zs[m])
        assert ys[m] == y, (length, m)
        assert proofs[m].limbs.tobytes() == proof.normalize().limbs.tobytes(), (length, m)
    c = kzg.commit(s, p)
    assert kzg.verify_batch(s, [c] * n, zs, ys, proofs).all(), length
    assert not kzg.verify_batch(s, [c] * n, zs, ys[1:] + ys[:1], proofs).any(), length


@pytest.mark.parametrize("log_n, n", SIZES)
def test_commit_evals_is_commit_of_the_interpolated_polynomial(srs, log_n, n):
    import bn_amd
    from bn_amd import Fr, kzg
    s, _ = srs
    l = kzg.lagrange_srs(s, log_n)
    for evals in (_draws(960 + n, n), [0] * n, [7] * n):
        coeffs = bn_amd.fr_ntt([Fr(v) for v in evals], inverse=True)
        assert [c.v for c in coeffs] == NC.ntt(evals, True)
        assert kzg.commit_evals(l, [Fr(v) for v in evals]) == kzg.commit(s, coeffs)
        assert kzg.commit_evals(l, FC.rows(evals)).limbs.tobytes() == kzg.commit(s, coeffs).normalize().limbs.tobytes()
    with pytest.raises(ValueError, match="evaluations"):
        kzg.commit_evals(l, [Fr.one()] * (n - 1))


@pytest.mark.parametrize("log_n, n", SIZES)
def test_open_all_gives_the_proofs_of_open_and_they_verify(srs, log_n, n):
    from bn_amd import Fr, G1, kzg
    s, _ = srs
    w = NC.root(log_n)
    for length in LENGTHS:
        if length > n:
            with pytest.raises(ValueError, match="domain"):
                kzg.open_all(s, [Fr.one()] * length, log_n)
            continue
        p = [Fr(v) for v in _draws(970 + 10 * n + length, length)]
        ys, proofs = kzg.open_all(s, p, log_n)
        assert len(ys) == len(proofs) == n
        zs = [Fr(pow(w, m, FC.R)) for m in range(n)]
        for m in range(n):
            y, proof = kzg.open(s, p, zs[m])
            assert ys[m] == y, (n, length, m)
            assert proofs[m].limbs.tobytes() == proof.normalize().limbs.tobytes(), (n, length, m)
        if length <= 1:
            assert all(pr == G1.zero() for pr in proofs)
        c = kzg.commit(s, p)
        assert kzg.verify_batch(s, [c] * n, zs, ys, proofs).all(), (n, length)
        if length >= 2:
            assert not kzg.verify_batch(s, [c] * n, zs, ys[1:] + ys[:1], proofs).any(), (n, length)
