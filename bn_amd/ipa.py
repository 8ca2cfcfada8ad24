"""The Bulletproofs inner-product argument over Grumpkin (bn_amd.grumpkin) for vectors of n = 2^k entries: a proof of 2 k points and two scalars
that the prover knows a and b with

    C = sum of [a_i] G_i + [<a, b>] u                                          (commitment(gens, u, a, b))

When the verifier knows b - the powers of an evaluation point, as in the polynomial commitments of Halo-style systems - it passes it to
verify(), which then also checks the b the proof ends with; without it the argument shows knowledge of an opening of C over (G, u).

Scalars are Python integers mod q, the group order; the inner products, the folds of a and b and the challenge inverses are host arithmetic.
Every sum of points is a bn_amd.grumpkin_msm_batch: per round L and R are ONE call of two segments and the fold of the generators ONE call of
n / 2 two-term segments; the verifier folds the generators with one sum over the vector s of challenge products.

    round over halves (lo, hi):  L = <a_lo, G_hi> + [<a_lo, b_hi>] u,  R = <a_hi, G_lo> + [<a_hi, b_lo>] u,  x = challenge(L, R)
    a' = x a_lo + x^-1 a_hi,  b' = x^-1 b_lo + x b_hi,  G' = [x^-1] G_lo + [x] G_hi,  C' = [x^2] L + C + [x^-2] R
    at n = 1:  C == [a] G_0 + [a b] u

THE TRANSCRIPT AND THE GENERATORS ARE THIS PROJECT'S OWN (bn_amd.pedersen.generators; the SHA-256 chain of bn_amd.sumcheck.Transcript with the
challenge reduced mod q instead of mod r): proofs made here verify here and nowhere else.  The exact bytes: start state = SHA256(label);
the statement absorbs n, then C and u; a point is absorbed as its two coordinates, 32 bytes each, big endian (O as zeros); a challenge is
int(SHA256(state || 0x00) || SHA256(state || 0x01)) mod q, drawn again while it is zero, and the state ratchets as in sumcheck.Transcript."""
import collections
import hashlib

from . import grumpkin as GK
from . import sumcheck

Proof = collections.namedtuple("Proof", "L R a_final b_final")
Proof.__doc__ = "L, R: k grumpkin.Point each, one pair per round; a_final, b_final: the folded vectors' last entries, integers mod q"


class Transcript(sumcheck.Transcript):
    """sumcheck.Transcript over Grumpkin: points and integers go in, challenges come out mod q"""

    def absorb_ints(self, xs):
        self.state = hashlib.sha256(self.state + b"".join(int(x).to_bytes(32, "big") for x in xs)).digest()

    def absorb_points(self, pts):
        self.absorb_ints([c for p in pts for c in (p.x, p.y)])

    def challenge(self):
        while True:
            x = int.from_bytes(hashlib.sha256(self.state + b"\x00").digest() + hashlib.sha256(self.state + b"\x01").digest(), "big") % GK.Q
            self.state = hashlib.sha256(self.state + b"\x02").digest()
            if x:
                return x


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % GK.Q


def _check_size(gens, n):
    if n < 1 or n & (n - 1) or len(gens) != n:
        raise ValueError(f"the vectors and the generators need the same power-of-two length, got {n} and {len(gens)}")


def commitment(gens, u, a, b, engine=None):
    """sum of [a_i] gens[i] + [<a, b>] u -> grumpkin.Point: one grumpkin_msm_batch of one segment"""
    a = [int(x) % GK.Q for x in a]; b = [int(x) % GK.Q for x in b]
    return GK.grumpkin_msm_batch(list(gens) + [u], a + [_dot(a, b)], [0, len(a) + 1], engine=engine)[0]


def prove(gens, u, a, b, transcript, engine=None):
    """Proof that commitment(gens, u, a, b) opens to (a, b).  gens: n = 2^k grumpkin.Point; u: a grumpkin.Point; a, b: n integers mod q;
    transcript: an ipa.Transcript, advanced as verify() will advance its own"""
    a = [int(x) % GK.Q for x in a]; b = [int(x) % GK.Q for x in b]; g = list(gens)
    n = len(a)
    _check_size(g, n)
    if len(b) != n:
        raise ValueError(f"{n} entries of a, {len(b)} of b")
    transcript.absorb_ints([n])
    transcript.absorb_points([commitment(g, u, a, b, engine=engine), u])
    Ls, Rs = [], []
    while n > 1:
        h = n // 2
        a_lo, a_hi, b_lo, b_hi, g_lo, g_hi = a[:h], a[h:], b[:h], b[h:], g[:h], g[h:]
        L, R = GK.grumpkin_msm_batch(g_hi + [u] + g_lo + [u], a_lo + [_dot(a_lo, b_hi)] + a_hi + [_dot(a_hi, b_lo)], [0, h + 1, 2 * h + 2], engine=engine)
        transcript.absorb_points([L, R])
        x = transcript.challenge(); xi = pow(x, -1, GK.Q)
        a = [(x * lo + xi * hi) % GK.Q for lo, hi in zip(a_lo, a_hi)]
        b = [(xi * lo + x * hi) % GK.Q for lo, hi in zip(b_lo, b_hi)]
        g = GK.grumpkin_msm_batch([p for pair in zip(g_lo, g_hi) for p in pair], [xi, x] * h, list(range(0, 2 * h + 1, 2)), engine=engine)
        Ls.append(L); Rs.append(R); n = h
    return Proof(Ls, Rs, a[0], b[0])


def verify(gens, u, commitment, proof, transcript, b=None, engine=None):
    """True iff the proof opens `commitment` over (gens, u) - and, when the verifier's own b is given, ends with that vector's fold"""
    g = list(gens); n = len(g)
    _check_size(g, n)
    k = n.bit_length() - 1
    if len(proof.L) != k or len(proof.R) != k or not 0 <= proof.a_final < GK.Q or not 0 <= proof.b_final < GK.Q:
        return False
    transcript.absorb_ints([n])
    transcript.absorb_points([commitment, u])
    xs = []
    for L, R in zip(proof.L, proof.R):
        transcript.absorb_points([L, R])
        xs.append(transcript.challenge())
    xis = [pow(x, -1, GK.Q) for x in xs]
    # s_i: round j halves on bit k - 1 - j of i; the upper half took x_j, the lower x_j^-1
    s = []
    for i in range(n):
        v = 1
        for j in range(k):
            v = v * (xs[j] if (i >> (k - 1 - j)) & 1 else xis[j]) % GK.Q
        s.append(v)
    if b is not None:
        if len(b) != n or _dot(s, b) != proof.b_final:       # b folds with the same products as the generators
            return False
    g_final = GK.grumpkin_msm_batch(g, s, [0, n], engine=engine)[0]
    lhs_pts = [commitment] + list(proof.L) + list(proof.R)
    lhs_ks = [1] + [x * x % GK.Q for x in xs] + [xi * xi % GK.Q for xi in xis]
    lhs, rhs = GK.grumpkin_msm_batch(lhs_pts + [g_final, u], lhs_ks + [proof.a_final, proof.a_final * proof.b_final % GK.Q], [0, len(lhs_pts), len(lhs_pts) + 2], engine=engine)
    return lhs == rhs
