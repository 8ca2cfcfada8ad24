"""Poseidon over Fr: the circomlib / iden3 instance (S-box x^5, width t = arity + 1 for arity 1 .. 4, R_F = 8 and R_P = 56 / 57 / 56 / 60 for
t = 2 / 3 / 4 / 5), its constants from the Grain LFSR of the Poseidon paper, the permutation and the hash in host integers, and the hash on
the GPU (bn_amd.fr_poseidon_batch).

This module is the single source of the constants: tools/gen_poseidon_constants.py writes bn_amd/csrc/poseidon_constants.hpp from
constants(t), and nothing is downloaded or stored - the published known answers (hash(1, 2) = 7853200120776062878684798364095072458815029376092732009249414926327459813530)
come out of the derivation below.

    hash(x_1 .. x_arity) = permute([0, x_1, .., x_arity])[0]
    one round: add the t round constants C[round * t + i]; S-box on every element (first and last R_F / 2 rounds) or on element 0 only (the R_P
    rounds between); new[i] = sum_j M[i][j] * s[j]"""
import functools

from .api import R_MOD, Fr, _scalar_array, default_engine

R_F = 8
R_P = {2: 56, 3: 57, 4: 56, 5: 60, 6: 60}      # width 6 is the challenge of EdDSA-Poseidon (bn_amd.eddsa): host functions and its own device calls only
ARITY_MAX = 4


class _Grain:
    """The 80-bit LFSR of the Poseidon paper (appendix F): start bits, most significant first, 1 in 2 bits (a prime field), 0 in 4 bits (the
    S-box x^alpha), the field size in 12 bits, t in 12, R_F in 10, R_P in 10, thirty ones; the first 160 outputs are discarded."""

    def __init__(self, t, r_f, r_p, field_bits=254):
        bits = []
        for value, width in ((1, 2), (0, 4), (field_bits, 12), (t, 12), (r_f, 10), (r_p, 10), ((1 << 30) - 1, 30)):
            bits += [(value >> (width - 1 - i)) & 1 for i in range(width)]
        assert len(bits) == 80
        self.b = bits
        for _ in range(160):
            self._step()

    def _step(self):
        b = self.b
        new = b[62] ^ b[51] ^ b[38] ^ b[23] ^ b[13] ^ b[0]
        b.pop(0)
        b.append(new)
        return new

    def bit(self):
        """one stream bit: outputs are taken in pairs, and a pair whose first bit is 0 is thrown away"""
        while self._step() == 0:
            self._step()
        return self._step()

    def draw(self, nbits=254):
        v = 0
        for _ in range(nbits):
            v = v << 1 | self.bit()
        return v


@functools.lru_cache(maxsize=None)
def constants(t):
    """(C, M) of width t = 2 .. 6 as Python integers: C the (R_F + R_P) * t round constants in round order, M the t x t Cauchy matrix as a
    tuple of rows, M[i][j] = 1 / (xs[i] + ys[j])"""
    if t not in R_P:
        raise ValueError(f"Poseidon width t = {t}: 2 .. 6 are defined")
    g = _Grain(t, R_F, R_P[t])
    C = []
    while len(C) < (R_F + R_P[t]) * t:
        v = g.draw()
        if v < R_MOD:                        # rejection sampling: a draw at or above r is skipped
            C.append(v)
    xy = [g.draw() % R_MOD for _ in range(2 * t)]          # the matrix draws are reduced, not rejected
    xs, ys = xy[:t], xy[t:]
    # the first attempt is good at all five widths (distinct values, no zero sum): there is no retry
    assert len(set(xy)) == 2 * t and all((x + y) % R_MOD for x in xs for y in ys), "the Cauchy draw of this width needs the retry this module does not have"
    M = tuple(tuple(pow(x + y, -1, R_MOD) for y in ys) for x in xs)
    return tuple(C), M


def permute_host(state):
    """the permutation of a list of t = 2 .. 6 integers mod r, in host integers -> list of t integers"""
    s = [int(x) % R_MOD for x in state]
    t = len(s)
    C, M = constants(t)
    half = R_F // 2
    for rnd in range(R_F + R_P[t]):
        s = [(x + C[rnd * t + i]) % R_MOD for i, x in enumerate(s)]
        if rnd < half or rnd >= half + R_P[t]:
            s = [pow(x, 5, R_MOD) for x in s]
        else:
            s[0] = pow(s[0], 5, R_MOD)
        s = [sum(M[i][j] * s[j] for j in range(t)) % R_MOD for i in range(t)]
    return s


def hash_host(inputs):
    """hash of 1 .. 4 integers mod r, in host integers -> integer"""
    inputs = list(inputs)
    if not 1 <= len(inputs) <= ARITY_MAX:
        raise ValueError(f"Poseidon hashes 1 .. {ARITY_MAX} inputs, not {len(inputs)}")
    return permute_host([0] + inputs)[0]


def hash(inputs, engine=None):
    """hash of 1 .. 4 Fr on the GPU -> Fr (one lane; hash many with bn_amd.fr_poseidon_batch)"""
    x = _scalar_array(inputs)
    if not 1 <= x.shape[0] <= ARITY_MAX:
        raise ValueError(f"Poseidon hashes 1 .. {ARITY_MAX} inputs, not {x.shape[0]}")
    return Fr.from_limbs((engine or default_engine()).fr_poseidon_batch(x.reshape(1, x.shape[0], 4))[0])
