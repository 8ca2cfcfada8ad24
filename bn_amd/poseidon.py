"""Poseidon over Fr: the circomlib / iden3 instance (S-box x^5, width t = arity + 1 for arity 1 .. 4, R_F = 8 and R_P = 56 / 57 / 56 / 60 for
t = 2 / 3 / 4 / 5), its constants from the Grain LFSR of the Poseidon paper, the permutation and the hash in host integers, and the hash on
the GPU (bn_amd.fr_poseidon_batch).

This module is the single source of the constants: tools/gen_poseidon_constants.py writes bn_amd/csrc/poseidon_constants.hpp from
constants(t), and nothing is downloaded or stored - the published known answers (hash(1, 2) = 7853200120776062878684798364095072458815029376092732009249414926327459813530)
come out of the derivation below.

    hash(x_1 .. x_arity) = permute([0, x_1, .., x_arity])[0]
    one round: add the t round constants C[round * t + i]; S-box on every element (first and last R_F / 2 rounds) or on element 0 only (the R_P
    rounds between); new[i] = sum_j M[i][j] * s[j]

The wide forms reach every width circomlib defines, t = 2 .. 17 (R_P below): hash_ex / hash_ex_host are circomlib's PoseidonEx(n_inputs, n_outs)
with an initial state for 1 .. 16 inputs, hash_chain / hash_chain_host digest a record of any length by chaining PoseidonEx(rate, 1) through
that state - this package's own framing.  On the GPU they are bn_amd.fr_poseidon_ex_batch and bn_amd.fr_poseidon_chain_batch, in which several
lanes share one permutation and the constants are derived on the host at the first use of a width (bn_amd/csrc/poseidon_wide_table.hpp restates
constants() below; the tests compare every element).  hash, hash_host and ARITY_MAX are what they were."""
import functools

from .api import R_MOD, Fr, _scalar_array, default_engine

R_F = 8
# widths 2 .. 5 are the public hash (ARITY_MAX), width 6 also the challenge of EdDSA-Poseidon (bn_amd.eddsa), and all of 2 .. 17 the wide calls
# (hash_ex, hash_chain: bn_amd.fr_poseidon_ex_batch and bn_amd.fr_poseidon_chain_batch), which circomlib defines for 1 .. 16 inputs
R_P = dict(zip(range(2, 18), (56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68)))
ARITY_MAX = 4
EX_INPUTS_MAX = 16


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
    """(C, M) of width t = 2 .. 17 as Python integers: C the (R_F + R_P) * t round constants in round order, M the t x t Cauchy matrix as a
    tuple of rows, M[i][j] = 1 / (xs[i] + ys[j])"""
    if t not in R_P:
        raise ValueError(f"Poseidon width t = {t}: 2 .. 17 are defined")
    g = _Grain(t, R_F, R_P[t])
    C = []
    while len(C) < (R_F + R_P[t]) * t:
        v = g.draw()
        if v < R_MOD:                        # rejection sampling: a draw at or above r is skipped
            C.append(v)
    xy = [g.draw() % R_MOD for _ in range(2 * t)]          # the matrix draws are reduced, not rejected
    xs, ys = xy[:t], xy[t:]
    # the first attempt is good at all sixteen widths (distinct values, no zero sum): there is no retry
    assert len(set(xy)) == 2 * t and all((x + y) % R_MOD for x in xs for y in ys), "the Cauchy draw of this width needs the retry this module does not have"
    M = tuple(tuple(pow(x + y, -1, R_MOD) for y in ys) for x in xs)
    return tuple(C), M


def permute_host(state):
    """the permutation of a list of t = 2 .. 17 integers mod r, in host integers -> list of t integers"""
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


def hash_ex_host(inputs, init=0, n_outs=1):
    """circomlib's PoseidonEx in host integers: the first n_outs elements of permute([init, x_1, .., x_n]) for 1 .. 16 inputs -> list of n_outs
    integers (1 <= n_outs <= n + 1).  hash_ex_host(x)[0] is hash_host(x) where that is defined."""
    inputs = list(inputs)
    if not 1 <= len(inputs) <= EX_INPUTS_MAX:
        raise ValueError(f"PoseidonEx takes 1 .. {EX_INPUTS_MAX} inputs, not {len(inputs)}")
    if not 1 <= n_outs <= len(inputs) + 1:
        raise ValueError(f"n_outs = {n_outs}: 1 .. {len(inputs) + 1} for {len(inputs)} inputs")
    return permute_host([init] + inputs)[:n_outs]


def chain_blocks(length, rate):
    """blocks of `rate` elements a record of `length` elements is cut into: max(1, ceil(length / rate))"""
    return max(1, -(-length // rate))


def hash_chain_host(values, rate=16):
    """This package's own framing of a record of any length (no other library's format, and not an additive sponge): c = len(values); the
    record is cut into max(1, ceil(len / rate)) blocks of `rate` elements, the last padded with zeros (an empty record is one block of zeros);
    per block c = permute([c, block..])[0] at width rate + 1 - PoseidonEx(rate, 1) chained through its initialState -> integer"""
    values = [int(v) % R_MOD for v in values]
    if not 1 <= rate <= EX_INPUTS_MAX:
        raise ValueError(f"rate = {rate}: 1 .. {EX_INPUTS_MAX}")
    c = len(values) % R_MOD
    padded = values + [0] * (chain_blocks(len(values), rate) * rate - len(values))
    for at in range(0, len(padded), rate):
        c = permute_host([c] + padded[at:at + rate])[0]
    return c


def hash_ex(inputs, init=0, n_outs=1, engine=None):
    """PoseidonEx of 1 .. 16 Fr on the GPU -> list of n_outs Fr (one permutation; hash many with bn_amd.fr_poseidon_ex_batch)"""
    import numpy as np
    x = _scalar_array(inputs)
    if not 1 <= x.shape[0] <= EX_INPUTS_MAX:
        raise ValueError(f"PoseidonEx takes 1 .. {EX_INPUTS_MAX} inputs, not {x.shape[0]}")
    if not 1 <= n_outs <= x.shape[0] + 1:
        raise ValueError(f"n_outs = {n_outs}: 1 .. {x.shape[0] + 1} for {x.shape[0]} inputs")
    init = init if isinstance(init, Fr) else Fr(init)
    out = (engine or default_engine()).fr_poseidon_ex_batch(x.reshape(1, x.shape[0], 4), _scalar_array([init]), n_outs)
    return [Fr.from_limbs(r) for r in np.asarray(out).reshape(n_outs, 4)]


def hash_chain(values, rate=16, engine=None):
    """hash_chain_host on the GPU -> Fr (one record; hash many with bn_amd.fr_poseidon_chain_batch)"""
    import numpy as np
    if not 1 <= rate <= EX_INPUTS_MAX:
        raise ValueError(f"rate = {rate}: 1 .. {EX_INPUTS_MAX}")
    values = list(values)
    x = _scalar_array(values) if values else np.zeros((0, 4), np.uint64)
    return Fr.from_limbs((engine or default_engine()).fr_poseidon_chain_batch(x, [0, x.shape[0]], rate)[0])
