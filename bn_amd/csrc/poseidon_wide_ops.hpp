// The bodies of the wide Poseidon kernels (bn254_poseidon_wide.hip): bn254_fr_poseidon_ex_batch, bn254_fr_poseidon_chain_batch and their _dev twins.
// The instance of poseidon_ops.hpp at every width circomlib defines, t = 2 .. 17 (R_P and the tables: poseidon_wide_table.hpp).  The one-lane
// kernels keep the state in registers with compile-time indices and the matrix as literals; at t = 17 that is 289 literal products per round
// and 272 VGPRs of state, so here G lanes (4, 8 or 16; never across a wave) share one permutation:
//   * lane g of the group owns the state elements g, g + G, .. below t (at most ceil(17 / G));
//   * the state lives in an EXCHANGE BUFFER (LDS on the device, a plain array in the host simulation), two copies `cur` and `cur ^ 1`;
//   * a round is two phases.  add+sbox+publish: every lane adds the round constant to the elements it owns, raises them to the fifth power
//     (full round: all; partial round: element 0 only, so only its owner) and writes them back to `cur`.  rows: every lane reads the whole
//     state from `cur` and writes its own rows of M s to `cur ^ 1`.  Then the copies swap.  Between two phases the lanes of a group must all
//     have finished: Lanes::phase is that boundary (device: the lanes of a wave run in lockstep, so a wave-scope wait and a compiler barrier -
//     never a workgroup barrier, the groups of a wave run different numbers of blocks in the chain call; host: a loop over the group's lanes);
//   * t is a run-time value: the loops over rounds, elements and row chunks stay loops, the code exists once per G and not per width;
//   * a row of t terms is ceil(t / 5) fr_dot calls of at most five pairs (fr.hpp: sound while 5 r < 2^256) joined by fr_add; every partial
//     result is canonical, so the bytes depend neither on G nor on how a row is cut;
//   * round constants and matrix rows are read from the device table of the width (vector loads: the addresses differ by lane; a width's
//     matrix is at most 9 KB and stays in the vector cache), not from an LDS copy: a copy would need a workgroup barrier after it is filled
//     and would take the LDS the exchange buffers of more resident waves use.
// Everything takes plain pointers, so the host simulation (tests/hostsim/hostsim_poseidon_wide.cpp) runs the very same bodies.
#pragma once
#include "fr_ops.hpp"
#include "poseidon_wide_table.hpp"

// lanes per permutation of the shipped kernels: the smallest median of five runs of bn254_fr_poseidon_ex_batch_dev over 2^16 rows of 16
// inputs among 4 / 8 / 16 (the rule was fixed before measuring; tools/time_poseidon_wide.py, profiles/r27_poseidon_wide.txt)
#ifndef BN254_POSEIDON_WIDE_LANES
#define BN254_POSEIDON_WIDE_LANES 8
#endif

// the phases are lambdas handed to Lanes::phase: on the device they are inlined like every other body
#if defined(BN_HOSTSIM)
#define BN_PSDW_INLINE
#else
#define BN_PSDW_INLINE __attribute__((always_inline))
#endif

namespace bn254 {

constexpr int PSDW_T_MAX = psdw::T_MAX;
// words of the exchange buffers of one group: two copies of up to 17 records
constexpr int PSDW_GROUP_WORDS = 2 * PSDW_T_MAX * 8;

// Word w of element e of copy `buf` is base[((buf * 17 + e) * 8 + w) * stride].  Device: base = the workgroup's LDS array + the group's index
// in the workgroup, stride = groups per workgroup, so the lanes of one group read one address (a broadcast) and the groups of a wave read
// consecutive banks.  Host: stride 1.
struct PsdwExchange {
    uint32_t *base;
    uint32_t stride;
    BN_FN Fr get(int buf, int e) const {
        Fr r;
        const uint32_t *p = base + (size_t)((buf * PSDW_T_MAX + e) * 8) * stride;
#pragma unroll
        for (int w = 0; w < 8; ++w) r.w[w] = p[(size_t)w * stride];
        return r;
    }
    BN_FN void put(int buf, int e, const Fr &a) const {
        uint32_t *p = base + (size_t)((buf * PSDW_T_MAX + e) * 8) * stride;
#pragma unroll
        for (int w = 0; w < 8; ++w) p[(size_t)w * stride] = a.w[w];
    }
};

BN_FN Fr psdw_pow5(const Fr &x) {
    const Fr x2 = fr_mul(x, x);
    return fr_mul(fr_mul(x2, x2), x);
}
// the Montgomery image of the integer v < 2^64
BN_FN Fr psdw_from_u64(uint64_t v) {
    Fr raw = fr_zero();
    raw.w[0] = (uint32_t)v; raw.w[1] = (uint32_t)(v >> 32);
    return fr_mul(raw, fr_const(k::FR_R2_32));
}

// ---- the phases, for lane g of a group of G lanes
// add + sbox + publish, round `round` of width t; C: the round constants of the width
BN_FN void psdw_add_sbox(const PsdwExchange &ex, int cur, int g, int G, int t, const uint32_t *C, int round, bool full) {
#pragma unroll 1
    for (int e = g; e < t; e += G) {
        Fr x = fr_add(ex.get(cur, e), fr_load(C, (size_t)(round * t + e)));
        if (full || e == 0) x = psdw_pow5(x);
        ex.put(cur, e, x);
    }
}
// K <= 5 terms of a row: sum_q s[j0 + q] * m[q]
template <int K>
BN_FN Fr psdw_row_chunk(const PsdwExchange &ex, int cur, int j0, const uint32_t *m) {
    Fr a[K];
#pragma unroll
    for (int q = 0; q < K; ++q) a[q] = ex.get(cur, j0 + q);
    return fr_dot<K>(a, (const uint32_t (*)[8])m);
}
// rows g, g + G, .. of M s, read from `cur`, written to `cur ^ 1`; M: the matrix of the width, row-major
BN_FN void psdw_rows(const PsdwExchange &ex, int cur, int g, int G, int t, const uint32_t *M) {
#pragma unroll 1
    for (int i = g; i < t; i += G) {
        Fr acc = fr_zero();
#pragma unroll 1
        for (int j0 = 0; j0 < t; j0 += 5) {
            const uint32_t *m = M + (size_t)(i * t + j0) * 8;
            const int cnt = t - j0 < 5 ? t - j0 : 5;
            Fr part;
            switch (cnt) {
            case 1: part = psdw_row_chunk<1>(ex, cur, j0, m); break;
            case 2: part = psdw_row_chunk<2>(ex, cur, j0, m); break;
            case 3: part = psdw_row_chunk<3>(ex, cur, j0, m); break;
            case 4: part = psdw_row_chunk<4>(ex, cur, j0, m); break;
            default: part = psdw_row_chunk<5>(ex, cur, j0, m); break;
            }
            acc = j0 ? fr_add(acc, part) : part;
        }
        ex.put(cur ^ 1, i, acc);
    }
}

// ---- the programs of a group.  `Lanes` runs one phase for the lane(s) it stands for and ends it with the boundary described above:
//      lanes.phase(f) calls f(g) and has G = Lanes::G.
// the permutation of width t on the state in copy `cur`; returns the copy that holds the result.  rp: R_P of the width (the host's psdw::R_P[t]: a
// kernel argument), tbl: the table of the width
template <class Lanes>
BN_FN int psdw_permute(const PsdwExchange &ex, int cur, int t, int rp, const uint32_t *tbl, const Lanes &lanes) {
    const int half = psdw::R_F / 2, rounds = psdw::R_F + rp;
    const uint32_t *const C = tbl, *const M = tbl + (size_t)rounds * t * 8;
#pragma unroll 1
    for (int round = 0; round < rounds; ++round) {
        const bool full = round < half || round >= half + rp;
        lanes.phase([&](int g) BN_PSDW_INLINE { psdw_add_sbox(ex, cur, g, Lanes::G, t, C, round, full); });
        lanes.phase([&](int g) BN_PSDW_INLINE { psdw_rows(ex, cur, g, Lanes::G, t, M); });
        cur ^= 1;
    }
    return cur;
}
// PoseidonEx, row p: state [init ? init[p] : 0, in[p * n_inputs] ..], out[p * n_outs + j] = permute(state)[j]
template <class Lanes>
BN_FN void psdw_ex_body(const PsdwExchange &ex, const uint32_t *in, int n_inputs, const uint32_t *init, int n_outs, uint32_t *out, size_t p, int rp, const uint32_t *tbl,
                        const Lanes &lanes) {
    const int t = n_inputs + 1;
    lanes.phase([&](int g) BN_PSDW_INLINE {
#pragma unroll 1
        for (int e = g; e < t; e += Lanes::G)
            ex.put(0, e, e ? fr_load(in, p * (size_t)n_inputs + (size_t)(e - 1)) : (init ? fr_load(init, p) : fr_zero()));
    });
    const int cur = psdw_permute(ex, 0, t, rp, tbl, lanes);
    lanes.phase([&](int g) BN_PSDW_INLINE {
#pragma unroll 1
        for (int e = g; e < n_outs; e += Lanes::G) fr_store(ex.get(cur, e), out, p * (size_t)n_outs + (size_t)e);
    });
}
// the chain, record j = elements [first, first + len) of `in`: c = Fr(len); per block of `rate` elements (the last padded with zeros, an empty
// record is one block of zeros) c = permute([c, block..])[0]; out[j] = c.  The number of blocks is the group's own.
template <class Lanes>
BN_FN void psdw_chain_body(const PsdwExchange &ex, const uint32_t *in, uint64_t first, uint64_t len, int rate, uint32_t *out, size_t j, int rp, const uint32_t *tbl,
                           const Lanes &lanes) {
    const int t = rate + 1;
    const uint64_t blocks = len ? (len + (uint64_t)rate - 1) / (uint64_t)rate : 1;
    int cur = 0;
    lanes.phase([&](int g) BN_PSDW_INLINE { if (g == 0) ex.put(0, 0, psdw_from_u64(len)); });
#pragma unroll 1
    for (uint64_t b = 0; b < blocks; ++b) {
        lanes.phase([&](int g) BN_PSDW_INLINE {
#pragma unroll 1
            for (int e = g ? g : Lanes::G; e < t; e += Lanes::G) {               // element 0 is the running value
                const uint64_t pos = b * (uint64_t)rate + (uint64_t)(e - 1);
                ex.put(cur, e, pos < len ? fr_load(in, (size_t)(first + pos)) : fr_zero());
            }
        });
        cur = psdw_permute(ex, cur, t, rp, tbl, lanes);
    }
    lanes.phase([&](int g) BN_PSDW_INLINE { if (g == 0) fr_store(ex.get(cur, 0), out, j); });
}

}  // namespace bn254
