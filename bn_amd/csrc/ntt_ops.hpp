// The per-lane bodies of the number-theoretic transform over Fr (bn254_ntt.hip: bn254_fr_ntt_batch and its _dev twin).  A transform of
// n = 2^log_n elements is a few passes over global memory (host_plan.hpp bn_ntt_plan); a pass is one step of a Stockham autosort of radix
// R = 2^t, so the data are in natural order before the first and after the last pass and no pass reverses bits in global memory:
//     y[q + s (R p + k)] = w_n'^(p k) * sum_j x[q + s (p + m j)] w_R^(j k)       n' = R m the current length, s = n / n' the stride,
//                                                                                 p < m, q < s, j, k < R
// The R inputs of one such "small transform" lie n / R apart, and the small transforms u = q + s p = 0 .. n / R - 1 start at consecutive
// records: a workgroup takes C = 2^(T - t) consecutive ones, 2^T elements in all, so a row of its tile is a run of C adjacent records.  It
// runs the t radix-2 stages (decimation in frequency, the result bit-reversed INSIDE the tile) in LDS, and the store undoes the reversal,
// applies the twiddle w_n'^(p k) and - in the last pass of an inverse or coset transform - the factor n^-1 s^-j; the first pass of a forward
// coset transform multiplies its inputs by s^j.
// Twiddles (factored scheme): ONE table pair for every size and both directions, w_24^i for i < 2^12 and w_24^(2^12 i) for i < 2^12 (w_24 the
// root of the largest size, the smaller domains nest in it; w^-e = w^(2^24 - e)).  A stage's twiddle w_R^e = w_24^(e 2^(24 - t)) has no low
// part for t <= 12: one load, no product - a workgroup copies the R / 2 of its pass to LDS once.  The twiddle between passes is two loads and a product.  The powers of the shift come from a
// second pair of the same shape: s^i for a forward transform (keyed by the shift alone), n^-1 s^-i for an inverse one (shift and size).
// Everything is pure and written per lane as (pass, tile pointer, workgroup, lane, stage): the kernel calls the functions between
// __syncthreads(), the host simulation (tests/hostsim/hostsim_ntt.cpp) in a loop over lanes.
#pragma once
#include "fr_ops.hpp"

namespace bn254 {

constexpr uint32_t NTT_BLOCK = 256;            // lanes of a workgroup
// shipped T: a tile of 2^T elements is 32 << T bytes of LDS, its stage twiddles up to half as much again.  The run-time override of
// bn254_ntt.hip only goes DOWN from it, so the sweep of tools/time_ntt.py over 8 .. 11 runs on a variant library built with
// -DBN254_NTT_TILE_LOG=11 (tools/build_variant.sh).  The default is the fastest at 2^20 of 8 / 9 / 10 (profiles/r14_ntt.txt); 11 is a
// little faster there but clearly slower at 2^24, and needs more than the 64 KiB of LDS a workgroup gets without asking.
#ifndef BN254_NTT_TILE_LOG
#define BN254_NTT_TILE_LOG 9
#endif
constexpr uint32_t NTT_TILE_LOG = BN254_NTT_TILE_LOG;
constexpr uint32_t NTT_LOG_MAX = 24;           // BN254_NTT_LOG_MAX
constexpr uint32_t NTT_TBL_LOG = 12;           // entries per table half; a stage twiddle is one load while T <= NTT_TBL_LOG
constexpr uint32_t NTT_TBL = 1u << NTT_TBL_LOG;
static_assert(NTT_TILE_LOG <= NTT_TBL_LOG && 2 * NTT_TBL_LOG >= NTT_LOG_MAX, "a stage twiddle must have no low part");

// one launch of one pass: workgroup w takes the small transforms tile_lo + w C .. of the `in` / `out` arrays (whole transforms, tile 0 = the
// first small transform of the first one), up to tile_end
struct NttPass {
    const uint32_t *in; uint32_t *out;
    const uint32_t *wtbl, *stbl;               // root table pair; shift table pair (pre / post == 2 only)
    uint32_t tile_lo, tile_end;
    uint32_t log_n, t, log_m, log_s, T;        // bn_ntt_plan; T: tile log in force
    uint32_t inverse;                          // twiddles are powers of w^-1
    uint32_t pre;                              // 1: inputs times stbl[index] (forward coset, first pass)
    uint32_t post;                             // last pass of an inverse: 1 outputs times `scale` (n^-1), 2 times stbl[index] (n^-1 s^-index)
    Fr scale;
};

#if defined(BN_HOSTSIM)
inline int ntt_tile_errors = 0;                // accesses past the tile (host simulation only)
#endif
// element i of a tile of `size` elements: words 0..3 at 4 i, words 4..7 at 4 (size + i), so that adjacent lanes move adjacent 16 bytes
BN_FN Fr ntt_tile_load(const uint32_t *tile, uint32_t size, uint32_t i) {
    Fr r;
#if defined(BN_HOSTSIM)
    if (i >= size) { ++ntt_tile_errors; return fr_zero(); }
    for (int j = 0; j < 4; ++j) { r.w[j] = tile[4 * i + j]; r.w[4 + j] = tile[4 * (size + i) + j]; }
#else
    const uint4 lo = ((const uint4 *)tile)[i], hi = ((const uint4 *)tile)[size + i];
    r.w[0] = lo.x; r.w[1] = lo.y; r.w[2] = lo.z; r.w[3] = lo.w; r.w[4] = hi.x; r.w[5] = hi.y; r.w[6] = hi.z; r.w[7] = hi.w;
#endif
    return r;
}
BN_FN void ntt_tile_store(const Fr &a, uint32_t *tile, uint32_t size, uint32_t i) {
#if defined(BN_HOSTSIM)
    if (i >= size) { ++ntt_tile_errors; return; }
    for (int j = 0; j < 4; ++j) { tile[4 * i + j] = a.w[j]; tile[4 * (size + i) + j] = a.w[4 + j]; }
#else
    ((uint4 *)tile)[i] = make_uint4(a.w[0], a.w[1], a.w[2], a.w[3]);
    ((uint4 *)tile)[size + i] = make_uint4(a.w[4], a.w[5], a.w[6], a.w[7]);
#endif
}
// the low `bits` bits of k reversed
BN_FN uint32_t ntt_bitrev(uint32_t k, uint32_t bits) {
#if defined(BN_HOSTSIM)
    uint32_t r = 0;
    for (uint32_t b = 0; b < bits; ++b) r |= ((k >> b) & 1u) << (bits - 1 - b);
    return r;
#else
    return bits ? __brev(k) >> (32u - bits) : 0u;
#endif
}
// w_24^(+-x) for x < 2^24 a multiple of 2^12: one load
BN_FN Fr ntt_root_high(const NttPass &P, uint32_t x) {
    const uint32_t mask = (1u << NTT_LOG_MAX) - 1u, e = P.inverse ? (0u - x) & mask : x;
    return fr_load(P.wtbl, NTT_TBL + (e >> NTT_TBL_LOG));
}
// w_24^(+-x) for any x < 2^24
BN_FN Fr ntt_root_power(const NttPass &P, uint32_t x) {
    const uint32_t mask = (1u << NTT_LOG_MAX) - 1u, e = P.inverse ? (0u - x) & mask : x;
    return fr_mul(fr_load(P.wtbl, e & (NTT_TBL - 1u)), fr_load(P.wtbl, NTT_TBL + (e >> NTT_TBL_LOG)));
}
// the factor of element `idx` of a transform from the shift tables: c g^idx
BN_FN Fr ntt_shift_power(const NttPass &P, uint32_t idx) {
    const Fr lo = fr_load(P.stbl, idx & (NTT_TBL - 1u));
    if (P.log_n <= NTT_TBL_LOG) return lo;                                     // uniform: the high part would be one
    return fr_mul(lo, fr_load(P.stbl, NTT_TBL + (idx >> NTT_TBL_LOG)));
}
// small transform `c` of workgroup `wg`: false past the end of the launch; tr = its transform, u = its number inside the transform
BN_FN bool ntt_tile_of(const NttPass &P, uint32_t wg, uint32_t c, uint32_t &tr, uint32_t &u) {
    const uint32_t g = P.tile_lo + (wg << (P.T - P.t)) + c, per = P.log_n - P.t;
    tr = g >> per; u = g & ((1u << per) - 1u);
    return g < P.tile_end;
}

// slot e = j C + c of the tile takes input j of small transform c: lanes that follow each other read records that follow each other
BN_FN void ntt_load_lane(const NttPass &P, uint32_t *tile, uint32_t wg, uint32_t lane) {
    const uint32_t size = 1u << P.T, logC = P.T - P.t;
    for (uint32_t e = lane; e < size; e += NTT_BLOCK) {
        uint32_t tr, u;
        if (!ntt_tile_of(P, wg, e & ((1u << logC) - 1u), tr, u)) continue;
        const uint32_t idx = u + ((e >> logC) << (P.log_n - P.t));
        Fr x = fr_load(P.in, ((size_t)tr << P.log_n) + idx);
        if (P.pre) x = fr_mul(x, ntt_shift_power(P, idx));
        ntt_tile_store(x, tile, size, e);
    }
}
// the stage twiddles of a pass, w_R^e for e < R / 2, from the table to `tw` (LDS: R / 2 elements laid out like a tile), once per workgroup:
// every stage then reads its twiddles at LDS latency
BN_FN void ntt_twiddle_lane(const NttPass &P, uint32_t *tw, uint32_t lane) {
    const uint32_t half = (1u << P.t) >> 1;
    for (uint32_t e = lane; e < half; e += NTT_BLOCK) ntt_tile_store(ntt_root_high(P, e << (NTT_LOG_MAX - P.t)), tw, half, e);
}
// stage st < t of every small transform of the tile: (a, b) at distance 2^(t-1-st) -> (a + b, (a - b) w_R^(r 2^st)), r the offset in the half
BN_FN void ntt_stage_lane(const NttPass &P, uint32_t *tile, const uint32_t *tw, uint32_t wg, uint32_t lane, uint32_t st) {
    const uint32_t size = 1u << P.T, logC = P.T - P.t, lh = P.t - 1u - st;
    for (uint32_t b = lane; b < size / 2; b += NTT_BLOCK) {
        const uint32_t c = b & ((1u << logC) - 1u), bb = b >> logC, r = bb & ((1u << lh) - 1u);
        uint32_t tr, u;
        if (!ntt_tile_of(P, wg, c, tr, u)) continue;
        const uint32_t lo = (((((bb >> lh) << (lh + 1u)) | r)) << logC) | c, hi = lo + (1u << (lh + logC));
        const Fr x = ntt_tile_load(tile, size, lo), y = ntt_tile_load(tile, size, hi);
        Fr d = fr_sub(x, y);
        if (lh) d = fr_mul(d, ntt_tile_load(tw, (1u << P.t) >> 1, r << st));              // uniform: the last stage's twiddles are one
        ntt_tile_store(fr_add(x, y), tile, size, lo);
        ntt_tile_store(d, tile, size, hi);
    }
}
// output k of small transform c sits at the reversed position; lanes that follow each other write records that follow each other (the
// first pass: k runs fastest, its outputs are adjacent; later passes: c does, adjacent small transforms write adjacent records)
BN_FN void ntt_store_lane(const NttPass &P, const uint32_t *tile, uint32_t wg, uint32_t lane) {
    const uint32_t size = 1u << P.T, logC = P.T - P.t;
    for (uint32_t e = lane; e < size; e += NTT_BLOCK) {
        const uint32_t c = P.log_s ? e & ((1u << logC) - 1u) : e >> P.t, k = P.log_s ? e >> logC : e & ((1u << P.t) - 1u);
        uint32_t tr, u;
        if (!ntt_tile_of(P, wg, c, tr, u)) continue;
        const uint32_t q = u & ((1u << P.log_s) - 1u), p = u >> P.log_s;
        Fr x = ntt_tile_load(tile, size, (ntt_bitrev(k, P.t) << logC) | c);
        if (P.log_m) x = fr_mul(x, ntt_root_power(P, (p * k) << (NTT_LOG_MAX - P.log_m - P.t)));      // uniform: the last pass has p == 0
        const uint32_t idx = q + (((p << P.t) + k) << P.log_s);
        if (P.post == 1) x = fr_mul(x, P.scale);
        else if (P.post == 2) x = fr_mul(x, ntt_shift_power(P, idx));
        fr_store(x, P.out, ((size_t)tr << P.log_n) + idx);
    }
}

// entry i < 2 NTT_TBL of a table pair: c0 g0^i, then c1 g1^(i - NTT_TBL) - square and multiply over the NTT_TBL_LOG bits of the exponent
BN_FN void ntt_table_body(uint32_t *out, const Fr &c0, const Fr &g0, const Fr &c1, const Fr &g1, uint32_t i) {
    if (i >= 2 * NTT_TBL) return;
    const bool high = i >= NTT_TBL;
    const uint32_t e = i & (NTT_TBL - 1u);
    Fr acc = fr_select(high, c0, c1), sq = fr_select(high, g0, g1);
#pragma unroll 1
    for (uint32_t b = 0; b < NTT_TBL_LOG; ++b) {
        const Fr m = fr_mul(acc, sq);
        acc = fr_select((e >> b) & 1u, acc, m);
        sq = fr_mul(sq, sq);
    }
    fr_store(acc, out, i);
}

}  // namespace bn254
