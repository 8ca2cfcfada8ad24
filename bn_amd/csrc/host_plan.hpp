// Host arithmetic over sizes and offsets: the argument checks that need no device, the work lists of the segmented folds, the cutting of a
// prepared batch into Miller pieces, the workspace of the bucket method and its tail scalars, the scalars of the fixed-base tables, the passes of a transform, the pieces of a sparse linear map, the levels of a segmented scan and of a sumcheck round, the check and piece length of the fused fold-then-round call, the passes of the quotients of a multilinear opening.  Plain C++17: nothing here touches a device, so
// tests/hostsim/ compiles it with g++ and tests/test_host_plan.py replays the plans on the CPU.  (io.hpp: the two records the kernels read.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/bn254_hip.h"
#include "io.hpp"

using bn254::BnMillerPiece;
using bn254::BnSegPiece;

constexpr size_t BN_N_MAX = (size_t)1 << 40;            // sanity bound on a batch; launches are cut to size internally

// ---- argument checks (no device involved)
// bn254_pairing_product_batch* for m > 0: CSR offsets, sizes, pointers
inline int bn_seg_check(const void *p, const void *q, const size_t *offsets, size_t m, const void *out) {
    if (!offsets || offsets[0] != 0) return BN254_E_BAD_ARG;
    for (size_t j = 0; j < m; ++j)
        if (offsets[j + 1] < offsets[j]) return BN254_E_BAD_ARG;
    const size_t n = offsets[m];
    return (n > BN_N_MAX || !out || (n && (!p || !q))) ? BN254_E_BAD_ARG : BN254_OK;
}
// the same checks for bn254_g{1,2}_msm_batch* (points, scalars)
inline int bn_msm_check(const void *p, const void *k, const size_t *offsets, size_t m, const void *out) { return bn_seg_check(p, k, offsets, m, out); }
// bn254_g{1,2}_msm* (one sum of n terms)
inline int bn_msm1_check(const void *p, const void *k, size_t n, const void *out) { return (n > BN_N_MAX || !out || (n && (!p || !k))) ? BN254_E_BAD_ARG : BN254_OK; }
// every segment holds exactly one element: the call is the plain batch operation
inline bool bn_seg_all_ones(const size_t *off, size_t m) {
    bool ones = off[m] == m;
    for (size_t j = 0; ones && j < m; ++j) ones = off[j] == j;
    return ones;
}
inline size_t bn_seg_longest(const size_t *off, size_t m) {
    size_t longest = 0;
    for (size_t j = 0; j < m; ++j) longest = std::max(longest, off[j + 1] - off[j]);
    return longest;
}

// as few sub-launches as possible with none above one round, all of (nearly) the same size: a ragged tail of a few pairings
// would cost a whole kernel latency (one wave takes as long as a full machine)
inline size_t bn_equal_parts(size_t n, size_t round) {
    const size_t parts = (n + round - 1) / round;
    return parts <= 1 ? n : ((n + parts - 1) / parts + 31) / 32 * 32;
}

// sub-launches of at most `step` units: fn(lo, cnt) enqueues one
template <class Fn>
int bn_for_parts(size_t n, size_t step, Fn fn) {
    for (size_t lo = 0; lo < n; lo += step) {
        int rc = fn(lo, n - lo < step ? n - lo : step);
        if (rc) return rc;
    }
    return BN254_OK;
}

// ---- the plan of a segmented fold (bn254_seg.hip runs it: Fq12 products of the batched multi-pairings, point sums of the segmented MSM)
constexpr size_t BN_SEG_FOLD = 16;          // values per lane-pair piece of the fold: at most 15 products in a row (~20-30 us each)
constexpr size_t BN_TAIL_SEG_MAX = 16;      // values per wave in the ragged tail: at most 15 wave products (~2.7 us each) before the exponentiation
struct SegLaunch { bool tail; size_t first, count; };                                  // a range of the work list: one fold level or the tail
struct SegChunk { size_t lo, hi; bool carry_out; std::vector<SegLaunch> launches; };   // values [lo, hi) and what follows them
// partial products ALL fold levels of one chunk write, at most: a segment of L > BN_SEG_FOLD values gives ceil(L / BN_SEG_FOLD) < 2 L / BN_SEG_FOLD
// partials, so level 0 writes fewer than 2 (chunk_pairs + 1) / BN_SEG_FOLD and every further level fewer than 1/8 of the level before.
// Every partial of a chunk has a slot of its own (no level reuses another level's slots): a piece may read its inputs several levels
// after they were written - the ragged tail of the small route reads them only after the deepest level of the plan.
// (`fold` >= 4 values per piece - the multi-scalar multiplications plan with their own width, BN_MSM_FOLD: 2 L / fold (1 + 2 / fold + ...) <= 4 L / fold.)
inline size_t seg_partials_max(size_t chunk_pairs, size_t fold = BN_SEG_FOLD) { return 4 * (chunk_pairs + 1) / fold + 4; }
// workspace (in values: Fq12, or Jacobian points for the multi-scalar multiplications): [carry in][chunk_pairs values][partials of every level][carry out]
inline size_t seg_ws_values(size_t chunk_pairs, size_t fold = BN_SEG_FOLD) { return chunk_pairs + 2 + seg_partials_max(chunk_pairs, fold); }
// false if the partials would not fit their region (cannot happen by the bound above; checked, never written out of bounds)
// V: bytes per value; fold: values per piece; snap: cut at the last segment boundary inside a chunk (false: every chunk is full, and any
// segment across a cut carries).  The piece that writes out[j] carries last = 1 (read by the point fold only: it normalises there).
inline bool seg_plan(const size_t *off, size_t m, size_t chunk_pairs, bool small, char *ws, char *d_out, std::vector<BnSegPiece> &pieces, std::vector<SegChunk> &chunks,
                     size_t V, size_t fold = BN_SEG_FOLD, bool snap = true) {
    const size_t n = off[m], pb = seg_partials_max(chunk_pairs, fold), last_cap = small ? BN_TAIL_SEG_MAX : fold;
    char *const part = ws + (chunk_pairs + 1) * V, *const carry_out = ws + (chunk_pairs + 1 + pb) * V;
    size_t lo = 0, j = 0;
    bool carry = false;
    do {
        size_t hi = std::min(n, lo + chunk_pairs);
        if (snap && hi < n) {
            const size_t b = *(std::upper_bound(off, off + m + 1, hi) - 1);          // last segment boundary <= hi
            if (b > lo) hi = b;
        }
        // segments that start in front of hi (the last chunk also takes the empty segments at n)
        const size_t jend = hi == n ? m : (size_t)(std::lower_bound(off + j, off + m, hi) - off);
        std::vector<std::vector<BnSegPiece>> lv(1);
        size_t used = 0;                                                     // partial slots taken in this chunk
        std::vector<BnSegPiece> tail;
        SegChunk ch{lo, hi, false, {}};
        for (size_t jj = j; jj < jend; ++jj) {
            const bool from_carry = carry && jj == j, to_carry = off[jj + 1] > hi;
            const size_t a = from_carry ? 0 : off[jj] - lo + 1, b = std::min(off[jj + 1], hi) - lo + 1;      // value slots [a, b)
            const char *src = ws + a * V;
            size_t L = b - a, level = 0;
            while (L > last_cap) {
                if (lv.size() <= level) lv.emplace_back();
                char *base = part + used * V;
                const size_t k = (L + fold - 1) / fold;
                if (used + k > pb) return false;
                for (size_t i = 0; i < k; ++i)
                    lv[level].push_back({(const uint32_t *)(src + i * fold * V), (uint32_t *)(base + i * V), (uint32_t)std::min(fold, L - i * fold), 0u});
                used += k; src = base; L = k; ++level;
            }
            const BnSegPiece last = {(const uint32_t *)src, (uint32_t *)(to_carry ? carry_out : d_out + jj * V), (uint32_t)L, to_carry ? 0u : 1u};
            if (small) tail.push_back(last);
            else { if (lv.size() <= level) lv.resize(level + 1); lv[level].push_back(last); }
            ch.carry_out |= to_carry;
        }
        for (const auto &l : lv)
            if (!l.empty()) { ch.launches.push_back({false, pieces.size(), l.size()}); pieces.insert(pieces.end(), l.begin(), l.end()); }
        if (!tail.empty()) { ch.launches.push_back({true, pieces.size(), tail.size()}); pieces.insert(pieces.end(), tail.begin(), tail.end()); }
        carry = ch.carry_out;
        j = carry ? jend - 1 : jend;
        lo = hi;
        chunks.push_back(std::move(ch));
    } while (lo < n);
    return true;
}

// ---- a prepared batch cut into Miller pieces (bn254_pairing_product_batch_prepared_native*): every segment of L pairs gives ceil(L / 4)
// pieces of at most four consecutive pairs, or - `direct`: no segment above four pairs - exactly one (an empty segment: a piece of no pairs)
// derived offsets of the fold over the pieces' values: voff[j + 1] - voff[j] = ceil(L_j / 4)
inline std::vector<size_t> miller_value_offsets(const size_t *off, size_t m) {
    std::vector<size_t> voff(m + 1, 0);
    for (size_t j = 0; j < m; ++j) voff[j + 1] = voff[j] + (off[j + 1] - off[j] + 3) / 4;
    return voff;
}
struct MillerSub { size_t lo, cnt, base; };             // pieces [lo, lo + cnt) of the list; base: the first pair of the sub-launch
struct MillerCut { std::vector<BnMillerPiece> pieces; std::vector<MillerSub> subs; std::vector<size_t> chunk_subs; };      // subs [chunk_subs[i], chunk_subs[i + 1]): chunk i's
// the pieces in launch order and their sub-launches: of step(count) pieces for a chunk of `count` (at most one round of lane pairs), never
// across a chunk; a piece's `first` is relative to its sub-launch.  chunks: piece ranges [lo, hi) (direct: the one chunk {0, m})
template <class Step>
MillerCut miller_cut(const size_t *off, size_t m, bool direct, const std::vector<SegChunk> &chunks, Step step) {
    MillerCut cut;
    std::vector<size_t> first;                    // absolute until the sub-launches are cut
    for (size_t j = 0; j < m; ++j) {
        const size_t L = off[j + 1] - off[j];
        if (direct) { first.push_back(off[j]); cut.pieces.push_back({0u, (uint32_t)L}); }
        else for (size_t k = 0; k < L; k += 4) { first.push_back(off[j] + k); cut.pieces.push_back({0u, (uint32_t)std::min<size_t>(4, L - k)}); }
    }
    for (const SegChunk &ch : chunks) {
        cut.chunk_subs.push_back(cut.subs.size());
        const size_t count = ch.hi - ch.lo;
        bn_for_parts(count, count ? step(count) : 1, [&](size_t at, size_t cnt) {
            const size_t lo = ch.lo + at, base = first[lo];
            for (size_t k = lo; k < lo + cnt; ++k) cut.pieces[k].first = (uint32_t)(first[k] - base);
            cut.subs.push_back({lo, cnt, base});
            return 0;
        });
    }
    cut.chunk_subs.push_back(cut.subs.size());
    return cut;
}

// ---- bucket (Pippenger) route of bn254_g{1,2}_msm: window width, levels of the accumulation, workspace, tail scalars
constexpr unsigned BN_MSM_GROUP = 16;         // buckets per lane of the reduction: 32 additions in a row, 2^c / 8 tail terms per window
inline size_t bn_align256(size_t x) { return (x + 255) & ~(size_t)255; }
// window width by size when BN254_OPT_MSM_WINDOW_BITS is not set (forced < 1): the best measured width per size (profiles/r10_msm_bucket.txt)
inline unsigned bn_msm_window_bits(long forced, size_t n) {
    if (forced >= 1) return (unsigned)forced;
    unsigned lg = 0;
    while (((size_t)2 << lg) <= n) ++lg;                     // floor(log2 n), 0 for n <= 1
    // G1 and G2 agree on the best width at every measured size; between neighbouring widths the kernel time differs by a few percent
    // (the accumulation is bound by its gathers, not by the W additions per term) except where a width leaves a top window of one or
    // two bits, whose few buckets every term hits (13 at 2^19: 7.3 against 6.6 ms)
    return lg <= 14 ? 8 : lg == 15 ? 9 : lg <= 17 ? 11 : lg == 18 ? 12 : lg == 19 ? 11 : 14;
}
// cb-bit windows over chunks of at most `chunk` terms, V bytes per point, L = bn254_msm_piece_M() entries per lane and level
struct MsmBucketPlan {
    unsigned W, G, groups;                       // windows; buckets per group of the reduction; groups per window
    size_t K, count, n0max;                      // buckets; (window, group) pairs = tail terms / 2; entries of a chunk, at most
    std::vector<size_t> out_slots;               // slots every level writes, from the upper bound of its entries
    size_t o_counts, o_tiles, o_n0, o_idx, o_keys, o_buckets, o_terms, bytes;      // 256-byte aligned offsets into the workspace, and its size
    std::vector<std::pair<size_t, size_t>> o_level;                                // per level: partial sums, their keys
};
inline MsmBucketPlan msm_bucket_plan(unsigned cb, size_t chunk, size_t V, size_t L) {
    MsmBucketPlan p;
    p.W = (254 + cb - 1) / cb; p.G = std::min(BN_MSM_GROUP, 1u << cb); p.groups = (1u << cb) / p.G;
    p.K = (size_t)p.W << cb; p.count = (size_t)p.W * p.groups;
    p.n0max = (size_t)p.W * chunk;                 // < 254 * 2^22 < 2^32: positions and keys are 32-bit
    for (size_t N = p.n0max;;) {
        const size_t M = 2 * ((N + L - 1) / L);
        p.out_slots.push_back(M);
        if (N <= L) break;
        N = M;
    }
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += bn_align256(bytes); return o; };
    p.o_counts = take(p.K * 4); p.o_tiles = take(1024 * 4); p.o_n0 = take(4); p.o_idx = take(p.n0max * 4); p.o_keys = take(p.n0max * 4); p.o_buckets = take(p.K * V);
    for (size_t M : p.out_slots) { const size_t a = take(M * V), b = take(M * 4); p.o_level.push_back({a, b}); }
    p.o_terms = take(2 * p.count * V);
    p.bytes = at;
    return p;
}
constexpr uint64_t BN_FR_MOD64[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
// out = (a + b) mod r for a, b < r (r < 2^254: the sum fits four words)
inline void bn_fr_add(const uint64_t *a, const uint64_t *b, uint64_t *out) {
    uint64_t t[4], d[4];
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; ++i) { c += (unsigned __int128)a[i] + b[i]; t[i] = (uint64_t)c; c >>= 64; }
    unsigned __int128 br = 0;
    for (int i = 0; i < 4; ++i) { const unsigned __int128 x = (unsigned __int128)t[i] - BN_FR_MOD64[i] - br; d[i] = (uint64_t)x; br = (x >> 64) & 1; }
    for (int i = 0; i < 4; ++i) out[i] = br ? t[i] : d[i];
}
inline void bn_fr_one(bn_fr *out) {                           // 2^256 mod r: the Montgomery image of one
    uint64_t x[4] = {1, 0, 0, 0};
    for (int i = 0; i < 256; ++i) bn_fr_add(x, x, x);
    memcpy(out->l, x, sizeof x);
}
// the scalars of the tail's 2 * count terms as Montgomery images: base * 2^(c w) for the S term of every (window, group), then 2^(c w) for the T terms
inline void msm_tail_scalars(unsigned cb, std::vector<uint64_t> &h) {
    const unsigned W = (254 + cb - 1) / cb, G = std::min(BN_MSM_GROUP, 1u << cb), groups = (1u << cb) / G;
    const size_t count = (size_t)W * groups;
    h.assign(2 * count * 4, 0);
    bn_fr pw; bn_fr_one(&pw);
    for (unsigned w = 0; w < W; ++w) {
        uint64_t step[4], acc[4] = {0, 0, 0, 0};
        memcpy(step, pw.l, sizeof step);
        for (unsigned b = 1; b < G; b <<= 1) bn_fr_add(step, step, step);                  // G * 2^(c w)
        for (unsigned q = 0; q < groups; ++q) {
            memcpy(&h[((size_t)w * groups + q) * 4], acc, sizeof acc);
            memcpy(&h[(count + (size_t)w * groups + q) * 4], pw.l, sizeof acc);
            bn_fr_add(acc, step, acc);
        }
        for (unsigned b = 0; b < cb; ++b) bn_fr_add(pw.l, pw.l, pw.l);
    }
}

// ---- multi-scalar multiplication against prepared bases (bn254_g{1,2}_msm_prepare / bn254_g{1,2}_msm_prepared): the handle's table holds the
// affine points 2^(c w) P_i, so every (term, window) pair falls into ONE set of 2^(c-1) buckets by its signed digit, bucket b weighs b + 1
inline unsigned bn_msm_prepared_windows(unsigned cb) { return (254 + cb - 1) / cb; }
// Window width of a handle of n points when the caller passes 0: the width with the smallest median kernel time of the sweep over
// c = 10 .. 16 (tools/time_msm_prepared.py --widths, profiles/r29_msm_prepared.txt: G1 2^16 / 2^18 / 2^20 / 2^22 and G2 2^15 / 2^18 / 2^20), a
// size in between or outside taking the width of the nearest measured one.  The table has ONE entry: 16 won at all seven sizes, for both
// groups (G1 2^20: 7.27 ms against 7.41 at 15 and 7.59 at 14; G2 2^20: 11.53 against 12.04 and 12.57) - the counting sort's atomics meet in
// 2^(c-1) counters for ALL windows, so its time falls with every bit (G1 2^20: 18.3 ms at c = 10, 2.1 ms at 16), and 16 has the fewest
// windows, hence the fewest entries and the smallest table.  Total on every n.
inline unsigned bn_msm_prepared_window_bits(size_t n) {
    (void)n;
    return 16;
}
// what bn254_g{1,2}_msm_prepare* can refuse without a device: window_bits is 0 (default) or 3 .. 16 (c W > 254 rules out 1 and 2: the top
// window must not carry); a table index w * count + i must leave bit 31 to the sign
inline int bn_msm_prepare_check(const void *p, size_t n, int window_bits, const void *out) {
    if (!out || (n && !p) || n > BN_N_MAX) return BN254_E_BAD_ARG;
    if (window_bits != 0 && (window_bits < 3 || window_bits > 16)) return BN254_E_BAD_ARG;
    const unsigned cb = window_bits ? (unsigned)window_bits : bn_msm_prepared_window_bits(n);
    return (unsigned __int128)bn_msm_prepared_windows(cb) * n >= ((unsigned __int128)1 << 31) ? BN254_E_BAD_ARG : BN254_OK;
}
// ... and a call over a handle of `count` points of group `group`: the range [first, first + n) lies in the handle
inline int bn_msm_prepared_check(bool have_handle, int group, int g, size_t count, size_t first, const void *k, size_t n, const void *out) {
    if (!have_handle || group != g || !out || (n && !k)) return BN254_E_BAD_ARG;
    return first > count || n > count - first ? BN254_E_BAD_ARG : BN254_OK;
}
// The workspace of a call with cb-bit windows over chunks of at most `chunk` terms: msm_bucket_plan's layout with ONE window of
// K = 2^(cb-1) buckets for the reduction (count = groups lanes, 2 * count tail terms) and up to W * chunk sorted entries per chunk.
inline MsmBucketPlan msm_prepared_plan(unsigned cb, size_t chunk, size_t V, size_t L) {
    MsmBucketPlan p;
    p.W = bn_msm_prepared_windows(cb);
    p.K = (size_t)1 << (cb - 1);
    p.G = (unsigned)std::min<size_t>(BN_MSM_GROUP, p.K); p.groups = (unsigned)(p.K / p.G);
    p.count = p.groups;
    p.n0max = (size_t)p.W * chunk;                 // < 86 * 2^22 < 2^32: positions are 32-bit
    for (size_t N = p.n0max;;) {
        const size_t M = 2 * ((N + L - 1) / L);
        p.out_slots.push_back(M);
        if (N <= L) break;
        N = M;
    }
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += bn_align256(bytes); return o; };
    p.o_counts = take(p.K * 4); p.o_tiles = take(1024 * 4); p.o_n0 = take(4); p.o_idx = take(p.n0max * 4); p.o_keys = take(p.n0max * 4); p.o_buckets = take(p.K * V);
    for (size_t M : p.out_slots) { const size_t a = take(M * V), b = take(M * 4); p.o_level.push_back({a, b}); }
    p.o_terms = take(2 * p.count * V);
    p.bytes = at;
    return p;
}
// the scalars of the tail's 2 * groups terms as Montgomery images: base + 1 for the S term of the group whose first bucket is `base`
// (bucket b weighs b + 1), then 1 for every T term
inline void msm_prepared_tail_scalars(unsigned cb, std::vector<uint64_t> &h) {
    const size_t K = (size_t)1 << (cb - 1), G = std::min<size_t>(BN_MSM_GROUP, K), groups = K / G;
    h.assign(2 * groups * 4, 0);
    bn_fr one; bn_fr_one(&one);
    uint64_t step[4] = {0, 0, 0, 0}, acc[4];
    memcpy(acc, one.l, sizeof acc);
    for (size_t b = 0; b < G; ++b) bn_fr_add(step, one.l, step);                           // G
    for (size_t q = 0; q < groups; ++q) {
        memcpy(&h[q * 4], acc, sizeof acc);
        memcpy(&h[(groups + q) * 4], one.l, sizeof acc);
        bn_fr_add(acc, step, acc);
    }
}

// ---- fixed-base scalar multiplication (bn254_g{1,2}_mul_base_batch): the table of a base for signed c-bit windows holds d * 2^(c w) * B for
// w < W = ceil(254 / c) and d = 1 .. 2^(c-1), entry (w, d) at index w * 2^(c-1) + d - 1
inline unsigned bn_base_windows(unsigned cb) { return (254 + cb - 1) / cb; }
inline size_t bn_base_entries(unsigned cb) { return (size_t)bn_base_windows(cb) << (cb - 1); }
// the scalars the table is built with, in entry order, as Montgomery images: d * 2^(c w) mod r
inline void base_table_scalars(unsigned cb, std::vector<uint64_t> &h) {
    const unsigned W = bn_base_windows(cb);
    const size_t half = (size_t)1 << (cb - 1);
    h.assign(W * half * 4, 0);
    bn_fr pw; bn_fr_one(&pw);
    for (unsigned w = 0; w < W; ++w) {
        uint64_t acc[4];
        memcpy(acc, pw.l, sizeof acc);
        for (size_t d = 1; d <= half; ++d) {
            memcpy(&h[(w * half + d - 1) * 4], acc, sizeof acc);
            bn_fr_add(acc, pw.l, acc);
        }
        for (unsigned b = 0; b < cb; ++b) bn_fr_add(pw.l, pw.l, pw.l);
    }
}

// ---- number-theoretic transforms over Fr (bn254_fr_ntt_batch): the handful of field operations the HOST needs per call - the root of a size,
// the inverse of the coset shift, n^-1 - as Montgomery images, and the cut of a transform into passes
constexpr uint64_t BN_FR_INV64 = 0xc2e1f593efffffffull;                // -r^-1 mod 2^64
// the Montgomery image of w_28 = 5^((r-1)/2^28) = 19103219067921713944291392827692070036145651957329286315305642004821462161904 (ark-bn254's root)
constexpr uint64_t BN_FR_ROOT28[4] = {0x636e735580d13d9cull, 0xa22bf3742445ffd6ull, 0x56452ac01eb203d8ull, 0x1860ef942963f9e7ull};
constexpr uint64_t BN_FR_MINUS_2[4] = {0x43e1f593efffffffull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};   // r - 2 (raw)
constexpr int BN_NTT_ROOT_LOG = 28;
// out = a * b / 2^256 mod r for a canonical b (a: any four words), word-serial like fr.hpp's fr_mul; out may be a or b
inline void bn_fr_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) {
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; ++j) { c += (unsigned __int128)a[i] * b[j] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * BN_FR_INV64;
        c = ((unsigned __int128)m * BN_FR_MOD64[0] + t[0]) >> 64;
        for (int j = 1; j < 4; ++j) { c += (unsigned __int128)m * BN_FR_MOD64[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
    }
    uint64_t d[4];
    unsigned __int128 br = 0;
    for (int i = 0; i < 4; ++i) { const unsigned __int128 x = (unsigned __int128)t[i] - BN_FR_MOD64[i] - br; d[i] = (uint64_t)x; br = (x >> 64) & 1; }
    const bool ge = t[4] != 0 || br == 0;
    for (int i = 0; i < 4; ++i) out[i] = ge ? d[i] : t[i];
}
// out = a^e for the 256-bit integer e (four words, least significant first)
inline void bn_fr_pow(const uint64_t *a, const uint64_t *e, uint64_t *out) {
    bn_fr acc; bn_fr_one(&acc);
    for (int bit = 255; bit >= 0; --bit) {
        bn_fr_mul(acc.l, acc.l, acc.l);
        if ((e[bit >> 6] >> (bit & 63)) & 1) bn_fr_mul(acc.l, a, acc.l);
    }
    memcpy(out, acc.l, sizeof acc.l);
}
inline void bn_fr_inverse(const uint64_t *a, uint64_t *out) { bn_fr_pow(a, BN_FR_MINUS_2, out); }
// 2^-k as a Montgomery image: the n^-1 of an inverse transform of n = 2^k elements
constexpr uint64_t BN_FR_HALF[4] = {0x783c14d81ffffffeull, 0xaf982f6f0c8d1eddull, 0x8f5f7492fcfd4f45ull, 0x1f37631a3d9cbfacull};   // (r + 1) / 2
inline void bn_fr_inv_pow2(unsigned k, bn_fr *out) {
    bn_fr_one(out);
    for (unsigned i = 0; i < k; ++i) bn_fr_mul(out->l, BN_FR_HALF, out->l);
}
inline bool bn_fr_is_zero(const uint64_t *a) { return (a[0] | a[1] | a[2] | a[3]) == 0; }
// w_n for n = 2^log_n: w_28^(2^(28 - log_n)), so the domains of all sizes nest
inline int bn_fr_root(int log_n, bn_fr *out) {
    if (log_n < 0 || log_n > BN_NTT_ROOT_LOG || !out) return BN254_E_BAD_ARG;
    memcpy(out->l, BN_FR_ROOT28, sizeof out->l);
    for (int i = log_n; i < BN_NTT_ROOT_LOG; ++i) bn_fr_mul(out->l, out->l, out->l);
    return BN254_OK;
}
// A transform of n = 2^log_n over tiles of 2^T elements is P = ceil(log_n / T) passes (one for log_n == 0) of t_0 >= t_1 >= .. radix-2 stages
// with t_0 + .. = log_n, as even as they come.  Pass i is the step of a Stockham autosort that splits the current length n_i = 2^(log_m + t)
// into 2^t sub-transforms of length 2^log_m each, the data already interleaved at stride 2^log_s: log_s + t + log_m = log_n.
struct BnNttPass { unsigned t, log_m, log_s; };
constexpr unsigned BN_NTT_PASSES_MAX = 24;
inline unsigned bn_ntt_plan(unsigned log_n, unsigned T, BnNttPass *pass) {
    const unsigned P = log_n ? (log_n + T - 1) / T : 1, base = log_n / P, rem = log_n % P;
    unsigned done = 0;
    for (unsigned i = 0; i < P; ++i) {
        const unsigned t = base + (i < rem ? 1u : 0u);
        pass[i] = BnNttPass{t, log_n - done - t, done};
        done += t;
    }
    return P;
}
// The launches of a call: groups of whole transforms of at most `step` elements (a larger transform is a group of its own); per group the
// passes one after the other, each as sub-launches of at most `step` elements cut between small transforms (whole workgroups of
// C = 2^(T - t) of them where a sub-launch holds that many).  A pass reads one array and writes another: the last writes OUT, the ones before
// alternate between WS0 and OUT, and pass 0 reads IN - so an odd number (> 1) of passes in place would have pass 0 write what it still
// reads, and writes WS1 instead.  A single pass is in place by construction (a workgroup reads all of its transforms before it writes).
enum BnNttBuf { BN_NTT_IN, BN_NTT_OUT, BN_NTT_WS0, BN_NTT_WS1 };
struct BnNttRun {
    unsigned P; BnNttPass pass[BN_NTT_PASSES_MAX];
    size_t per_group;                   // transforms per group
    size_t most;                        // elements of the largest group: the size of one workspace array
    unsigned ws_bufs;                   // workspace arrays of `most` elements the call needs: 0, 1 or 2
};
inline BnNttRun bn_ntt_run(unsigned log_n, unsigned T, size_t count, size_t step, bool in_place) {
    BnNttRun r;
    r.P = bn_ntt_plan(log_n, T, r.pass);
    r.per_group = std::max<size_t>(1, step >> log_n);
    r.most = std::min(count, r.per_group) << log_n;
    r.ws_bufs = r.P < 2 ? 0u : (in_place && (r.P & 1) ? 2u : 1u);
    return r;
}
// one sub-launch: pass `i` of the group over small transforms [lo, lo + n) in `blocks` workgroups; pre: inputs times the shift's powers
// (forward coset, first pass); post: last pass of an inverse - 1 outputs times n^-1, 2 times n^-1 s^-index
struct BnNttStep { unsigned i; BnNttPass g; BnNttBuf src, dst; unsigned pre, post; size_t lo, n, blocks; };
// the sub-launches of one group of `cnt` transforms, in order: fn(step) enqueues one
template <class Fn>
int bn_ntt_group(const BnNttRun &r, unsigned log_n, unsigned T, size_t cnt, size_t step, bool in_place, bool shift, bool inverse, Fn fn) {
    BnNttBuf src = BN_NTT_IN;
    for (unsigned i = 0; i < r.P; ++i) {
        BnNttStep s;
        s.i = i; s.g = r.pass[i]; s.src = src;
        s.dst = ((r.P - 1 - i) & 1) ? BN_NTT_WS0 : BN_NTT_OUT;
        if (i == 0 && r.P > 1 && s.dst == BN_NTT_OUT && in_place) s.dst = BN_NTT_WS1;
        s.pre = (i == 0 && shift && !inverse) ? 1u : 0u;
        s.post = (i == r.P - 1 && inverse) ? (shift ? 2u : 1u) : 0u;
        const size_t tiles = cnt << (log_n - s.g.t), C = (size_t)1 << (T - s.g.t);
        size_t per_launch = std::max<size_t>(1, step >> s.g.t);
        if (per_launch >= C) per_launch -= per_launch % C;
        const int rc = bn_for_parts(tiles, per_launch, [&](size_t lo, size_t n) -> int {
            s.lo = lo; s.n = n; s.blocks = (n + C - 1) / C;
            return fn(s);
        });
        if (rc) return rc;
        src = s.dst;
    }
    return BN254_OK;
}

// ---- transforms over G1 / G2 (bn254_g{1,2}_ntt_batch): the argument check and the steps of a call
// in the order of ntt_check (the empty call is answered before): range of log_n, pointers, size, a zero shift
inline int bn_group_ntt_check(const void *in, const void *out, int log_n, size_t count, const bn_fr *shift) {
    if (log_n < 0 || log_n > BN254_GROUP_NTT_LOG_MAX || !in || !out) return BN254_E_BAD_ARG;
    if (count > (BN_N_MAX >> log_n)) return BN254_E_BAD_ARG;
    if (shift && bn_fr_is_zero(shift->l)) return BN254_E_BAD_ARG;
    return BN254_OK;
}
// A call runs in groups of whole transforms of at most `cap` points (a larger transform is a group of its own).  The steps of a group, each
// over all of its transforms:
//   SCALE      (forward with a shift, first)  point j times s^j, IN -> OUT: lane-local, so OUT may be IN
//   STAGE i    i < log_n, group_ntt_ops.hpp: reads one array and writes ANOTHER - the first one writes WS, then OUT and WS alternate
//   SCALE      (inverse, after the last stage) point j times n^-1 s^-j, or every point times n^-1: in place, wherever the last stage wrote
//   NORMALIZE  from there to OUT (in place when that is OUT)
// IN is never written and OUT only once IN has been read completely, so OUT may be IN; one workspace array of `most` Jacobian points serves
// every call with log_n >= 1.  At log_n == 0 every factor is one: the call is the normalisation.  A step is cut into sub-launches of at
// most `cap` units - butterflies for a stage, points otherwise -, and what runs chains (every step but stage 0 and the normalisation) of at
// most `chain_cap` besides: a lane's window table is scratch of the launch.
enum BnGroupNttKind { BN_GNTT_SCALE, BN_GNTT_STAGE, BN_GNTT_NORMALIZE };
struct BnGroupNttRun {
    unsigned stages;                    // log_n
    bool pre, post;                     // the two passes
    size_t per_group;                   // transforms per group
    size_t most;                        // points of the largest group: the size of the workspace array
    unsigned ws_bufs;                   // 0 or 1
};
inline BnGroupNttRun bn_group_ntt_run(unsigned log_n, size_t count, size_t cap, bool shift, bool inverse) {
    BnGroupNttRun r;
    r.stages = log_n;
    r.pre = log_n > 0 && shift && !inverse;
    r.post = log_n > 0 && inverse;
    r.per_group = std::max<size_t>(1, cap >> log_n);
    r.most = std::min(count, r.per_group) << log_n;
    r.ws_bufs = log_n ? 1u : 0u;
    return r;
}
// one sub-launch: units [lo, lo + n) of the step, counted from the group's first transform
struct BnGroupNttStep { BnGroupNttKind kind; unsigned stage; BnNttBuf src, dst; bool chain; size_t lo, n; };
// the sub-launches of one group of `cnt` transforms, in order: fn(step) enqueues one
template <class Fn>
int bn_group_ntt_group(const BnGroupNttRun &r, unsigned log_n, size_t cnt, size_t cap, size_t chain_cap, Fn fn) {
    const size_t points = cnt << log_n, chain_step = std::min(cap, chain_cap);
    BnNttBuf cur = BN_NTT_IN;
    auto step = [&](BnGroupNttKind kind, unsigned stage, BnNttBuf dst, bool chain, size_t units) -> int {
        BnGroupNttStep s = {kind, stage, cur, dst, chain, 0, 0};
        const int rc = bn_for_parts(units, chain ? chain_step : cap, [&](size_t lo, size_t n) -> int { s.lo = lo; s.n = n; return fn(s); });
        cur = dst;
        return rc;
    };
    int rc;
    if (r.pre && (rc = step(BN_GNTT_SCALE, 0, BN_NTT_OUT, true, points))) return rc;
    for (unsigned i = 0; i < r.stages; ++i)
        if ((rc = step(BN_GNTT_STAGE, i, cur == BN_NTT_WS0 ? BN_NTT_OUT : BN_NTT_WS0, i != 0, points / 2))) return rc;
    if (r.post && (rc = step(BN_GNTT_SCALE, 0, cur, true, points))) return rc;
    return step(BN_GNTT_NORMALIZE, 0, BN_NTT_OUT, false, points);
}

// ---- sparse linear maps over Fr (bn254_fr_dot_batch): the argument checks and the work list
// CSR offsets, sizes and pointers as for the other segmented calls; without an index the terms meet x one to one, so nx must be n
inline int bn_dot_check(const void *coeff, bool has_index, const void *x, size_t nx, const size_t *offsets, size_t m, const void *out) {
    const int rc = bn_seg_check(coeff, x, offsets, m, out);
    if (rc) return rc;
    return (!has_index && nx != offsets[m]) ? BN254_E_BAD_ARG : BN254_OK;
}
// the host-buffer form reads its index: the caller gets an error, never a wrong sum
inline int bn_dot_check_index(const uint64_t *index, size_t n, size_t nx) {
    for (size_t t = 0; index && t < n; ++t)
        if (index[t] >= nx) return BN254_E_BAD_ARG;
    return BN254_OK;
}
// Every segment of L terms is cut into k = ceil(L / P) pieces of at most P consecutive terms, one lane each (level 0: products and sums).
// k <= 1: the piece writes out[j] (an empty segment: a piece of no terms, which writes zero).  Otherwise the pieces write k partial sums to
// scratch slots of their own, and fold levels of at most F consecutive slots per lane (additions only) follow until one value is left, which
// goes to out[j]: ceil(log_F k) levels.  No slot is written twice, so a level may run as any number of sub-launches in any order after the
// level before it.  Slots: k (1 + 1/F + 1/F^2 + ..) + levels < 2 k + 64 per folded segment, fewer than 2 n / P + 64 m in all.
struct BnDotLevel { size_t first, count; };                 // a range of the work list
struct BnDotPlan {
    std::vector<bn254::BnDotPiece> pieces;                  // level after level
    std::vector<BnDotLevel> levels;                         // [0]: the product level (one piece per segment at least), then the fold levels
    size_t slots = 0;                                       // scratch records of 32 bytes
};
inline bn254::BnDotPiece bn_dot_piece(uint64_t first, size_t len, bool to_out, uint64_t dst) {
    return {first | (uint64_t)len << 48 | (uint64_t)(to_out ? 1 : 0) << 63, dst};
}
inline BnDotPlan bn_dot_plan(const size_t *off, size_t m, size_t P, size_t F) {
    BnDotPlan plan;
    std::vector<std::vector<bn254::BnDotPiece>> lv(1);
    lv[0].reserve(m + off[m] / P);
    for (size_t j = 0; j < m; ++j) {
        const size_t L = off[j + 1] - off[j];
        if (L <= P) { lv[0].push_back(bn_dot_piece(off[j], L, true, j)); continue; }
        size_t k = (L + P - 1) / P, src = plan.slots, level = 1;
        for (size_t i = 0; i < k; ++i) lv[0].push_back(bn_dot_piece(off[j] + i * P, std::min(P, L - i * P), false, src + i));
        plan.slots += k;
        for (; k > F; ++level) {
            const size_t k2 = (k + F - 1) / F, dst = plan.slots;
            if (lv.size() <= level) lv.emplace_back();
            for (size_t i = 0; i < k2; ++i) lv[level].push_back(bn_dot_piece(src + i * F, std::min(F, k - i * F), false, dst + i));
            plan.slots += k2; src = dst; k = k2;
        }
        if (lv.size() <= level) lv.emplace_back();
        lv[level].push_back(bn_dot_piece(src, k, true, j));
    }
    for (const auto &l : lv) {
        plan.levels.push_back({plan.pieces.size(), l.size()});
        plan.pieces.insert(plan.pieces.end(), l.begin(), l.end());
    }
    return plan;
}

// ---- segmented scans over Fr (bn254_fr_scan_batch): the argument checks and the work list
constexpr unsigned BN_SCAN_FLAGS_ALL = BN254_SCAN_REVERSE | BN254_SCAN_EXCLUSIVE | BN254_SCAN_A_PER_SEGMENT;
// one operand at least, known flags, CSR offsets as for the other segmented calls, an output.  init is optional, so nothing is asked of it.
inline int bn_scan_check(const void *a, const void *b, const size_t *offsets, size_t m, unsigned flags, const void *out) {
    if ((!a && !b) || (flags & ~BN_SCAN_FLAGS_ALL) || !offsets || offsets[0] != 0) return BN254_E_BAD_ARG;
    for (size_t j = 0; j < m; ++j)
        if (offsets[j + 1] < offsets[j]) return BN254_E_BAD_ARG;
    return (offsets[m] > BN_N_MAX || !out) ? BN254_E_BAD_ARG : BN254_OK;
}
// Every segment of L > 0 terms is cut into k = ceil(L / P) pieces of at most P consecutive terms, in the order of the recurrence (REVERSE:
// piece 0 holds the LAST terms and every piece walks downwards), one lane each in the APPLY level.  k == 1: the piece is "direct" - it starts
// from init[j] and needs nothing else.  Otherwise the pieces own scratch slots base .. base + k - 1 (the slot of a piece holds its map and
// the value in front of it), and the segment takes part in
//   REDUCE   once, over the work list of the apply level (a direct piece returns at once): every piece writes its map;
//   UP       u(k) levels, u(k) = the number of times k -> ceil(k / F) is taken while k > F (max(0, ceil(log_F k) - 1)): a lane composes at most F
//            consecutive maps of the level below into a slot of its own;
//   DOWN     u(k) + 1 levels: at the top ONE lane walks the at most F maps that are left from init[j]; below it a lane per slot of the level
//            above walks that slot's at most F children from the slot's carry;
//   APPLY    once.
// So a segment of L <= P terms is one level and a longer one 2 u(ceil(L / P)) + 3; a call runs the levels of its longest segment, shorter
// segments simply have no piece in the deeper ones.  No map and no carry is written twice, and a level reads only what earlier levels wrote,
// so a level may run as any number of sub-launches in any order after the level before it.  Slots: k (1 + 1/F + 1/F^2 + ..) + u < 2 k + 64
// per long segment, fewer than 2 n / P + 64 m in all; an empty segment has no piece at all.
enum BnScanKind { BN_SCAN_REDUCE, BN_SCAN_UP, BN_SCAN_DOWN, BN_SCAN_APPLY };
struct BnScanLevel { BnScanKind kind; size_t first, count; };       // a range of the work list
struct BnScanPlan {
    std::vector<bn254::BnScanPiece> pieces;                 // the apply level (shared with reduce), then the up levels, then the down levels
    std::vector<BnScanLevel> levels;                        // in launch order
    size_t slots = 0;                                       // scratch slots: a map (A, B) and a carry each
};
inline bn254::BnScanPiece bn_scan_piece(uint64_t first, size_t len, bool flag, uint64_t seg, uint64_t slot) {
    return {first | (uint64_t)len << 48 | (uint64_t)(flag ? 1 : 0) << 63, seg, slot};
}
inline BnScanPlan bn_scan_plan(const size_t *off, size_t m, size_t P, size_t F, bool reverse) {
    BnScanPlan plan;
    std::vector<bn254::BnScanPiece> apply;
    std::vector<std::vector<bn254::BnScanPiece>> up, down;
    apply.reserve(m + off[m] / P);
    for (size_t j = 0; j < m; ++j) {
        const size_t L = off[j + 1] - off[j];
        if (L == 0) continue;
        const size_t start = reverse ? off[j + 1] - 1 : off[j];
        if (L <= P) { apply.push_back(bn_scan_piece(start, L, true, j, 0)); continue; }
        size_t k = (L + P - 1) / P;
        std::vector<std::pair<size_t, size_t>> lv{{plan.slots, k}};               // (first slot, count) of every level of this segment's tree
        for (size_t i = 0; i < k; ++i) apply.push_back(bn_scan_piece(reverse ? start - i * P : start + i * P, std::min(P, L - i * P), false, j, plan.slots + i));
        plan.slots += k;
        for (size_t level = 0; k > F; ++level) {
            const size_t k2 = (k + F - 1) / F, src = lv.back().first, dst = plan.slots;
            if (up.size() <= level) up.emplace_back();
            for (size_t i = 0; i < k2; ++i) up[level].push_back(bn_scan_piece(src + i * F, std::min(F, k - i * F), false, j, dst + i));
            plan.slots += k2; lv.push_back({dst, k2}); k = k2;
        }
        if (down.size() < lv.size()) down.resize(lv.size());
        down[0].push_back(bn_scan_piece(lv.back().first, lv.back().second, true, j, 0));
        for (size_t d = 1; d < lv.size(); ++d) {
            const auto parent = lv[lv.size() - d], child = lv[lv.size() - 1 - d];
            for (size_t i = 0; i < parent.second; ++i) down[d].push_back(bn_scan_piece(child.first + i * F, std::min(F, child.second - i * F), false, j, parent.first + i));
        }
    }
    plan.pieces = std::move(apply);
    const size_t lanes = plan.pieces.size();
    if (!down.empty()) plan.levels.push_back({BN_SCAN_REDUCE, 0, lanes});
    for (const auto &l : up) { plan.levels.push_back({BN_SCAN_UP, plan.pieces.size(), l.size()}); plan.pieces.insert(plan.pieces.end(), l.begin(), l.end()); }
    for (const auto &l : down) { plan.levels.push_back({BN_SCAN_DOWN, plan.pieces.size(), l.size()}); plan.pieces.insert(plan.pieces.end(), l.begin(), l.end()); }
    plan.levels.push_back({BN_SCAN_APPLY, 0, lanes});
    return plan;
}

// ---- multilinear tables and sumcheck rounds over Fr (bn254_fr_mle_eq, bn254_fr_mle_fold, bn254_fr_sumcheck_round): the argument checks and the levels
inline int bn_mle_eq_check(const void *z, int nv, const void *out) { return (nv < 0 || nv > BN254_MLE_VARS_MAX || !out || (nv && !z)) ? BN254_E_BAD_ARG : BN254_OK; }
// for len > 0: an even number of records, one challenge
inline int bn_mle_fold_check(const void *in, size_t len, const void *r, const void *out) { return ((len & 1) || len > BN_N_MAX || !in || !r || !out) ? BN254_E_BAD_ARG : BN254_OK; }
// sizes, pointers and the groups in CSR form (offsets[0] == 0, every group of 1 .. degree table numbers below k); fills the record the
// round kernel reads.  group_coeff: g Montgomery images of four 64-bit limbs, copied as eight 32-bit words.
inline int bn_sumcheck_check(const void *tables, size_t n, size_t k, const size_t *offsets, const uint64_t *group_tables, const bn_fr *coeff, size_t g, int degree, const void *out,
                             bn254::BnSumcheckDesc *desc) {
    static_assert(BN254_SUMCHECK_GROUPS_MAX == bn254::BN_SUMCHECK_GROUPS && BN254_SUMCHECK_DEGREE_MAX == bn254::BN_SUMCHECK_FACTORS && BN254_SUMCHECK_TABLES_MAX <= 256,
                  "io.hpp BnSumcheckDesc mirrors the header's limits");
    if (!tables || !offsets || !group_tables || !coeff || !out) return BN254_E_BAD_ARG;
    if (n < 2 || (n & 1) || k < 1 || k > BN254_SUMCHECK_TABLES_MAX || g < 1 || g > BN254_SUMCHECK_GROUPS_MAX || degree < 1 || degree > BN254_SUMCHECK_DEGREE_MAX) return BN254_E_BAD_ARG;
    if (n > BN_N_MAX / k || offsets[0] != 0) return BN254_E_BAD_ARG;
    memset(desc, 0, sizeof *desc);
    desc->groups = (uint32_t)g;
    for (size_t c = 0; c < g; ++c) {
        if (offsets[c + 1] <= offsets[c] || offsets[c + 1] - offsets[c] > (size_t)degree) return BN254_E_BAD_ARG;
        desc->len[c] = (uint8_t)(offsets[c + 1] - offsets[c]);
        for (size_t f = 0; f < desc->len[c]; ++f) {
            const uint64_t j = group_tables[offsets[c] + f];
            if (j >= k) return BN254_E_BAD_ARG;
            desc->table[c][f] = (uint8_t)j;
        }
        memcpy(desc->coeff[c], coeff[c].l, sizeof desc->coeff[c]);
    }
    return BN254_OK;
}
// A round over h = n / 2 indices: lanes = ceil(h / P) lanes of the round kernel, lane l summing the indices l, l + lanes, .. (at most P).  One
// lane writes out and that is all.  Otherwise the lanes write (degree + 1) * lanes partial sums, laid out [t][lane], to the front of the scratch, and sum
// levels follow: a level over cnt sums per t has (degree + 1) * ceil(cnt / F) lanes and writes as many sums, [t][lane] again, behind its
// input - the last level (ceil(cnt / F) == 1) to out instead.  ceil(log_F lanes) levels; slots: (degree + 1) * lanes * (1 + 1/F + ..) < 2 (degree + 1) * lanes.
// No slot is written twice, so a level may run as any number of sub-launches in any order after the level before it.
struct BnSumcheckLevel { size_t cnt, lanes, src, dst; bool to_out; };        // src, dst: first scratch slot
struct BnSumcheckPlan {
    size_t lanes = 0;                                       // of the round kernel
    std::vector<BnSumcheckLevel> levels;                    // the sum levels, in launch order
    size_t slots = 0;                                       // scratch records of 32 bytes
};
inline BnSumcheckPlan bn_sumcheck_plan(size_t h, unsigned degree, size_t P, size_t F) {
    BnSumcheckPlan plan;
    plan.lanes = (h + P - 1) / P;
    if (plan.lanes <= 1) return plan;
    const size_t T = degree + 1;
    size_t cnt = plan.lanes, src = 0;
    plan.slots = T * cnt;
    for (;;) {
        const size_t cnt2 = (cnt + F - 1) / F;
        plan.levels.push_back({cnt, T * cnt2, src, plan.slots, cnt2 == 1});
        if (cnt2 == 1) break;
        src = plan.slots; plan.slots += T * cnt2; cnt = cnt2;
    }
    return plan;
}

// ---- the fused fold-then-round call (bn254_fr_sumcheck_fold_round): the argument check and the indices per lane
inline bool bn_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb ? pb - pa < a_bytes : pa - pb < b_bytes;
}
// n = 4 h2 rows of k tables are folded to n / 2 rows, and the round runs over those: everything bn_sumcheck_check rejects for
// (n / 2, k, groups, degree), a whole number of row quadruples, one challenge, n k within the limit.  `folded` (n / 2 * k records) may be
// exactly `tables` (n k records) and must not overlap it otherwise; `out` (degree + 1 records) must overlap neither.
inline int bn_sumcheck_fold_check(const void *tables, size_t n, size_t k, const void *r, const size_t *offsets, const uint64_t *group_tables, const bn_fr *coeff, size_t g, int degree,
                                  const void *folded, const void *out, bn254::BnSumcheckDesc *desc) {
    if (n < 4 || (n & 3) || !r || !folded) return BN254_E_BAD_ARG;
    const int rc = bn_sumcheck_check(tables, n / 2, k, offsets, group_tables, coeff, g, degree, out, desc); if (rc) return rc;
    if (n > BN_N_MAX / k) return BN254_E_BAD_ARG;
    const size_t table_bytes = n * k * sizeof(bn_fr), out_bytes = (size_t)(degree + 1) * sizeof(bn_fr);
    if (folded != tables && bn_ranges_overlap(tables, table_bytes, folded, table_bytes / 2)) return BN254_E_BAD_ARG;
    if (bn_ranges_overlap(tables, table_bytes, out, out_bytes) || bn_ranges_overlap(folded, table_bytes / 2, out, out_bytes)) return BN254_E_BAD_ARG;
    return BN254_OK;
}
// Indices per lane of the fused kernel over h2 indices: the shipped P, halved down to 4 while its ceil(h2 / P) lanes are fewer than `fill` -
// the lanes that occupy every SIMD with the two waves these kernels hold from degree 2 on, cus * 4 SIMDs * 64 lanes * 2.  A prover walks
// through every size, and below `fill` lanes a long piece only leaves compute units idle.  The bytes do not depend on P.
inline size_t bn_sumcheck_fold_fill(size_t cus) { return cus * 4 * 64 * 2; }
inline size_t bn_sumcheck_fold_piece(size_t h2, size_t P, size_t fill) {
    while (P > 4 && (h2 + P - 1) / P < fill) P /= 2;
    return P;
}

// ---- the quotients of a multilinear opening (bn254_fr_mle_quotients): the argument check and the passes
// a and out hold 2^nv records of 32 bytes each and must not overlap (a pass reads a while the quotients of its levels are written)
inline int bn_mle_quotients_check(const void *a, int nv, const void *z, const void *out) {
    if (nv < 0 || nv > BN254_MLE_VARS_MAX || !a || !out || (nv && !z)) return BN254_E_BAD_ARG;
    const uintptr_t pa = (uintptr_t)a, po = (uintptr_t)out, bytes = (uintptr_t)sizeof(bn_fr) << nv;
    return (pa < po ? po - pa < bytes : pa - po < bytes) ? BN254_E_BAD_ARG : BN254_OK;
}
// The nv levels of a call run as passes of `rho` levels each, the full ones first, and the remainder nv mod rho last, on the small table.  A
// pass of `levels` levels over the working table of 2^vars records has lanes = 2^(vars - levels) lanes; lane i reads the records i + c * lanes,
// c < 2^levels, writes the quotient of level k (k < levels, variable j = vars - 1 - k) at index i + c * lanes, c < 2^(levels - 1 - k), to record
// 2^j + i + c * lanes of the output, and record i of the folded table.  The first pass reads `a` and writes the folded table to the scratch
// (`slots` records: its lanes); the later ones read the scratch and write it in place.  The last pass has one lane and its folded record is
// record 0 of the output.  nv == 0 has no pass: the one record is copied.
struct BnMleQuotPass { unsigned levels, vars; size_t lanes; bool first, last; };
struct BnMleQuotPlan {
    std::vector<BnMleQuotPass> passes;
    size_t slots = 0;                                       // scratch records of 32 bytes
};
inline BnMleQuotPlan bn_mle_quotients_plan(unsigned nv, unsigned rho) {
    BnMleQuotPlan plan;
    for (unsigned vars = nv; vars > 0;) {
        const unsigned levels = vars >= rho ? rho : vars;
        plan.passes.push_back({levels, vars, (size_t)1 << (vars - levels), vars == nv, vars == levels});
        vars -= levels;
    }
    if (!plan.passes.empty()) plan.slots = plan.passes[0].lanes;
    return plan;
}

// ---- Poseidon hashes and Merkle trees over Fr (bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch, bn254_fr_merkle_tree): the argument checks and the levels
// n states of t records (a hash of arity t - 1 reads n * (t - 1) of them: the bound is taken on n * t either way); n == 0 is answered before
inline int bn_poseidon_check(const void *in, int t, const void *out, size_t n) {
    if (t < 2 || t > BN254_POSEIDON_ARITY_MAX + 1) return BN254_E_BAD_ARG;
    return (n > BN_N_MAX / (size_t)t || !in || !out) ? BN254_E_BAD_ARG : BN254_OK;
}
inline int bn_merkle_check(const void *leaves, int log_n, const void *nodes) {
    if (log_n < 0 || log_n > BN254_MERKLE_LOG_MAX) return BN254_E_BAD_ARG;
    return (log_n > 0 && (!leaves || !nodes)) ? BN254_E_BAD_ARG : BN254_OK;
}
// The tree over n = 2^log_n leaves: log_n levels, level l (from 0) of n >> (l + 1) parents.  Level 0 reads the leaves, level l > 0 the nodes
// from `src`; every level writes the nodes from `dst`, behind the level before it, so the root is node n - 2 and no record is written twice.
// `parts`: the sub-launches of at most `step` lanes the level is cut into.
struct BnMerkleLevel { size_t cnt, src, dst, parts; bool from_leaves; };
inline std::vector<BnMerkleLevel> bn_merkle_plan(int log_n, size_t step) {
    std::vector<BnMerkleLevel> levels;
    size_t src = 0, dst = 0;
    for (int l = 0; l < log_n; ++l) {
        const size_t cnt = (size_t)1 << (log_n - 1 - l);
        levels.push_back({cnt, src, dst, (cnt + step - 1) / step, l == 0});
        src = dst; dst += cnt;
    }
    return levels;
}

// ---- the wide Poseidon calls (bn254_fr_poseidon_ex_batch, bn254_fr_poseidon_chain_batch): the argument checks.  The ranges of n_inputs, n_outs and
// rate are answered even for an empty call; with work to do, pointers and sizes follow.
inline int bn_poseidon_ex_range(int n_inputs, int n_outs) {
    return (n_inputs < 1 || n_inputs > BN254_POSEIDON_EX_INPUTS_MAX || n_outs < 1 || n_outs > n_inputs + 1) ? BN254_E_BAD_ARG : BN254_OK;
}
// n > 0 rows: `init` may be NULL; host_buffers: `out` (n * n_outs records) must overlap neither `in` (n * n_inputs) nor `init` (n)
inline int bn_poseidon_ex_check(const void *in, int n_inputs, const void *init, int n_outs, const void *out, size_t n, bool host_buffers) {
    const int rc = bn_poseidon_ex_range(n_inputs, n_outs); if (rc) return rc;
    if (!in || !out || n > BN_N_MAX / (size_t)(n_inputs + 1)) return BN254_E_BAD_ARG;
    if (!host_buffers) return BN254_OK;
    const size_t rec = 32, out_bytes = n * (size_t)n_outs * rec;
    if (bn_ranges_overlap(in, n * (size_t)n_inputs * rec, out, out_bytes) || (init && bn_ranges_overlap(init, n * rec, out, out_bytes))) return BN254_E_BAD_ARG;
    return BN254_OK;
}
// m > 0 records: CSR offsets in host memory (m + 1 entries from 0, non-decreasing), at most 2^40 records and 2^40 elements
inline int bn_poseidon_chain_check(const void *in, const size_t *offsets, size_t m, int rate, const void *out, bool host_buffers) {
    if (rate < 1 || rate > BN254_POSEIDON_EX_INPUTS_MAX) return BN254_E_BAD_ARG;
    if (!offsets || !out || m > BN_N_MAX || offsets[0] != 0) return BN254_E_BAD_ARG;
    for (size_t j = 0; j < m; ++j)
        if (offsets[j + 1] < offsets[j]) return BN254_E_BAD_ARG;
    const size_t n = offsets[m];
    if (n > BN_N_MAX || (n && !in)) return BN254_E_BAD_ARG;
    return (host_buffers && n && bn_ranges_overlap(in, n * 32, out, m * 32)) ? BN254_E_BAD_ARG : BN254_OK;
}
