// TEST INFRASTRUCTURE - host simulation of the multi-scalar multiplication against prepared bases (bn254_g{1,2}_msm_prepare / _prepared):
// the bodies of bn_amd/csrc/group_ops.hpp (msm_signed_digit, msm_prep_double_body, msm_acc_prep_body and, above level 0 and for the
// reduction, the bodies the bucket method already had) and the planner of bn_amd/csrc/host_plan.hpp, compiled with g++ for the CPU: the very
// code the kernels and the host unit run, one loop over lanes (G1) or simulated lane pairs (G2) per launch, over host arrays.  Built with
// -DBN_BOUNDS by tests/hostsim_msm_prepared_lib.py: every limb / value bound of the lazy number system is enforced at run time.  Never
// loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "lanequad.hpp"
#include "../../bn_amd/csrc/group_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <algorithm>
#include <cstring>
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))
typedef FqField G1S;
typedef Fq2Field<Fq2B<FeP>> G2S;

EXPORT int hsp_bounds_enabled() {
#ifdef BN_BOUNDS
    return 1;
#else
    return 0;
#endif
}
EXPORT uint32_t hsp_piece() { return MSM_PIECE; }
// the W signed digits of the canonical integer `raw` (8 words): |d| and the sign of every window; returns the carry the top window leaves
EXPORT uint32_t hsp_signed_digits(const uint32_t *raw, uint32_t c, uint32_t *mag, uint32_t *neg) {
    const uint32_t W = (254 + c - 1) / c;
    uint32_t carry = 0;
    for (uint32_t w = 0; w < W; ++w) { bool n; mag[w] = msm_signed_digit(raw, w, c, carry, n); neg[w] = n ? 1u : 0u; }
    return carry;
}
// a simulated lane pair holds both components of an entry: it fetches both records (the kernel's lanes one each, BaseTableMem)
struct TablePair {
    const uint4 *table;
    Aff<G2S> get(uint32_t e, bool &inf) const {
        bool inf1;
        const Aff<FqField> c0 = base_entry<FqField>(table + (size_t)e * 2 * AFF_ENTRY_U4, inf), c1 = base_entry<FqField>(table + ((size_t)e * 2 + 1) * AFF_ENTRY_U4, inf1);
        return {{{{c0.x, c1.x}}}, {{{c0.y, c1.y}}}};
    }
};
// record `r` of a table from one component of an affine coordinate pair in the reference image, flagged when at infinity
EXPORT void hsp_record(const uint32_t *x, const uint32_t *y, uint32_t flag, uint32_t *table, uint32_t r) {
    aff_record_pack(fe_from_u32x8(x), fe_from_u32x8(y), flag, (uint4 *)table, (size_t)r);
}
// one window step of a table build: the n Jacobian points doubled c times in place, and one lane more, which the launch never has
template <class F>
static void doubles(uint32_t *pts, uint32_t n, uint32_t c) {
    const MsmPrepDoubleArgs a = {pts, c};
    for (uint32_t i = 0; i < n; ++i) msm_prep_double_body<F>(a, i, PointIo<F>());
}
EXPORT void hsp_double(int g, uint32_t *pts, uint32_t n, uint32_t c) { if (g == 1) doubles<G1S>(pts, n, c); else doubles<G2S>(pts, n, c); }
// what BaseRepackOp does with a normalised point: every component's record, flagged when z is zero
static void repack(int g, const uint32_t *p, uint4 *table, size_t e) {
    const uint32_t comps = g == 1 ? 1u : 2u;
    uint32_t z = 0;
    for (uint32_t j = 0; j < 8u * comps; ++j) z |= p[16u * comps + j];
    for (uint32_t comp = 0; comp < comps; ++comp)
        aff_record_pack(fe_from_u32x8(p + 8u * comp), fe_from_u32x8(p + 8u * comps + 8u * comp), z == 0 ? 1u : 0u, table, e * comps + comp);
}
// a simulated lane pair keeps both records of a prefix product (hostsim_normalize.cpp)
struct PrefixPair {
    uint4 *base;
    void put(uint32_t j, const Fq2B<FeP> &a) const {
        prefix_record_put(a.v.v[0], base + (size_t)j * 2 * NORM_PREFIX_U4); prefix_record_put(a.v.v[1], base + ((size_t)j * 2 + 1) * NORM_PREFIX_U4);
    }
    Fq2B<FeP> get(uint32_t j) const {
        return {{{prefix_record_get(base + (size_t)j * 2 * NORM_PREFIX_U4), prefix_record_get(base + ((size_t)j * 2 + 1) * NORM_PREFIX_U4)}}};
    }
};
// the build of a handle as bn_msmp_build runs it: window by window, normalise the running copy, repack, double c times.
// table: W * n entries of 20 (G1) / 40 (G2) words; kept: the n normalised points
EXPORT void hsp_table(int g, const uint32_t *pts, uint32_t n, uint32_t c, uint32_t *table, uint32_t *kept) {
    const uint32_t W = (254 + c - 1) / c, words = g == 1 ? 24u : 48u;
    std::vector<uint32_t> run(pts, pts + (size_t)n * words), norm((size_t)n * words);
    std::vector<uint4> prefix((size_t)n * (g == 1 ? 1 : 2) * NORM_PREFIX_U4 + 1);
    for (uint32_t w = 0; w < W; ++w) {
        const NormalizeArgs a = {run.data(), norm.data(), prefix.data(), n};
        for (uint32_t i = 0; i < (n + NORM_RUN - 1) / NORM_RUN; ++i) {
            if (g == 1) normalize_body<G1S>(a, i, NORM_RUN, PrefixMem<G1S>{a.prefix, 0u}, PointIo<G1S>());
            else normalize_body<G2S>(a, i, NORM_RUN, PrefixPair{a.prefix}, PointIo<G2S>());
        }
        if (w == 0) memcpy(kept, norm.data(), norm.size() * 4);
        for (uint32_t i = 0; i < n; ++i) repack(g, norm.data() + (size_t)i * words, (uint4 *)table, (size_t)w * n + i);
        if (w + 1 < W) hsp_double(g, run.data(), n, c);
    }
}
// the accumulation of one chunk as bn_launch_msmp_bucket runs it: level 0 from the records, the levels above by msm_acc_body, every level with
// one lane more than needed (it must retire), until one lane covers the level.  levels_out: the number of levels run.
template <class F, class Tab>
static void acc(Tab tab, const uint4 *table, const uint32_t *idx, const uint32_t *keys, uint32_t n0, uint32_t *buckets, uint32_t *levels_out) {
    const uint32_t W = PointIo<F>::WORDS;
    std::vector<uint32_t> in_pts, in_keys(keys, keys + n0), out_pts, out_keys;
    uint32_t level = 0;
    for (;; ++level) {
        const uint32_t N = msm_level_len(n0, level), lanes = (N + MSM_PIECE - 1) / MSM_PIECE;
        out_pts.assign((size_t)2 * (lanes + 1) * W, 0u); out_keys.assign((size_t)2 * (lanes + 1), 0xdeadbeefu);
        in_keys.resize(N + 1, MSM_NONE);
        if (level == 0) {
            const MsmAccPrepArgs a = {table, idx, in_keys.data(), &n0, out_pts.data(), out_keys.data(), buckets};
            for (uint32_t i = 0; i < lanes + 1; ++i) msm_acc_prep_body<F>(a, i, tab);
        } else {
            const MsmAccArgs a = {in_pts.data(), nullptr, in_keys.data(), &n0, level, out_pts.data(), out_keys.data(), buckets};
            for (uint32_t i = 0; i < lanes + 1; ++i) msm_acc_body<F>(a, i);
        }
        if (lanes <= 1) break;
        in_pts.swap(out_pts); in_keys.swap(out_keys);
    }
    *levels_out = level + 1;
}
EXPORT void hsp_acc(int g, const uint32_t *table, const uint32_t *idx, const uint32_t *keys, uint32_t n0, uint32_t *buckets, uint32_t *levels_out) {
    const uint4 *t = (const uint4 *)table;
    if (g == 1) acc<G1S>(BaseTableMem<G1S>{t, 0u}, t, idx, keys, n0, buckets, levels_out);
    else acc<G2S>(TablePair{t}, t, idx, keys, n0, buckets, levels_out);
}
// The whole route over a table of `count` points and the n scalars k (Montgomery images) against points [first, first + n), in chunks of
// `chunk` terms: digits and the counting sort (a stable sort by key stands in for the scan and the scatter), the accumulation, the one-window
// reduction.  buckets: 2^(c-1) points; terms: S of every group, then T of every group - the tail's operands.
EXPORT void hsp_route(int g, const uint32_t *table, uint32_t count, uint32_t first, const uint32_t *k, uint32_t n, uint32_t c, uint32_t chunk, uint32_t *buckets, uint32_t *terms) {
    const MsmBucketPlan bp = msm_prepared_plan(c, chunk, g == 1 ? 96 : 192, MSM_PIECE);
    const uint32_t words = g == 1 ? 24u : 48u;
    memset(buckets, 0, bp.K * words * 4);
    for (uint32_t lo = 0; lo < n; lo += chunk) {
        const uint32_t len = std::min(chunk, n - lo);
        std::vector<std::pair<uint32_t, uint32_t>> ent;                // (key, index)
        for (uint32_t i = 0; i < len; ++i) {
            uint32_t raw[8], carry = 0;
            fr_load_raw(k + 8u * (lo + i), raw);
            for (uint32_t w = 0; w < bp.W; ++w) {
                bool neg;
                const uint32_t d = msm_signed_digit(raw, w, c, carry, neg);
                if (d) ent.push_back({d - 1u, (w * count + first + lo + i) | (neg ? MSM_NEG : 0u)});
            }
        }
        std::stable_sort(ent.begin(), ent.end(), [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) { return a.first < b.first; });
        std::vector<uint32_t> idx(ent.size() + 1), keys(ent.size() + 1);
        for (size_t j = 0; j < ent.size(); ++j) { keys[j] = ent[j].first; idx[j] = ent[j].second; }
        uint32_t levels;
        hsp_acc(g, table, idx.data(), keys.data(), (uint32_t)ent.size(), buckets, &levels);
    }
    const MsmReduceArgs a = {buckets, bp.G, bp.groups, c - 1, (uint32_t)bp.count, terms};
    for (uint32_t t = 0; t < bp.count; ++t) { if (g == 1) msm_reduce_body<G1S>(a, t); else msm_reduce_body<G2S>(a, t); }
}
// ---- the planner and the checks (bn_amd/csrc/host_plan.hpp)
// head: W, G, groups, K, count, n0max, o_counts, o_tiles, o_n0, o_idx, o_keys, o_buckets, o_terms, bytes, levels; levels: (out_slots, o_points, o_keys)
EXPORT int hsp_plan(unsigned cb, size_t chunk, size_t V, size_t L, uint64_t *head, uint64_t *levels, size_t cap) {
    const MsmBucketPlan p = msm_prepared_plan(cb, chunk, V, L);
    const uint64_t h[15] = {p.W, p.G, p.groups, p.K, p.count, p.n0max, p.o_counts, p.o_tiles, p.o_n0, p.o_idx, p.o_keys, p.o_buckets, p.o_terms, p.bytes, p.out_slots.size()};
    memcpy(head, h, sizeof h);
    if (p.out_slots.size() > cap || p.o_level.size() != p.out_slots.size()) return 0;
    for (size_t i = 0; i < p.out_slots.size(); ++i) { levels[3 * i] = p.out_slots[i]; levels[3 * i + 1] = p.o_level[i].first; levels[3 * i + 2] = p.o_level[i].second; }
    return 1;
}
EXPORT size_t hsp_tail_scalars(unsigned cb, uint64_t *out, size_t cap) {           // words written (4 per scalar), or needed
    std::vector<uint64_t> h;
    msm_prepared_tail_scalars(cb, h);
    if (h.size() <= cap) memcpy(out, h.data(), h.size() * 8);
    return h.size();
}
EXPORT unsigned hsp_window_bits(size_t n) { return bn_msm_prepared_window_bits(n); }
EXPORT uint32_t hsp_level_len(uint32_t n, uint32_t level) { return msm_level_len(n, level); }
EXPORT int hsp_prepare_check(const void *p, size_t n, int window_bits, const void *out) { return bn_msm_prepare_check(p, n, window_bits, out); }
EXPORT int hsp_prepared_check(int have, int group, int g, size_t count, size_t first, const void *k, size_t n, const void *out) {
    return bn_msm_prepared_check(have != 0, group, g, count, first, k, n, out);
}
