// TEST INFRASTRUCTURE - host simulation of bn254_g{1,2}_ntt_batch_dev (bn_amd/csrc/group_ntt_ops.hpp: the butterfly and pass bodies;
// group_ops.hpp normalize_body; host_plan.hpp bn_group_ntt_run / bn_group_ntt_group: the steps) compiled with g++ for the CPU: the very
// code the kernels run, one loop over lanes (G1) or simulated lane pairs (G2) per launch, over host arrays, walked the way
// bn254_group_ntt.hip walks the plan.  Built with -DBN_BOUNDS by tests/test_hostsim_group_ntt.py: every limb / value bound of the lazy
// number system is enforced at run time.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "lanequad.hpp"
#include "../../bn_amd/csrc/group_ntt_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))
typedef FqField G1S;
typedef Fq2Field<Fq2B<FeP>> G2S;

namespace {
Fr fr_of(const uint64_t *l) {
    Fr r;
    for (int i = 0; i < 4; ++i) { r.w[2 * i] = (uint32_t)l[i]; r.w[2 * i + 1] = (uint32_t)(l[i] >> 32); }
    return r;
}
void build_pair(uint32_t *out, const uint64_t *c0, const uint64_t *g0) {
    const uint64_t e[4] = {NTT_TBL, 0, 0, 0};
    bn_fr one, g1;
    bn_fr_one(&one);
    bn_fr_pow(g0, e, g1.l);
    for (uint32_t i = 0; i < 2 * NTT_TBL; ++i) ntt_table_body(out, fr_of(c0), fr_of(g0), fr_of(one.l), fr_of(g1.l), i);
}
// the root table pair of every call: the powers of w_24
const uint32_t *root_pair() {
    static std::vector<uint32_t> tbl;
    if (tbl.empty()) {
        tbl.assign((size_t)8 * 2 * NTT_TBL, 0xffffffffu);
        bn_fr one, w;
        bn_fr_one(&one); bn_fr_root((int)NTT_LOG_MAX, &w);
        build_pair(tbl.data(), one.l, w.l);
    }
    return tbl.data();
}
// the shift table pair of a call: s^j forward, n^-1 s^-j inverse
void shift_pair(uint32_t *out, uint32_t log_n, int inverse, const uint64_t *shift) {
    bn_fr one, n_inv, g0;
    bn_fr_one(&one); bn_fr_inv_pow2(log_n, &n_inv);
    memcpy(g0.l, shift, sizeof g0.l);
    if (inverse) bn_fr_inverse(shift, g0.l);
    build_pair(out, inverse ? n_inv.l : one.l, g0.l);
}
// a simulated lane pair holds both components of a prefix product: it keeps both records (tests/hostsim/hostsim_normalize.cpp)
struct PrefixPair {
    uint4 *base;
    void put(uint32_t j, const Fq2B<FeP> &a) const {
        prefix_record_put(a.v.v[0], base + (size_t)j * 2 * NORM_PREFIX_U4); prefix_record_put(a.v.v[1], base + ((size_t)j * 2 + 1) * NORM_PREFIX_U4);
    }
    Fq2B<FeP> get(uint32_t j) const {
        return {{{prefix_record_get(base + (size_t)j * 2 * NORM_PREFIX_U4), prefix_record_get(base + ((size_t)j * 2 + 1) * NORM_PREFIX_U4)}}};
    }
};
size_t g_chains = 0;          // chains run since the last reset: the bodies with a window table
template <class F>
void stage(const GroupNttStageArgs &a, size_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        if (a.stage == 0) { group_ntt_stage0_body<F>(a, i, PointIo<F>()); continue; }
        AffTableVars<F> tab;
        group_ntt_stage_body<F>(a, i, tab, PointIo<F>());
        ++g_chains;
    }
}
template <class F>
void scale(const GroupNttScaleArgs &a, size_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        AffTableVars<F> tab;
        group_ntt_scale_body<F>(a, i, tab, PointIo<F>());
        ++g_chains;
    }
}
void normalize(int g, const uint32_t *p, uint32_t *out, uint32_t n) {
    std::vector<uint4> prefix((size_t)n * (g == 1 ? 1 : 2) * NORM_PREFIX_U4 + 1, uint4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu});
    const NormalizeArgs a = {p, out, prefix.data(), n};
    for (uint32_t i = 0; i < (n + NORM_RUN - 1) / NORM_RUN + 1; ++i) {
        if (g == 1) normalize_body<G1S>(a, i, NORM_RUN, PrefixMem<G1S>{a.prefix, 0u}, PointIo<G1S>());
        else normalize_body<G2S>(a, i, NORM_RUN, PrefixPair{a.prefix}, PointIo<G2S>());
    }
}
}  // namespace

EXPORT int hsg_bounds_enabled() {
#ifdef BN_BOUNDS
    return 1;
#else
    return 0;
#endif
}
EXPORT size_t hsg_chains() { return g_chains; }
EXPORT int hsg_check(const void *in, const void *out, int log_n, size_t count, const uint64_t *shift) { return bn_group_ntt_check(in, out, log_n, count, (const bn_fr *)shift); }
// The plan of a call without a device (tests/test_host_plan_group_ntt.py): head = {stages, pre, post, per_group, most, ws_bufs}; every
// sub-launch as eight numbers {first transform of its group, kind, stage, src, dst, chain, lo, n}.  Returns their number (only the first
// `cap_steps` are written).
EXPORT size_t hsg_plan(uint32_t log_n, size_t count, size_t cap, size_t chain_cap, int shift, int inverse, uint64_t *head, uint64_t *steps, size_t cap_steps) {
    const BnGroupNttRun run = bn_group_ntt_run(log_n, count, cap, shift != 0, inverse != 0);
    head[0] = run.stages; head[1] = run.pre; head[2] = run.post; head[3] = run.per_group; head[4] = run.most; head[5] = run.ws_bufs;
    size_t k = 0;
    bn_for_parts(count, run.per_group, [&](size_t tr0, size_t cnt) -> int {
        return bn_group_ntt_group(run, log_n, cnt, cap, chain_cap, [&](const BnGroupNttStep &st) -> int {
            if (k < cap_steps) {
                const uint64_t rec[8] = {tr0, (uint64_t)st.kind, st.stage, (uint64_t)st.src, (uint64_t)st.dst, st.chain ? 1u : 0u, st.lo, st.n};
                memcpy(steps + 8 * k, rec, sizeof rec);
            }
            ++k;
            return 0;
        });
    });
    return k;
}
// the records a butterfly reads and writes and the exponent of its twiddle: out = {a, b, o0, o1, e}
EXPORT void hsg_index(uint32_t log_n, uint32_t stage, uint32_t g, uint32_t *out) {
    const GroupNttIdx x = group_ntt_index(log_n, stage, g);
    out[0] = x.a; out[1] = x.b; out[2] = x.o0; out[3] = x.o1; out[4] = x.e;
}
// the twiddle group_ntt_stage_body multiplies record b of butterfly g with, by its own calls over the root table pair: eight Montgomery words
EXPORT void hsg_twiddle(uint32_t log_n, uint32_t stage, uint32_t g, int inverse, uint32_t *out) {
    const GroupNttIdx x = group_ntt_index(log_n, stage, g);
    NttPass P = {};
    P.wtbl = root_pair(); P.inverse = inverse ? 1u : 0u;
    const Fr w = ntt_root_power(P, x.e);
    memcpy(out, w.w, sizeof w.w);
}
// the factor group_ntt_scale_body multiplies point j of the arrays with, by its own calls over the shift table pair hsg_ntt builds (kept
// until another log_n, direction or shift is asked for); shift == nullptr: the `scale` of an inverse, n^-1.  Eight Montgomery words.
EXPORT void hsg_scale_factor(uint32_t log_n, uint32_t j, int inverse, const uint64_t *shift, uint32_t *out) {
    static std::vector<uint32_t> stbl;
    static uint64_t key[6] = {~0ull, 0, 0, 0, 0, 0};
    bn_fr n_inv;
    bn_fr_inv_pow2(log_n, &n_inv);
    Fr c = fr_of(n_inv.l);
    if (shift) {
        const uint64_t want[6] = {log_n, inverse ? 1u : 0u, shift[0], shift[1], shift[2], shift[3]};
        if (stbl.empty() || memcmp(key, want, sizeof key)) {
            stbl.assign((size_t)8 * 2 * NTT_TBL, 0xffffffffu);
            shift_pair(stbl.data(), log_n, inverse, shift);
            memcpy(key, want, sizeof key);
        }
        NttPass P = {};
        P.stbl = stbl.data(); P.log_n = log_n;
        c = ntt_shift_power(P, j & ((1u << log_n) - 1u));
    }
    memcpy(out, c.w, sizeof c.w);
}
// bn254_g{1,2}_ntt_batch_dev over host arrays with sub-launches of `cap` units and chain launches of at most `chain_cap`; d_out may be d_in.
// The workspace is filled with a pattern that is no point, and IN is compared with a copy afterwards unless it is OUT.  Returns 0, -1 when a
// step breaks the buffer rules of the plan, -2 when IN was written.
EXPORT int hsg_ntt(int g, const uint32_t *d_in, uint32_t *d_out, uint32_t log_n, size_t count, int inverse, const uint64_t *shift, size_t cap, size_t chain_cap) {
    g_chains = 0;
    const size_t W = g == 1 ? PointIo<G1S>::WORDS : PointIo<G2S>::WORDS, N = (size_t)1 << log_n;
    const uint32_t *const wtbl = root_pair();
    std::vector<uint32_t> stbl((size_t)8 * 2 * NTT_TBL, 0xffffffffu);
    bn_fr n_inv;
    bn_fr_inv_pow2(log_n, &n_inv);
    if (shift) shift_pair(stbl.data(), log_n, inverse, shift);
    const bool in_place = d_in == d_out;
    const std::vector<uint32_t> in_copy(d_in, d_in + count * N * W);
    const BnGroupNttRun run = bn_group_ntt_run(log_n, count, cap, shift != nullptr, inverse != 0);
    std::vector<uint32_t> ws(run.ws_bufs * run.most * W, 0xffffffffu);
    for (size_t tr0 = 0; tr0 < count; tr0 += run.per_group) {
        const size_t cnt = std::min(run.per_group, count - tr0);
        if ((cnt << log_n) > run.most && run.ws_bufs) return -1;
        uint32_t *const buf[3] = {(uint32_t *)d_in + tr0 * N * W, d_out + tr0 * N * W, ws.data()};
        const int rc = bn_group_ntt_group(run, log_n, cnt, cap, chain_cap, [&](const BnGroupNttStep &st) -> int {
            if ((st.src == BN_NTT_WS0 || st.dst == BN_NTT_WS0) && !run.ws_bufs) return -1;
            if (st.dst == BN_NTT_IN || st.src > BN_NTT_WS0 || st.dst > BN_NTT_WS0) return -1;
            if (st.kind == BN_GNTT_STAGE && (st.src == st.dst || (in_place && st.src == BN_NTT_IN && st.dst == BN_NTT_OUT))) return -1;
            if (st.n > (st.chain ? std::min(cap, chain_cap) : cap)) return -1;
            if (st.kind == BN_GNTT_STAGE) {
                const GroupNttStageArgs a = {buf[st.src], buf[st.dst], wtbl, log_n, st.stage, inverse ? 1u : 0u, (uint32_t)st.lo};
                if (g == 1) stage<G1S>(a, st.n); else stage<G2S>(a, st.n);
            } else if (st.kind == BN_GNTT_SCALE) {
                const GroupNttScaleArgs a = {buf[st.src], buf[st.dst], stbl.data(), log_n, shift ? 1u : 0u, (uint32_t)st.lo, fr_of(n_inv.l)};
                if (g == 1) scale<G1S>(a, st.n); else scale<G2S>(a, st.n);
            } else {
                normalize(g, buf[st.src] + st.lo * W, buf[st.dst] + st.lo * W, (uint32_t)st.n);
            }
            return 0;
        });
        if (rc) return rc;
    }
    if (!in_place && memcmp(in_copy.data(), d_in, in_copy.size() * 4)) return -2;
    return 0;
}
