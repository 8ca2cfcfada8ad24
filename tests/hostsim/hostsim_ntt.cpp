// TEST INFRASTRUCTURE - host simulation of the bodies of bn254_fr_ntt_batch (bn_amd/csrc/ntt_ops.hpp over fr.hpp, planned by host_plan.hpp's
// bn_ntt_plan) compiled with g++ for the CPU: the very code the kernels run - table build, load, stages, store -, one loop over lanes where
// the kernel has a __syncthreads(), one loop over workgroups per launch, over host arrays, for ANY tile log.  The tile accessor counts
// every index past the tile.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // host_plan.hpp reaches the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/ntt_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

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
    for (uint32_t i = 0; i < 2 * NTT_TBL + 3; ++i) ntt_table_body(out, fr_of(c0), fr_of(g0), fr_of(one.l), fr_of(g1.l), i);     // lanes past the table retire
}
void launch(const NttPass &K, size_t blocks) {
    std::vector<uint32_t> tile((size_t)8 << K.T), tw((size_t)8 << K.T >> 1);
    for (size_t wg = 0; wg < blocks; ++wg) {
        std::fill(tile.begin(), tile.end(), 0xa5a5a5a5u);
        std::fill(tw.begin(), tw.end(), 0xa5a5a5a5u);
        for (uint32_t lane = 0; lane < NTT_BLOCK; ++lane) ntt_twiddle_lane(K, tw.data(), lane);
        for (uint32_t lane = 0; lane < NTT_BLOCK; ++lane) ntt_load_lane(K, tile.data(), (uint32_t)wg, lane);
        for (uint32_t st = 0; st < K.t; ++st)
            for (uint32_t lane = 0; lane < NTT_BLOCK; ++lane) ntt_stage_lane(K, tile.data(), tw.data(), (uint32_t)wg, lane, st);
        for (uint32_t lane = 0; lane < NTT_BLOCK; ++lane) ntt_store_lane(K, tile.data(), (uint32_t)wg, lane);
    }
}
}  // namespace

EXPORT uint32_t hsn_shipped_tile_log() { return NTT_TILE_LOG; }
EXPORT int hsn_root(int log_n, uint64_t *out) { return bn_fr_root(log_n, (bn_fr *)out); }
EXPORT uint32_t hsn_passes(uint32_t log_n, uint32_t T) { BnNttPass plan[BN_NTT_PASSES_MAX]; return bn_ntt_plan(log_n, T, plan); }
// out = a * b and a^-1 through the host arithmetic of host_plan.hpp
EXPORT void hsn_host_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) { bn_fr_mul(a, b, out); }
EXPORT void hsn_host_inverse(const uint64_t *a, uint64_t *out) { bn_fr_inverse(a, out); }

// bn254_fr_ntt_batch_dev over host arrays: the groups, passes, buffers and sub-launches are the shipped planner's (host_plan.hpp bn_ntt_run
// / bn_ntt_group, which bn254_ntt.hip's ntt_run walks in the same way) with tile log T and sub-launches of `step` elements; out may be in.
// The workspace holds exactly the arrays the plan asks for.  Returns the number of tile accesses out of range, or -1 when a step names a
// workspace array the plan did not ask for.
EXPORT int hsn_ntt(const uint32_t *d_in, uint32_t *d_out, uint32_t log_n, size_t count, int inverse, const uint64_t *shift, uint32_t T, size_t step) {
    ntt_tile_errors = 0;
    static std::vector<uint32_t> tbl;                                           // like the context: the root pair once, the shift pair per key
    static uint64_t key[5];
    static bool key_valid = false;
    bn_fr one, w, scale;
    bn_fr_one(&one); bn_fr_root((int)NTT_LOG_MAX, &w);
    if (tbl.empty()) {
        tbl.assign((size_t)8 * 4 * NTT_TBL, 0xffffffffu);
        build_pair(tbl.data(), one.l, w.l);
    }
    bn_fr_inv_pow2(log_n, &scale);
    if (shift) {
        const uint64_t now[5] = {shift[0], shift[1], shift[2], shift[3], inverse ? (uint64_t)log_n << 1 | 1u : 0u};
        if (!key_valid || memcmp(now, key, sizeof key)) {
            bn_fr g0;
            memcpy(g0.l, shift, sizeof g0.l);
            if (inverse) bn_fr_inverse(shift, g0.l);
            build_pair(tbl.data() + 8 * 2 * NTT_TBL, inverse ? scale.l : one.l, g0.l);
            memcpy(key, now, sizeof key); key_valid = true;
        }
    }
    const size_t N = (size_t)1 << log_n;
    const bool in_place = d_in == d_out;
    const BnNttRun run = bn_ntt_run(log_n, T, count, step, in_place);
    std::vector<uint32_t> ws(run.ws_bufs * 8 * run.most, 0x5a5a5a5au);
    NttPass K = {};
    K.wtbl = tbl.data(); K.stbl = tbl.data() + 8 * 2 * NTT_TBL;
    K.log_n = log_n; K.T = T; K.inverse = inverse != 0;
    K.scale = fr_of(scale.l);
    for (size_t tr0 = 0; tr0 < count; tr0 += run.per_group) {
        const size_t cnt = std::min(run.per_group, count - tr0);
        uint32_t *const buf[4] = {(uint32_t *)d_in + 8 * tr0 * N, d_out + 8 * tr0 * N, ws.data(), ws.data() + 8 * run.most};
        const int rc = bn_ntt_group(run, log_n, T, cnt, step, in_place, shift != nullptr, inverse != 0, [&](const BnNttStep &st) -> int {
            if ((st.src == BN_NTT_WS0 || st.dst == BN_NTT_WS0) && run.ws_bufs < 1) return -1;
            if ((st.src == BN_NTT_WS1 || st.dst == BN_NTT_WS1) && run.ws_bufs < 2) return -1;
            if (st.dst == BN_NTT_IN || (run.P > 1 && st.src == st.dst)) return -1;
            K.in = buf[st.src]; K.out = buf[st.dst];
            K.t = st.g.t; K.log_m = st.g.log_m; K.log_s = st.g.log_s;
            K.pre = st.pre; K.post = st.post;
            K.tile_lo = (uint32_t)st.lo; K.tile_end = (uint32_t)(st.lo + st.n);
            launch(K, st.blocks + 1);                                          // one workgroup more than needed: it must retire
            return 0;
        });
        if (rc) return rc;
    }
    return ntt_tile_errors;
}
