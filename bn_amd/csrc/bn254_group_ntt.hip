// Transforms over G1 and G2 on the device (include/bn254_hip.h bn254_g{1,2}_ntt_batch and their _dev twins): the host side.  The kernels are
// bn254_kernels_mul.hip's (further instances of the generic point kernels bn254_g{1,2}_add_M<Args> over the bodies of group_ntt_ops.hpp,
// reached through its launchers only); the steps of a call - groups of transforms, stages, the passes of a shift or an inverse, the normalisation,
// their buffers and sub-launches - are host_plan.hpp's (bn_group_ntt_run, bn_group_ntt_group).  Here the buffers get their addresses and
// every step becomes one launch.  The twiddle tables are those of bn254_fr_ntt_batch (bn_ntt_tables).
#include <algorithm>

#include "host_ctx.hpp"
#include "lane_launch.hpp"

namespace {
constexpr unsigned GNTT_TBL = 1u << 12;                      // ntt_ops.hpp NTT_TBL: records per half of a table pair
// tests and tools/time_group_ntt.py only: the sub-launch size, in butterflies of a stage / points of a pass
BnLaunchMax g_gntt_launch_max;

// scratch guard held by the caller
int gntt_run(bn254_ctx *c, int g, const void *d_in, void *d_out, int log_n, size_t count, int inverse, const bn_fr *shift, hipStream_t s) {
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2), N = (size_t)1 << log_n, cap = g_gntt_launch_max.step();
    const size_t chain_cap = BN_MUL_LANES_PER_LAUNCH / (g == 1 ? 1 : 2);
    const BnGroupNttRun run = bn_group_ntt_run((unsigned)log_n, count, cap, shift != nullptr, inverse != 0);
    int rc;
    if (run.stages && (rc = bn_ntt_tables(c, log_n, inverse, shift, s))) return rc;
    if (run.ws_bufs && (rc = c->gntt_ws.reserve(run.most * V))) return rc;
    if (run.stages > 1 || run.pre || run.post)
        if ((rc = c->mul_tbl.reserve(bn254_mul_table_bytes_M(g, std::min(std::min(cap, chain_cap), run.most))))) return rc;
    if ((rc = c->norm_prefix.reserve(bn254_normalize_prefix_bytes_M(g, std::min(cap, run.most))))) return rc;
    const char *const wtbl = (const char *)c->ntt_tbl.p, *const stbl = wtbl + 2 * (size_t)GNTT_TBL * sizeof(bn_fr);
    bn_fr n_inv;
    bn_fr_inv_pow2((unsigned)log_n, &n_inv);
    const char *const scope[3] = {g == 1 ? "g1_ntt_scale" : "g2_ntt_scale", g == 1 ? "g1_ntt" : "g2_ntt", g == 1 ? "g1_ntt_normalize" : "g2_ntt_normalize"};
    return bn_for_parts(count, run.per_group, [&](size_t tr0, size_t cnt) -> int {
        char *const buf[3] = {(char *)d_in + tr0 * N * V, (char *)d_out + tr0 * N * V, (char *)c->gntt_ws.p};
        return bn_group_ntt_group(run, (unsigned)log_n, cnt, cap, chain_cap, [&](const BnGroupNttStep &st) -> int {
            BnScope sc(c, s, scope[st.kind]);
            if (st.kind == BN_GNTT_STAGE) return bn254_launch_group_ntt_stage_M(g, buf[st.src], buf[st.dst], wtbl, (unsigned)log_n, st.stage, inverse, st.lo, st.n, c->mul_tbl.p, s);
            if (st.kind == BN_GNTT_SCALE) return bn254_launch_group_ntt_scale_M(g, buf[st.src], buf[st.dst], stbl, (unsigned)log_n, shift ? nullptr : n_inv.l, st.lo, st.n, c->mul_tbl.p, s);
            return bn254_launch_normalize_M(g, buf[st.src] + st.lo * V, buf[st.dst] + st.lo * V, st.n, c->norm_prefix.p, s);
        });
    });
}

int gntt_dev(bn254_ctx *ctx, int g, const void *d_in, void *d_out, int log_n, size_t count, int inverse, const bn_fr *shift, void *stream) {
    if (count == 0) return BN254_OK;
    int rc = bn_group_ntt_check(d_in, d_out, log_n, count, shift); if (rc) return rc;      // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return gntt_run(ctx, g, d_in, d_out, log_n, count, inverse, shift, s); });
}
int gntt_host(bn254_ctx *ctx, int g, const void *in, void *out, int log_n, size_t count, int inverse, const bn_fr *shift) {
    if (count == 0) return BN254_OK;
    int rc = bn_group_ntt_check(in, out, log_n, count, shift); if (rc) return rc;          // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    const size_t bytes = (count << log_n) * (g == 1 ? sizeof(bn_g1) : sizeof(bn_g2));
    return bn_staged(ctx, {in, bytes}, {nullptr, 0}, out, bytes, nullptr, 0,
                     [&](const BnStaged &d) { return gntt_dev(ctx, g, d.in[0], d.out, log_n, count, inverse, shift, ctx->stream); });
}
}  // namespace

extern "C" {

int bn254_g1_ntt_batch_dev(bn254_ctx *c, const void *i, void *o, int log_n, size_t count, int inverse, const bn_fr *shift, void *s) { return gntt_dev(c, 1, i, o, log_n, count, inverse, shift, s); }
int bn254_g2_ntt_batch_dev(bn254_ctx *c, const void *i, void *o, int log_n, size_t count, int inverse, const bn_fr *shift, void *s) { return gntt_dev(c, 2, i, o, log_n, count, inverse, shift, s); }
int bn254_g1_ntt_batch(bn254_ctx *c, const bn_g1 *in, bn_g1 *out, int log_n, size_t count, int inverse, const bn_fr *shift) { return gntt_host(c, 1, in, out, log_n, count, inverse, shift); }
int bn254_g2_ntt_batch(bn254_ctx *c, const bn_g2 *in, bn_g2 *out, int log_n, size_t count, int inverse, const bn_fr *shift) { return gntt_host(c, 2, in, out, log_n, count, inverse, shift); }

// internal (not in the header; tests and tools/time_group_ntt.py): an override of the sub-launch size (0 restores BN_LAUNCH_MAX), so that a
// test reaches the seams between groups and sub-launches with a handful of butterflies
int bn254_group_ntt_set_launch_max(size_t units) { return g_gntt_launch_max.set(units); }

}  // extern "C"
