// Multilinear tables and sumcheck rounds over Fr on the device (include/bn254_hip.h bn254_fr_mle_eq, bn254_fr_mle_fold, bn254_fr_sumcheck_round,
// bn254_fr_sumcheck_fold_round, bn254_fr_mle_quotients and their _dev twins): the kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like
// the other integer kernels, one lane of the bodies of mle_ops.hpp each -, the levels host_plan.hpp's bn_sumcheck_plan and the passes its
// bn_mle_quotients_plan compute as sub-launches, and the ten entry points.
#include <algorithm>
#include <cstring>

#include "mle_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned MLE_BLOCK = 256;

// lanes [lo, lo + n) of a call: a sub-launch
struct FrMleEqOp {
    const uint32_t *z; uint32_t nv; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * MLE_BLOCK + threadIdx.x;
        if (i < n) fr_mle_eq_body(z, nv, out, lo + i);
    }
};
struct FrMleFoldOp {
    const uint32_t *in; Fr r; uint32_t *out; uint64_t half, lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * MLE_BLOCK + threadIdx.x;
        if (i < n) fr_mle_fold_body(in, r, out, half, lo + i);
    }
};
template <int D>
struct FrSumcheckRoundOp {
    const uint32_t *tables; uint64_t h; uint32_t k; BnSumcheckDesc desc; uint64_t lanes; uint32_t *dst; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * MLE_BLOCK + threadIdx.x;
        if (i < n) fr_sumcheck_round_body<D>(tables, h, k, desc, lanes, dst, lo + i);
    }
};
// the fused fold-then-round kernel: r by value like the fold's
template <int D>
struct FrSumcheckFoldRoundOp {
    const uint32_t *tables; Fr r; uint32_t *folded; uint64_t h2; uint32_t k; BnSumcheckDesc desc; uint64_t lanes; uint32_t *dst; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * MLE_BLOCK + threadIdx.x;
        if (i < n) fr_sumcheck_fold_round_body<D>(tables, r, folded, h2, k, desc, lanes, dst, lo + i);
    }
};
struct FrSumcheckSumOp {
    const uint32_t *src; uint64_t cnt; uint32_t F; uint32_t *dst; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * MLE_BLOCK + threadIdx.x;
        if (i < n) fr_sumcheck_sum_body(src, cnt, F, dst, lo + i);
    }
};
// a pass of RHO levels over the working table of 2^m records: zz[k] = z[m - 1 - k], by value like the fold's r
template <int RHO>
struct FrMleQuotOp {
    const uint32_t *src; Fr zz[RHO]; uint32_t m; uint32_t *fold_dst, *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * MLE_BLOCK + threadIdx.x;
        if (i < n) fr_mle_quotients_body<RHO>(src, zz, m, fold_dst, out, lo + i);
    }
};

// tests and tools/time_mle.py, tools/time_mle_open.py, tools/time_fold_round.py only: the sub-launch size, the piece lengths and the levels
// per quotient pass the sweeps time (for the fused call 0 = the adaptive choice)
BnLaunchMax g_mle_launch_max;
BnOverride<unsigned> g_sumcheck_piece, g_sumcheck_fold_piece, g_mle_quot_levels;
// an override holds at every size; otherwise the shipped piece, halved while the lanes do not fill a device of `cus` compute units
unsigned sumcheck_fold_piece(size_t h2, size_t cus) {
    return g_sumcheck_fold_piece.get((unsigned)bn_sumcheck_fold_piece(h2, FR_SUMCHECK_FOLD_PIECE, bn_sumcheck_fold_fill(cus)));
}

int eq_run(bn254_ctx *c, const void *d_z, int nv, void *d_out, hipStream_t s) {
    return bn_for_parts((size_t)1 << nv, g_mle_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, "fr_mle_eq");
        return bn_lane_launch<MLE_BLOCK>(FrMleEqOp{(const uint32_t *)d_z, (uint32_t)nv, (uint32_t *)d_out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
    });
}
int fold_run(bn254_ctx *c, const void *d_in, size_t len, const bn_fr *r, void *d_out, hipStream_t s) {
    Fr rr;
    memcpy(rr.w, r->l, sizeof rr.w);
    return bn_for_parts(len / 2, g_mle_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, "fr_mle_fold");
        return bn_lane_launch<MLE_BLOCK>(FrMleFoldOp{(const uint32_t *)d_in, rr, (uint32_t *)d_out, (uint64_t)(len / 2), (uint64_t)lo, (uint32_t)cnt}, cnt, s);
    });
}
template <int D>
int round_launch(const uint32_t *tables, size_t h, size_t k, const BnSumcheckDesc &desc, size_t lanes, uint32_t *dst, size_t lo, size_t cnt, hipStream_t s) {
    return bn_lane_launch<MLE_BLOCK>(FrSumcheckRoundOp<D>{tables, (uint64_t)h, (uint32_t)k, desc, (uint64_t)lanes, dst, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
}
// scratch guard held by the caller.  The lanes of `plan` through launch(dst, lo, cnt) under `scope` - the round kernel or the fused one -,
// then the sum levels in the plan's order, each as sub-launches of at most g_mle_launch_max.step() lanes; the stream orders them.
template <class Launch>
int levels_run(bn254_ctx *c, const BnSumcheckPlan &plan, const char *scope, void *d_out, hipStream_t s, Launch launch) {
    int rc = c->mle_ws.reserve(plan.slots * sizeof(bn_fr)); if (rc) return rc;
    uint32_t *const ws = (uint32_t *)c->mle_ws.p, *const out = (uint32_t *)d_out;
    rc = bn_for_parts(plan.lanes, g_mle_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, scope);
        return launch(plan.levels.empty() ? out : ws, lo, cnt);
    });
    if (rc) return rc;
    for (const BnSumcheckLevel &lv : plan.levels) {
        rc = bn_for_parts(lv.lanes, g_mle_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
            BnScope sc(c, s, "fr_sumcheck_sum");
            return bn_lane_launch<MLE_BLOCK>(FrSumcheckSumOp{ws + 8 * lv.src, (uint64_t)lv.cnt, FR_SUMCHECK_FAN, lv.to_out ? out : ws + 8 * lv.dst, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        });
        if (rc) return rc;
    }
    return BN254_OK;
}
int round_run(bn254_ctx *c, const void *d_tables, size_t n, size_t k, const BnSumcheckDesc &desc, int degree, void *d_out, hipStream_t s) {
    const size_t h = n / 2;
    const BnSumcheckPlan plan = bn_sumcheck_plan(h, (unsigned)degree, g_sumcheck_piece.get(FR_SUMCHECK_PIECE), FR_SUMCHECK_FAN);
    const uint32_t *tables = (const uint32_t *)d_tables;
    return levels_run(c, plan, "fr_sumcheck_round", d_out, s, [&](uint32_t *dst, size_t lo, size_t cnt) -> int {
        switch (degree) {
        case 1: return round_launch<1>(tables, h, k, desc, plan.lanes, dst, lo, cnt, s);
        case 2: return round_launch<2>(tables, h, k, desc, plan.lanes, dst, lo, cnt, s);
        case 3: return round_launch<3>(tables, h, k, desc, plan.lanes, dst, lo, cnt, s);
        default: return round_launch<4>(tables, h, k, desc, plan.lanes, dst, lo, cnt, s);
        }
    });
}
template <int D>
int fold_round_launch(const uint32_t *tables, const Fr &r, uint32_t *folded, size_t h2, size_t k, const BnSumcheckDesc &desc, size_t lanes, uint32_t *dst, size_t lo, size_t cnt,
                      hipStream_t s) {
    return bn_lane_launch<MLE_BLOCK>(FrSumcheckFoldRoundOp<D>{tables, r, folded, (uint64_t)h2, (uint32_t)k, desc, (uint64_t)lanes, dst, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
}
// scratch guard held by the caller.  The fused kernel over the n / 4 indices of the round that follows the fold, then the round's own sum levels.
int fold_round_run(bn254_ctx *c, const void *d_tables, size_t n, size_t k, const bn_fr *r, const BnSumcheckDesc &desc, int degree, void *d_folded, void *d_out, hipStream_t s) {
    const size_t h2 = n / 4;
    const BnSumcheckPlan plan = bn_sumcheck_plan(h2, (unsigned)degree, sumcheck_fold_piece(h2, (size_t)c->cus), FR_SUMCHECK_FAN);
    const uint32_t *tables = (const uint32_t *)d_tables;
    uint32_t *folded = (uint32_t *)d_folded;
    Fr rr;
    memcpy(rr.w, r->l, sizeof rr.w);
    return levels_run(c, plan, FR_SUMCHECK_FOLD_ROUND_SCOPE, d_out, s, [&](uint32_t *dst, size_t lo, size_t cnt) -> int {
        switch (degree) {
        case 1: return fold_round_launch<1>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt, s);
        case 2: return fold_round_launch<2>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt, s);
        case 3: return fold_round_launch<3>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt, s);
        default: return fold_round_launch<4>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt, s);
        }
    });
}
template <int RHO>
int quot_launch(const uint32_t *src, const bn_fr *z, unsigned m, uint32_t *fold_dst, uint32_t *out, size_t lo, size_t cnt, hipStream_t s) {
    FrMleQuotOp<RHO> op{src, {}, (uint32_t)m, fold_dst, out, (uint64_t)lo, (uint32_t)cnt};
    for (int k = 0; k < RHO; ++k) memcpy(op.zz[k].w, z[m - 1 - k].l, sizeof op.zz[k].w);
    return bn_lane_launch<MLE_BLOCK>(op, cnt, s);
}
// scratch guard held by the caller.  The passes in the plan's order, each as sub-launches of at most g_mle_launch_max.step() lanes; the stream orders
// them.  The first reads a and leaves the folded table in the scratch, the later ones run in place there; a is never written.
int quotients_run(bn254_ctx *c, const void *d_a, int nv, const bn_fr *z, void *d_out, hipStream_t s) {
    uint32_t *const out = (uint32_t *)d_out;
    if (nv == 0) return (int)hipMemcpyAsync(out, d_a, sizeof(bn_fr), hipMemcpyDeviceToDevice, s);
    const BnMleQuotPlan plan = bn_mle_quotients_plan((unsigned)nv, g_mle_quot_levels.get(FR_MLE_QUOT_LEVELS));
    int rc = c->mle_ws.reserve(plan.slots * sizeof(bn_fr)); if (rc) return rc;
    uint32_t *const ws = (uint32_t *)c->mle_ws.p;
    for (const BnMleQuotPass &ps : plan.passes) {
        const uint32_t *src = ps.first ? (const uint32_t *)d_a : ws;
        uint32_t *fold_dst = ps.last ? out : ws;
        rc = bn_for_parts(ps.lanes, g_mle_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
            BnScope sc(c, s, FR_MLE_QUOT_SCOPE);
            switch (ps.levels) {
            case 1: return quot_launch<1>(src, z, ps.vars, fold_dst, out, lo, cnt, s);
            case 2: return quot_launch<2>(src, z, ps.vars, fold_dst, out, lo, cnt, s);
            case 3: return quot_launch<3>(src, z, ps.vars, fold_dst, out, lo, cnt, s);
            default: return quot_launch<4>(src, z, ps.vars, fold_dst, out, lo, cnt, s);
            }
        });
        if (rc) return rc;
    }
    return BN254_OK;
}
}  // namespace

extern "C" {

// order of the checks everywhere: arguments (nothing of them touches a device), then context and device; nothing waits, nothing is read back
int bn254_fr_mle_eq_dev(bn254_ctx *ctx, const void *d_z, int nv, void *d_out, void *stream) {
    int rc = bn_mle_eq_check(d_z, nv, d_out); if (rc) return rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return eq_run(ctx, d_z, nv, d_out, s); });
}
int bn254_fr_mle_eq(bn254_ctx *ctx, const bn_fr *z, int nv, bn_fr *out) {
    int rc = bn_mle_eq_check(z, nv, out); if (rc) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {z, (size_t)nv * sizeof(bn_fr)}, {nullptr, 0}, out, sizeof(bn_fr) << nv, nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_mle_eq_dev(ctx, d.in[0], nv, d.out, ctx->stream); });
}
int bn254_fr_mle_fold_dev(bn254_ctx *ctx, const void *d_in, size_t len, const bn_fr *r, void *d_out, void *stream) {
    if (len == 0) return BN254_OK;
    int rc = bn_mle_fold_check(d_in, len, r, d_out); if (rc) return rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return fold_run(ctx, d_in, len, r, d_out, s); });
}
int bn254_fr_mle_fold(bn254_ctx *ctx, const bn_fr *in, size_t len, const bn_fr *r, bn_fr *out) {
    if (len == 0) return BN254_OK;
    int rc = bn_mle_fold_check(in, len, r, out); if (rc) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {in, len * sizeof(bn_fr)}, {nullptr, 0}, out, len / 2 * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_mle_fold_dev(ctx, d.in[0], len, r, d.out, ctx->stream); });
}
int bn254_fr_sumcheck_round_dev(bn254_ctx *ctx, const void *d_tables, size_t n, size_t k, const size_t *group_offsets, const uint64_t *group_tables, const bn_fr *group_coeff,
                                size_t g, int degree, void *d_out, void *stream) {
    BnSumcheckDesc desc;
    int rc = bn_sumcheck_check(d_tables, n, k, group_offsets, group_tables, group_coeff, g, degree, d_out, &desc); if (rc) return rc;      // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return round_run(ctx, d_tables, n, k, desc, degree, d_out, s); });
}
int bn254_fr_sumcheck_round(bn254_ctx *ctx, const bn_fr *tables, size_t n, size_t k, const size_t *group_offsets, const uint64_t *group_tables, const bn_fr *group_coeff, size_t g,
                            int degree, bn_fr *out) {
    BnSumcheckDesc desc;
    int rc = bn_sumcheck_check(tables, n, k, group_offsets, group_tables, group_coeff, g, degree, out, &desc); if (rc) return rc;          // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {tables, n * k * sizeof(bn_fr)}, {nullptr, 0}, out, (size_t)(degree + 1) * sizeof(bn_fr), nullptr, 0, [&](const BnStaged &d) {
        return bn254_fr_sumcheck_round_dev(ctx, d.in[0], n, k, group_offsets, group_tables, group_coeff, g, degree, d.out, ctx->stream);
    });
}
// r and the groups are HOST memory in both forms.  d_folded may be exactly d_tables: the kernel runs in place, the upper half is left as it was
int bn254_fr_sumcheck_fold_round_dev(bn254_ctx *ctx, const void *d_tables, size_t n, size_t k, const bn_fr *r, const size_t *group_offsets, const uint64_t *group_tables,
                                     const bn_fr *group_coeff, size_t g, int degree, void *d_folded, void *d_out, void *stream) {
    BnSumcheckDesc desc;
    int rc = bn_sumcheck_fold_check(d_tables, n, k, r, group_offsets, group_tables, group_coeff, g, degree, d_folded, d_out, &desc); if (rc) return rc;      // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return fold_round_run(ctx, d_tables, n, k, r, desc, degree, d_folded, d_out, s); });
}
// the staged copy is folded out of place on the device; with folded == tables only the lower half of the caller's array is written back
int bn254_fr_sumcheck_fold_round(bn254_ctx *ctx, const bn_fr *tables, size_t n, size_t k, const bn_fr *r, const size_t *group_offsets, const uint64_t *group_tables,
                                 const bn_fr *group_coeff, size_t g, int degree, bn_fr *folded, bn_fr *out) {
    BnSumcheckDesc desc;
    int rc = bn_sumcheck_fold_check(tables, n, k, r, group_offsets, group_tables, group_coeff, g, degree, folded, out, &desc); if (rc) return rc;            // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {tables, n * k * sizeof(bn_fr)}, {nullptr, 0}, folded, n / 2 * k * sizeof(bn_fr), out, (size_t)(degree + 1) * sizeof(bn_fr), [&](const BnStaged &d) {
        return bn254_fr_sumcheck_fold_round_dev(ctx, d.in[0], n, k, r, group_offsets, group_tables, group_coeff, g, degree, d.out, d.out2, ctx->stream);
    });
}
// z is HOST memory in both forms: its records travel as kernel arguments.  out must not overlap a.
int bn254_fr_mle_quotients_dev(bn254_ctx *ctx, const void *d_a, int nv, const bn_fr *z, void *d_out, void *stream) {
    int rc = bn_mle_quotients_check(d_a, nv, z, d_out); if (rc) return rc;
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return quotients_run(ctx, d_a, nv, z, d_out, s); });
}
int bn254_fr_mle_quotients(bn254_ctx *ctx, const bn_fr *a, int nv, const bn_fr *z, bn_fr *out) {
    int rc = bn_mle_quotients_check(a, nv, z, out); if (rc) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {a, sizeof(bn_fr) << nv}, {nullptr, 0}, out, sizeof(bn_fr) << nv, nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_mle_quotients_dev(ctx, d.in[0], nv, z, d.out, ctx->stream); });
}

// internal (not in the header; tests and tools/time_mle.py): the shipped piece length and fan of the round, an override of the sub-launch
// size of all three calls (0 restores BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of lanes, and
// - for the sweep only - a process-wide override of the piece length (0 restores the shipped one; same bytes whatever is set)
unsigned bn254_fr_sumcheck_piece(void) { return FR_SUMCHECK_PIECE; }
unsigned bn254_fr_sumcheck_fan(void) { return FR_SUMCHECK_FAN; }
int bn254_fr_mle_set_launch_max(size_t lanes) { return g_mle_launch_max.set(lanes); }
// the shipped levels per quotient pass and - for the sweep of tools/time_mle_open.py only - a process-wide override (0 restores the shipped
// one; same bytes whatever is set)
unsigned bn254_fr_mle_quotients_levels(void) { return FR_MLE_QUOT_LEVELS; }
int bn254_fr_mle_quotients_set_levels(unsigned rho) { return rho > FR_MLE_QUOT_LEVELS_MAX ? BN254_E_BAD_ARG : g_mle_quot_levels.set(rho); }
int bn254_fr_sumcheck_set_piece(unsigned P) { return P > 64 ? BN254_E_BAD_ARG : g_sumcheck_piece.set(P); }
// the shipped piece length of the fused fold-then-round kernel, a process-wide override of it for the sweep of tools/time_fold_round.py and
// the tests (0 restores the adaptive choice; same bytes whatever is set), and the piece a call over h2 indices runs with on `cus` compute units
unsigned bn254_fr_sumcheck_fold_piece(void) { return FR_SUMCHECK_FOLD_PIECE; }
int bn254_fr_sumcheck_fold_set_piece(unsigned P) { return P > 64 ? BN254_E_BAD_ARG : g_sumcheck_fold_piece.set(P); }
unsigned bn254_fr_sumcheck_fold_piece_for(size_t h2, size_t cus) { return sumcheck_fold_piece(h2, cus); }

}  // extern "C"
