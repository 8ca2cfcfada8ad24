// Grumpkin on the device (include/bn254_hip.h bn254_grumpkin_validate_batch, bn254_grumpkin_add_batch, bn254_grumpkin_mul_batch,
// bn254_grumpkin_msm_batch and their _dev twins): the kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one
// lane of a body of grumpkin_ops.hpp each - and the eight entry points.  validate / add / mul: a kind table and a launch switch on
// record_call.hpp's one path - one launch per call (and per sub-launch of a large one), no scratch, nothing waits.  The segmented sum: the work list of host_plan.hpp's bn_dot_plan with one term per lane goes up through
// the context's work-list staging, level 0 runs the chains, the fold levels add scratch slots of 96 bytes (ctx->grk_ws, under the scratch guard).
// Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>

#include "grumpkin_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"
#include "record_call.hpp"

using namespace bn254;

// lanes per workgroup, 64 or 512 (a measurement switch: UNITS=bn254_grumpkin tools/build_variant.sh grk_b512 -DBN254_GRUMPKIN_BLOCK=512).  The
// workgroup size is the only say the shell gives over the register budget: 512 lanes are two waves per SIMD, so at most 256 VGPRs
#ifndef BN254_GRUMPKIN_BLOCK
#define BN254_GRUMPKIN_BLOCK 64
#endif

namespace {
constexpr unsigned GRK_BLOCK = BN254_GRUMPKIN_BLOCK;
constexpr size_t GRK_SLOT_BYTES = 3 * sizeof(bn_fr);

// lanes [lo, lo + n) of a call: a sub-launch, one record per lane
struct GrkValidateOp {
    const uint32_t *p; int32_t *status; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * GRK_BLOCK + threadIdx.x;
        if (i < n) grk_validate_body(p, status, lo + i);
    }
};
struct GrkAddOp {
    const uint32_t *p, *q; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * GRK_BLOCK + threadIdx.x;
        if (i < n) grk_add_body(p, q, out, lo + i);
    }
};
struct GrkMulOp {
    const uint32_t *p, *k; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * GRK_BLOCK + threadIdx.x;
        if (i < n) grk_mul_body(p, k, out, lo + i);
    }
};
// pieces [0, n) of `list`: a sub-launch of one level of the segmented sum
struct GrkMsmOp {
    const uint32_t *p, *k; const BnDotPiece *list; uint32_t *part, *out; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * GRK_BLOCK + threadIdx.x;
        if (i < n) grk_msm_piece_body(p, k, list, part, out, i);
    }
};
struct GrkMsmFoldOp {
    const BnDotPiece *list; uint32_t *part, *out; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * GRK_BLOCK + threadIdx.x;
        if (i < n) grk_msm_fold_body(list, part, out, i);
    }
};

BnLaunchMax g_grk_launch_max;          // tests only: the sub-launch size

// validate / add / mul are a record family (record_call.hpp): scope, inputs and the bytes of one record of each, of the output, of a second output
enum { GRK_VALIDATE, GRK_ADD, GRK_MUL, GRK_KINDS };
constexpr BnRecordKind GRK_KIND[GRK_KINDS] = {{"grumpkin_validate", 1, {64}, sizeof(int32_t), 0}, {"grumpkin_add", 2, {64, 64}, 64, 0}, {"grumpkin_mul", 2, {64, 32}, 64, 0}};
struct GrkLaunch {
    int what;
    int operator()(const BnRecordArgs &a, size_t lo, size_t cnt, hipStream_t s) const {
        const uint32_t *const i0 = (const uint32_t *)a.in[0], *const i1 = (const uint32_t *)a.in[1];
        switch (what) {
        case GRK_VALIDATE: return bn_lane_launch<GRK_BLOCK>(GrkValidateOp{i0, (int32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        case GRK_ADD: return bn_lane_launch<GRK_BLOCK>(GrkAddOp{i0, i1, (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        default: return bn_lane_launch<GRK_BLOCK>(GrkMulOp{i0, i1, (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        }
    }
};
// the two forms of a call of kind `what`: checks, sub-launches, staging
int grk_host(bn254_ctx *ctx, int what, const BnRecordArgs &a, size_t n) { return bn_record_host(ctx, GRK_KIND[what], g_grk_launch_max, a, n, GrkLaunch{what}); }
int grk_dev(bn254_ctx *ctx, int what, const BnRecordArgs &a, size_t n, void *stream) { return bn_record_dev(ctx, GRK_KIND[what], g_grk_launch_max, a, n, stream, GrkLaunch{what}); }

// scratch guard held by the caller.  The work list goes up in one copy (bn_plan_upload: `off` may be freed as soon as the call returns).
// Then level 0 and the fold levels, each as sub-launches of at most g_grk_launch_max.step() pieces.
int grk_msm_run(bn254_ctx *c, const void *d_p, const void *d_k, const size_t *off, size_t m, void *d_out, hipStream_t s) {
    const BnDotPlan plan = bn_dot_plan(off, m, 1, GRK_MSM_FAN);
    int rc = c->grk_ws.reserve(plan.slots * GRK_SLOT_BYTES); if (rc) return rc;
    if ((rc = bn_plan_upload(c, plan.pieces.data(), plan.pieces.size() * sizeof(BnDotPiece), nullptr, 0, s))) return rc;
    const BnDotPiece *list = (const BnDotPiece *)c->seg_plan.p;
    uint32_t *const part = (uint32_t *)c->grk_ws.p, *const out = (uint32_t *)d_out;
    for (size_t l = 0; l < plan.levels.size(); ++l) {
        const BnDotLevel &lv = plan.levels[l];
        rc = bn_for_parts(lv.count, g_grk_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
            const BnDotPiece *at = list + lv.first + lo;
            BnScope sc(c, s, l ? "grumpkin_msm_fold" : "grumpkin_msm");
            if (l) return bn_lane_launch<GRK_BLOCK>(GrkMsmFoldOp{at, part, out, (uint32_t)cnt}, cnt, s);
            return bn_lane_launch<GRK_BLOCK>(GrkMsmOp{(const uint32_t *)d_p, (const uint32_t *)d_k, at, part, out, (uint32_t)cnt}, cnt, s);
        });
        if (rc) return rc;
    }
    return BN254_OK;
}
}  // namespace

extern "C" {

int bn254_grumpkin_validate_batch(bn254_ctx *ctx, const bn_fr *p, int32_t *status, size_t n) { return grk_host(ctx, GRK_VALIDATE, {{p}, status}, n); }
int bn254_grumpkin_add_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *q, bn_fr *out, size_t n) { return grk_host(ctx, GRK_ADD, {{p, q}, out}, n); }
int bn254_grumpkin_mul_batch(bn254_ctx *ctx, const bn_fr *p, const uint8_t *k32, bn_fr *out, size_t n) { return grk_host(ctx, GRK_MUL, {{p, k32}, out}, n); }
int bn254_grumpkin_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream) { return grk_dev(ctx, GRK_VALIDATE, {{d_p}, d_status}, n, stream); }
int bn254_grumpkin_add_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, void *d_out, size_t n, void *stream) { return grk_dev(ctx, GRK_ADD, {{d_p, d_q}, d_out}, n, stream); }
int bn254_grumpkin_mul_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k32, void *d_out, size_t n, void *stream) { return grk_dev(ctx, GRK_MUL, {{d_p, d_k32}, d_out}, n, stream); }

// order of the checks: empty call, arguments (nothing of them touches a device), then context and device; nothing waits, nothing is read back
int bn254_grumpkin_msm_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k32, const size_t *offsets, size_t m, void *d_out, void *stream) {
    if (m == 0) return BN254_OK;
    int rc = bn_seg_check(d_p, d_k32, offsets, m, d_out); if (rc) return rc;                 // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return grk_msm_run(ctx, d_p, d_k32, offsets, m, d_out, s); });
}
int bn254_grumpkin_msm_batch(bn254_ctx *ctx, const bn_fr *p, const uint8_t *k32, const size_t *offsets, size_t m, bn_fr *out) {
    if (m == 0) return BN254_OK;
    int rc = bn_seg_check(p, k32, offsets, m, out); if (rc) return rc;                       // before any device lookup
    const size_t n = offsets[m];
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_no_throw([&] {
        return bn_staged(ctx, {n ? p : nullptr, n * 64}, {n ? k32 : nullptr, n * 32}, out, m * 64, nullptr, 0,
                         [&](const BnStaged &d) { return bn254_grumpkin_msm_batch_dev(ctx, d.in[0], d.in[1], offsets, m, d.out, ctx->stream); });
    });
}

// internal (not in the header; tests and tools/time_grumpkin.py): an override of the sub-launch size of the calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records, and the window of [k]P
int bn254_grumpkin_set_launch_max(size_t lanes) { return g_grk_launch_max.set(lanes); }
int bn254_grumpkin_window(void) { return GRK_MUL_WINDOW; }

}  // extern "C"
