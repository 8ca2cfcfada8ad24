// Sparse linear maps over Fr on the device (include/bn254_hip.h bn254_fr_dot_batch and its _dev twin): the two kernels - Ops of
// lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one piece of the work list per lane over the bodies of dot_ops.hpp -,
// the upload of the work list host_plan.hpp's bn_dot_plan builds from the offsets, the levels as sub-launches, and the two entry points.
#include <algorithm>

#include "dot_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned DOT_BLOCK = 256;

struct FrDotOp {
    const uint32_t *coeff; const uint64_t *index; const uint32_t *x; uint64_t nx; const BnDotPiece *list; uint32_t *part, *out; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * DOT_BLOCK + threadIdx.x;
        if (i < n) fr_dot_piece_body(coeff, index, x, nx, list, part, out, i);
    }
};
struct FrDotFoldOp {
    const BnDotPiece *list; uint32_t *part, *out; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * DOT_BLOCK + threadIdx.x;
        if (i < n) fr_dot_fold_body(list, part, out, i);
    }
};
// tests and tools/time_dot.py only: the sub-launch size and the piece length the sweep times
BnLaunchMax g_dot_launch_max;
BnOverride<unsigned> g_dot_piece;

// scratch guard held by the caller.  The work list goes up in one copy (bn_plan_upload: `off` may be freed as soon as the call returns).
// Then the product level and the fold levels, each as sub-launches of at most g_dot_launch_max.step() pieces.
int dot_run(bn254_ctx *c, const void *d_coeff, const void *d_index, const void *d_x, size_t nx, const size_t *off, size_t m, void *d_out, hipStream_t s) {
    const BnDotPlan plan = bn_dot_plan(off, m, g_dot_piece.get(FR_DOT_PIECE), FR_DOT_FAN);
    int rc = c->dot_ws.reserve(plan.slots * sizeof(bn_fr)); if (rc) return rc;
    if ((rc = bn_plan_upload(c, plan.pieces.data(), plan.pieces.size() * sizeof(BnDotPiece), nullptr, 0, s))) return rc;
    const BnDotPiece *list = (const BnDotPiece *)c->seg_plan.p;
    uint32_t *const part = (uint32_t *)c->dot_ws.p, *const out = (uint32_t *)d_out;
    for (size_t l = 0; l < plan.levels.size(); ++l) {
        const BnDotLevel &lv = plan.levels[l];
        rc = bn_for_parts(lv.count, g_dot_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
            const BnDotPiece *at = list + lv.first + lo;
            BnScope sc(c, s, l ? "fr_dot_fold" : "fr_dot");
            if (l) return bn_lane_launch<DOT_BLOCK>(FrDotFoldOp{at, part, out, (uint32_t)cnt}, cnt, s);
            return bn_lane_launch<DOT_BLOCK>(FrDotOp{(const uint32_t *)d_coeff, (const uint64_t *)d_index, (const uint32_t *)d_x, (uint64_t)nx, at, part, out, (uint32_t)cnt}, cnt, s);
        });
        if (rc) return rc;
    }
    return BN254_OK;
}
}  // namespace

extern "C" {

// order of the checks: empty call, arguments (nothing of them touches a device), then context and device; nothing waits, nothing is read back
int bn254_fr_dot_batch_dev(bn254_ctx *ctx, const void *d_coeff, const void *d_index, const void *d_x, size_t nx, const size_t *offsets, size_t m, void *d_out,
                           void *stream) {
    if (m == 0) return BN254_OK;
    int rc = bn_dot_check(d_coeff, d_index != nullptr, d_x, nx, offsets, m, d_out); if (rc) return rc;       // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return dot_run(ctx, d_coeff, d_index, d_x, nx, offsets, m, d_out, s); });
}
int bn254_fr_dot_batch(bn254_ctx *ctx, const bn_fr *coeff, const uint64_t *index, const bn_fr *x, size_t nx, const size_t *offsets, size_t m, bn_fr *out) {
    if (m == 0) return BN254_OK;
    int rc = bn_dot_check(coeff, index != nullptr, x, nx, offsets, m, out); if (rc) return rc;               // before any device lookup
    const size_t n = offsets[m];
    if ((rc = bn_dot_check_index(index, n, nx))) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;               // coeff, x and - the third staged input, d.in[2] - index
    return bn_staged(ctx, {coeff, n * sizeof(bn_fr)}, {x, n ? nx * sizeof(bn_fr) : 0}, out, m * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_dot_batch_dev(ctx, d.in[0], d.in[2], d.in[1], nx, offsets, m, d.out, ctx->stream); },
                     {index, n * sizeof(uint64_t)});
}

// internal (not in the header; tests and tools/time_dot.py): the shipped piece length and fan of the fold, an override of the sub-launch
// size (0 restores BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of pieces, and - for the sweep
// only - a process-wide override of the piece length (0 restores the shipped one; same bytes whatever is set)
unsigned bn254_fr_dot_piece(void) { return FR_DOT_PIECE; }
unsigned bn254_fr_dot_fan(void) { return FR_DOT_FAN; }
int bn254_fr_dot_set_launch_max(size_t pieces) { return g_dot_launch_max.set(pieces); }
int bn254_fr_dot_set_piece(unsigned P) { return P > 64 ? BN254_E_BAD_ARG : g_dot_piece.set(P); }

}  // extern "C"
