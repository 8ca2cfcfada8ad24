// Sparse linear maps over Fr on the device (include/bn254_hip.h bn254_fr_dot_batch and its _dev twin): the two kernels - instances of
// bn254_fr_decode_k<Op> like the other integer kernels, one piece of the work list per lane over the bodies of dot_ops.hpp -, the upload of
// the work list host_plan.hpp's bn_dot_plan builds from the offsets, the levels as sub-launches, and the two entry points.
#include <algorithm>
#include <atomic>
#include <cstring>

#include "dot_ops.hpp"
#include "host_ctx.hpp"

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
template <class Op>
__global__ void __launch_bounds__(DOT_BLOCK) bn254_fr_decode_k(Op op) { op(); }

template <class Op>
int dot_launch(const Op &op, size_t lanes, hipStream_t s) {
    hipLaunchKernelGGL(bn254_fr_decode_k<Op>, dim3((unsigned)((lanes + DOT_BLOCK - 1) / DOT_BLOCK)), dim3(DOT_BLOCK), 0, s, op);
    return (int)hipGetLastError();
}

// tests and tools/time_dot.py only: the sub-launch size (0 = BN_LAUNCH_MAX) and the piece length the sweep times (0 = the shipped constant)
std::atomic<size_t> g_dot_launch_max;
std::atomic<unsigned> g_dot_piece;
size_t dot_step() { const size_t set = g_dot_launch_max.load(std::memory_order_relaxed); return set ? set : BN_LAUNCH_MAX; }
unsigned dot_piece() { const unsigned set = g_dot_piece.load(std::memory_order_relaxed); return set ? set : FR_DOT_PIECE; }

// scratch guard held by the caller.  ONE copy of the work list per call through the context's pinned staging (shared with the segmented
// folds), which is rewritten only after its previous copy completed - so `off` may be freed as soon as the call returns.  Then the product
// level and the fold levels, each as sub-launches of at most dot_step() pieces.
int dot_run(bn254_ctx *c, const void *d_coeff, const void *d_index, const void *d_x, size_t nx, const size_t *off, size_t m, void *d_out, hipStream_t s) {
    const BnDotPlan plan = bn_dot_plan(off, m, dot_piece(), FR_DOT_FAN);
    const size_t bytes = plan.pieces.size() * sizeof(BnDotPiece);
    int rc;
    if (c->seg_plan_ev) HIP_TRY(hipEventSynchronize(c->seg_plan_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->seg_plan_ev, hipEventDisableTiming));
    if ((rc = c->seg_plan_host.reserve(bytes)) || (rc = c->seg_plan.reserve(bytes)) || (rc = c->dot_ws.reserve(plan.slots * sizeof(bn_fr)))) return rc;
    memcpy(c->seg_plan_host.p, plan.pieces.data(), bytes);
    HIP_TRY(hipMemcpyAsync(c->seg_plan.p, c->seg_plan_host.p, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->seg_plan_ev, s));
    const BnDotPiece *list = (const BnDotPiece *)c->seg_plan.p;
    uint32_t *const part = (uint32_t *)c->dot_ws.p, *const out = (uint32_t *)d_out;
    for (size_t l = 0; l < plan.levels.size(); ++l) {
        const BnDotLevel &lv = plan.levels[l];
        rc = bn_for_parts(lv.count, dot_step(), [&](size_t lo, size_t cnt) -> int {
            const BnDotPiece *at = list + lv.first + lo;
            BnScope sc(c, s, l ? "fr_dot_fold" : "fr_dot");
            if (l) return dot_launch(FrDotFoldOp{at, part, out, (uint32_t)cnt}, cnt, s);
            return dot_launch(FrDotOp{(const uint32_t *)d_coeff, (const uint64_t *)d_index, (const uint32_t *)d_x, (uint64_t)nx, at, part, out, (uint32_t)cnt}, cnt, s);
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
    if ((rc = bn_get_ctx(ctx))) return rc;
    BnDev d(ctx, stream); if (!d.go) return d.rc;
    BnScratchGuard g(ctx, d.s); if (g.rc) return g.rc;
    return bn_no_throw([&] { return dot_run(ctx, d_coeff, d_index, d_x, nx, offsets, m, d_out, d.s); });
}
// three inputs, so the staging is spelled out: coeff and x in the two input buffers, index in the second output's, out in the first's
int bn254_fr_dot_batch(bn254_ctx *ctx, const bn_fr *coeff, const uint64_t *index, const bn_fr *x, size_t nx, const size_t *offsets, size_t m, bn_fr *out) {
    if (m == 0) return BN254_OK;
    int rc = bn_dot_check(coeff, index != nullptr, x, nx, offsets, m, out); if (rc) return rc;               // before any device lookup
    const size_t n = offsets[m];
    if ((rc = bn_dot_check_index(index, n, nx))) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    const hipStream_t s = ctx->stream;
    auto run = [&]() -> int {
        const void *src[3] = {coeff, x, index};
        const size_t bytes[3] = {n * sizeof(bn_fr), n ? nx * sizeof(bn_fr) : 0, index ? n * sizeof(uint64_t) : 0};
        BnBuf *const buf[3] = {&ctx->stage[0], &ctx->stage[1], &ctx->stage[3]};
        int r;
        for (int i = 0; i < 3; ++i) {
            if ((r = buf[i]->reserve(bytes[i]))) return r;
            if (bytes[i]) HIP_TRY(hipMemcpyAsync(buf[i]->p, src[i], bytes[i], hipMemcpyHostToDevice, s));
        }
        if ((r = ctx->stage[2].reserve(m * sizeof(bn_fr)))) return r;
        if ((r = bn254_fr_dot_batch_dev(ctx, ctx->stage[0].p, index ? ctx->stage[3].p : nullptr, ctx->stage[1].p, nx, offsets, m, ctx->stage[2].p, s))) return r;
        HIP_TRY(hipMemcpyAsync(out, ctx->stage[2].p, m * sizeof(bn_fr), hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(s);          // copies that read or write the caller's buffers may still be in flight
    return rc;
}

// internal (not in the header; tests and tools/time_dot.py): the shipped piece length and fan of the fold, an override of the sub-launch
// size (0 restores BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of pieces, and - for the sweep
// only - a process-wide override of the piece length (0 restores the shipped one; same bytes whatever is set)
unsigned bn254_fr_dot_piece(void) { return FR_DOT_PIECE; }
unsigned bn254_fr_dot_fan(void) { return FR_DOT_FAN; }
int bn254_fr_dot_set_launch_max(size_t pieces) {
    if (pieces > BN_LAUNCH_MAX) return BN254_E_BAD_ARG;
    g_dot_launch_max.store(pieces, std::memory_order_relaxed);
    return BN254_OK;
}
int bn254_fr_dot_set_piece(unsigned P) {
    if (P > 64) return BN254_E_BAD_ARG;
    g_dot_piece.store(P, std::memory_order_relaxed);
    return BN254_OK;
}

}  // extern "C"
