// Segmented scans over Fr on the device (include/bn254_hip.h bn254_fr_scan_batch and its _dev twin): the four kernels - instances of
// bn254_fr_decode_k<Op> like the other integer kernels, one piece of the work list per lane over the bodies of scan_ops.hpp -, the upload of
// the work list host_plan.hpp's bn_scan_plan builds from the offsets, the levels as sub-launches, and the two entry points.
#include <algorithm>
#include <atomic>
#include <cstring>

#include "scan_ops.hpp"
#include "host_ctx.hpp"

using namespace bn254;

static_assert(FR_SCAN_REVERSE == BN254_SCAN_REVERSE && FR_SCAN_EXCLUSIVE == BN254_SCAN_EXCLUSIVE && FR_SCAN_A_PER_SEGMENT == BN254_SCAN_A_PER_SEGMENT, "scan_ops.hpp mirrors the header's flags");

namespace {
constexpr unsigned SCAN_BLOCK = 256;

// one kernel per kind of level: the arrays of the call, the level's range of the work list, its lanes
template <BnScanKind K>
struct FrScanOp {
    FrScanArrays s; const BnScanPiece *list; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
        if (i >= n) return;
        if (K == BN_SCAN_REDUCE) fr_scan_reduce_body(s, list, i);
        else if (K == BN_SCAN_UP) fr_scan_up_body(s, list, i);
        else if (K == BN_SCAN_DOWN) fr_scan_down_body(s, list, i);
        else fr_scan_apply_body(s, list, i);
    }
};
template <class Op>
__global__ void __launch_bounds__(SCAN_BLOCK) bn254_fr_decode_k(Op op) { op(); }

template <BnScanKind K>
int scan_launch(const FrScanArrays &a, const BnScanPiece *list, size_t lanes, hipStream_t s) {
    hipLaunchKernelGGL(bn254_fr_decode_k<FrScanOp<K>>, dim3((unsigned)((lanes + SCAN_BLOCK - 1) / SCAN_BLOCK)), dim3(SCAN_BLOCK), 0, s, FrScanOp<K>{a, list, (uint32_t)lanes});
    return (int)hipGetLastError();
}

// tests and tools/time_scan.py only: the sub-launch size (0 = BN_LAUNCH_MAX) and the piece length the sweep times (0 = the shipped constant)
std::atomic<size_t> g_scan_launch_max;
std::atomic<unsigned> g_scan_piece;
size_t scan_step() { const size_t set = g_scan_launch_max.load(std::memory_order_relaxed); return set ? set : BN_LAUNCH_MAX; }
unsigned scan_piece() { const unsigned set = g_scan_piece.load(std::memory_order_relaxed); return set ? set : FR_SCAN_PIECE; }

// scratch guard held by the caller.  ONE copy of the work list per call through the context's pinned staging (shared with the segmented
// folds and the sparse linear maps), which is rewritten only after its previous copy completed - so `off` may be freed as soon as the call
// returns.  Then the levels in the plan's order, each as sub-launches of at most scan_step() lanes; the stream orders them.
int scan_run(bn254_ctx *c, const void *d_a, const void *d_b, const void *d_init, const size_t *off, size_t m, unsigned flags, void *d_out, hipStream_t s) {
    const BnScanPlan plan = bn_scan_plan(off, m, scan_piece(), FR_SCAN_FAN, (flags & BN254_SCAN_REVERSE) != 0);
    const size_t bytes = plan.pieces.size() * sizeof(BnScanPiece);
    int rc;
    if (c->seg_plan_ev) HIP_TRY(hipEventSynchronize(c->seg_plan_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->seg_plan_ev, hipEventDisableTiming));
    if ((rc = c->seg_plan_host.reserve(bytes)) || (rc = c->seg_plan.reserve(bytes)) || (rc = c->scan_ws.reserve(3 * plan.slots * sizeof(bn_fr)))) return rc;
    memcpy(c->seg_plan_host.p, plan.pieces.data(), bytes);
    HIP_TRY(hipMemcpyAsync(c->seg_plan.p, c->seg_plan_host.p, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->seg_plan_ev, s));
    const BnScanPiece *list = (const BnScanPiece *)c->seg_plan.p;
    uint32_t *const ws = (uint32_t *)c->scan_ws.p;
    const FrScanArrays arr = {(const uint32_t *)d_a, (const uint32_t *)d_b, (const uint32_t *)d_init, ws, ws + 8 * plan.slots, ws + 16 * plan.slots, (uint32_t *)d_out, flags};
    for (const BnScanLevel &lv : plan.levels) {
        rc = bn_for_parts(lv.count, scan_step(), [&](size_t lo, size_t cnt) -> int {
            const BnScanPiece *at = list + lv.first + lo;
            switch (lv.kind) {
            case BN_SCAN_REDUCE: { BnScope sc(c, s, "fr_scan_reduce"); return scan_launch<BN_SCAN_REDUCE>(arr, at, cnt, s); }
            case BN_SCAN_UP: { BnScope sc(c, s, "fr_scan_up"); return scan_launch<BN_SCAN_UP>(arr, at, cnt, s); }
            case BN_SCAN_DOWN: { BnScope sc(c, s, "fr_scan_down"); return scan_launch<BN_SCAN_DOWN>(arr, at, cnt, s); }
            default: { BnScope sc(c, s, "fr_scan"); return scan_launch<BN_SCAN_APPLY>(arr, at, cnt, s); }
            }
        });
        if (rc) return rc;
    }
    return BN254_OK;
}
}  // namespace

extern "C" {

// order of the checks: empty call, arguments (nothing of them touches a device; then a call without terms is done), then context and
// device; nothing waits, nothing is read back
int bn254_fr_scan_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_b, const void *d_init, const size_t *offsets, size_t m, unsigned int flags, void *d_out,
                            void *stream) {
    if (m == 0) return BN254_OK;
    int rc = bn_scan_check(d_a, d_b, offsets, m, flags, d_out); if (rc) return rc;                            // before any device lookup
    if (offsets[m] == 0) return BN254_OK;
    if ((rc = bn_get_ctx(ctx))) return rc;
    BnDev d(ctx, stream); if (!d.go) return d.rc;
    BnScratchGuard g(ctx, d.s); if (g.rc) return g.rc;
    return bn_no_throw([&] { return scan_run(ctx, d_a, d_b, d_init, offsets, m, flags, d_out, d.s); });
}
// three inputs, so the staging is spelled out: a and b in the two input buffers, init in the second output's, out in the first's
int bn254_fr_scan_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *b, const bn_fr *init, const size_t *offsets, size_t m, unsigned int flags, bn_fr *out) {
    if (m == 0) return BN254_OK;
    int rc = bn_scan_check(a, b, offsets, m, flags, out); if (rc) return rc;                                  // before any device lookup
    const size_t n = offsets[m];
    if (n == 0) return BN254_OK;
    BnHost h(ctx); if (h.rc) return h.rc;
    const hipStream_t s = ctx->stream;
    auto run = [&]() -> int {
        const void *src[3] = {a, b, init};
        const size_t bytes[3] = {a ? ((flags & BN254_SCAN_A_PER_SEGMENT) ? m : n) * sizeof(bn_fr) : 0, b ? n * sizeof(bn_fr) : 0, init ? m * sizeof(bn_fr) : 0};
        BnBuf *const buf[3] = {&ctx->stage[0], &ctx->stage[1], &ctx->stage[3]};
        int r;
        for (int i = 0; i < 3; ++i) {
            if ((r = buf[i]->reserve(bytes[i]))) return r;
            if (bytes[i]) HIP_TRY(hipMemcpyAsync(buf[i]->p, src[i], bytes[i], hipMemcpyHostToDevice, s));
        }
        if ((r = ctx->stage[2].reserve(n * sizeof(bn_fr)))) return r;
        if ((r = bn254_fr_scan_batch_dev(ctx, a ? ctx->stage[0].p : nullptr, b ? ctx->stage[1].p : nullptr, init ? ctx->stage[3].p : nullptr, offsets, m, flags, ctx->stage[2].p, s)))
            return r;
        HIP_TRY(hipMemcpyAsync(out, ctx->stage[2].p, n * sizeof(bn_fr), hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(s);          // copies that read or write the caller's buffers may still be in flight
    return rc;
}

// internal (not in the header; tests and tools/time_scan.py): the shipped piece length and fan, an override of the sub-launch size
// (0 restores BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of pieces, and - for the sweep only -
// a process-wide override of the piece length (0 restores the shipped one; same bytes whatever is set)
unsigned bn254_fr_scan_piece(void) { return FR_SCAN_PIECE; }
unsigned bn254_fr_scan_fan(void) { return FR_SCAN_FAN; }
int bn254_fr_scan_set_launch_max(size_t lanes) {
    if (lanes > BN_LAUNCH_MAX) return BN254_E_BAD_ARG;
    g_scan_launch_max.store(lanes, std::memory_order_relaxed);
    return BN254_OK;
}
int bn254_fr_scan_set_piece(unsigned P) {
    if (P > 64) return BN254_E_BAD_ARG;
    g_scan_piece.store(P, std::memory_order_relaxed);
    return BN254_OK;
}

}  // extern "C"
