// Segmented scans over Fr on the device (include/bn254_hip.h bn254_fr_scan_batch and its _dev twin): the four kernels - Ops of
// lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one piece of the work list per lane over the bodies of scan_ops.hpp -,
// the upload of the work list host_plan.hpp's bn_scan_plan builds from the offsets, the levels as sub-launches, and the two entry points.
#include <algorithm>

#include "scan_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

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
template <BnScanKind K>
int scan_launch(const FrScanArrays &a, const BnScanPiece *list, size_t lanes, hipStream_t s) {
    return bn_lane_launch<SCAN_BLOCK>(FrScanOp<K>{a, list, (uint32_t)lanes}, lanes, s);
}

// tests and tools/time_scan.py only: the sub-launch size and the piece length the sweep times
BnLaunchMax g_scan_launch_max;
BnOverride<unsigned> g_scan_piece;

// scratch guard held by the caller.  The work list goes up in one copy (bn_plan_upload: `off` may be freed as soon as the call returns).
// Then the levels in the plan's order, each as sub-launches of at most g_scan_launch_max.step() lanes; the stream orders them.
int scan_run(bn254_ctx *c, const void *d_a, const void *d_b, const void *d_init, const size_t *off, size_t m, unsigned flags, void *d_out, hipStream_t s) {
    const BnScanPlan plan = bn_scan_plan(off, m, g_scan_piece.get(FR_SCAN_PIECE), FR_SCAN_FAN, (flags & BN254_SCAN_REVERSE) != 0);
    int rc = c->scan_ws.reserve(3 * plan.slots * sizeof(bn_fr)); if (rc) return rc;
    if ((rc = bn_plan_upload(c, plan.pieces.data(), plan.pieces.size() * sizeof(BnScanPiece), nullptr, 0, s))) return rc;
    const BnScanPiece *list = (const BnScanPiece *)c->seg_plan.p;
    uint32_t *const ws = (uint32_t *)c->scan_ws.p;
    const FrScanArrays arr = {(const uint32_t *)d_a, (const uint32_t *)d_b, (const uint32_t *)d_init, ws, ws + 8 * plan.slots, ws + 16 * plan.slots, (uint32_t *)d_out, flags};
    for (const BnScanLevel &lv : plan.levels) {
        rc = bn_for_parts(lv.count, g_scan_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
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
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return scan_run(ctx, d_a, d_b, d_init, offsets, m, flags, d_out, s); });
}
int bn254_fr_scan_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *b, const bn_fr *init, const size_t *offsets, size_t m, unsigned int flags, bn_fr *out) {
    if (m == 0) return BN254_OK;
    int rc = bn_scan_check(a, b, offsets, m, flags, out); if (rc) return rc;                                  // before any device lookup
    const size_t n = offsets[m];
    if (n == 0) return BN254_OK;
    BnHost h(ctx); if (h.rc) return h.rc;               // a, b and - the third staged input, d.in[2] - init
    return bn_staged(ctx, {a, ((flags & BN254_SCAN_A_PER_SEGMENT) ? m : n) * sizeof(bn_fr)}, {b, n * sizeof(bn_fr)}, out, n * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_scan_batch_dev(ctx, d.in[0], d.in[1], d.in[2], offsets, m, flags, d.out, ctx->stream); },
                     {init, m * sizeof(bn_fr)});
}

// internal (not in the header; tests and tools/time_scan.py): the shipped piece length and fan, an override of the sub-launch size
// (0 restores BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of pieces, and - for the sweep only -
// a process-wide override of the piece length (0 restores the shipped one; same bytes whatever is set)
unsigned bn254_fr_scan_piece(void) { return FR_SCAN_PIECE; }
unsigned bn254_fr_scan_fan(void) { return FR_SCAN_FAN; }
int bn254_fr_scan_set_launch_max(size_t lanes) { return g_scan_launch_max.set(lanes); }
int bn254_fr_scan_set_piece(unsigned P) { return P > 64 ? BN254_E_BAD_ARG : g_scan_piece.set(P); }

}  // extern "C"
