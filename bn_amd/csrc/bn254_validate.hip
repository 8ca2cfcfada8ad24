// Validation of raw points on the device (include/bn254_hip.h bn254_g1_validate_batch, bn254_g2_validate_batch and their _dev twins): the
// kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one lane of a body of subgroup_ops.hpp each - and the
// four entry points.  One launch per call (and per sub-launch of a large one): a lane compares its record's words with q, checks the curve
// equation and - G2 - runs the endomorphism subgroup test, so the _dev calls use no scratch and wait on nothing.
// Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>

#include "subgroup_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned VAL_BLOCK = 64;
constexpr size_t VAL_N_MAX = (size_t)1 << 40;

// lanes [lo, lo + n) of a call: a sub-launch, one record per lane
struct G1ValidateOp {
    const uint32_t *p; int32_t *status; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * VAL_BLOCK + threadIdx.x;
        if (i < n) g1_validate_body(p, status, lo + i);
    }
};
struct G2ValidateOp {
    const uint32_t *p; int32_t *status; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * VAL_BLOCK + threadIdx.x;
        if (i < n) g2_validate_body(p, status, lo + i);
    }
};

BnLaunchMax g_validate_launch_max;     // tests only: the sub-launch size

// arguments only: nothing here touches a device.  1 = nothing to do
int validate_check(const void *p, const void *status, size_t n) {
    if (n == 0) return 1;
    return (!p || !status || n > VAL_N_MAX) ? BN254_E_BAD_ARG : BN254_OK;
}
int validate_run(bn254_ctx *ctx, int g, const void *d_p, void *d_status, size_t n, hipStream_t s) {
    return bn_for_parts(n, g_validate_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(ctx, s, g == 1 ? "g1_validate" : "g2_validate");
        if (g == 1) return bn_lane_launch<VAL_BLOCK>(G1ValidateOp{(const uint32_t *)d_p, (int32_t *)d_status, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        return bn_lane_launch<VAL_BLOCK>(G2ValidateOp{(const uint32_t *)d_p, (int32_t *)d_status, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
    });
}
// order of the checks: arguments, then context and device; nothing waits, nothing is read back
int validate_dev(bn254_ctx *ctx, int g, const void *d_p, void *d_status, size_t n, void *stream) {
    int rc = validate_check(d_p, d_status, n); if (rc) return rc == 1 ? BN254_OK : rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return validate_run(ctx, g, d_p, d_status, n, s); });
}
int validate_host(bn254_ctx *ctx, int g, const void *p, int32_t *status, size_t n) {
    int rc = validate_check(p, status, n); if (rc) return rc == 1 ? BN254_OK : rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {p, n * (g == 1 ? sizeof(bn_g1) : sizeof(bn_g2))}, {nullptr, 0}, status, n * sizeof(int32_t), nullptr, 0,
                     [&](const BnStaged &d) { return validate_run(ctx, g, d.in[0], d.out, n, ctx->stream); });
}
}  // namespace

extern "C" {

int bn254_g1_validate_batch(bn254_ctx *ctx, const bn_g1 *p, int32_t *status, size_t n) { return validate_host(ctx, 1, p, status, n); }
int bn254_g2_validate_batch(bn254_ctx *ctx, const bn_g2 *p, int32_t *status, size_t n) { return validate_host(ctx, 2, p, status, n); }
int bn254_g1_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream) { return validate_dev(ctx, 1, d_p, d_status, n, stream); }
int bn254_g2_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream) { return validate_dev(ctx, 2, d_p, d_status, n, stream); }

// internal (not in the header; tests and tools/time_validate.py): an override of the sub-launch size of the four calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records
int bn254_validate_set_launch_max(size_t lanes) { return g_validate_launch_max.set(lanes); }

}  // extern "C"
