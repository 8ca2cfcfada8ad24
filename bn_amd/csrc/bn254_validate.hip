// Validation of raw points on the device (include/bn254_hip.h bn254_g1_validate_batch, bn254_g2_validate_batch and their _dev twins): the
// kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one lane of a body of subgroup_ops.hpp each -, the
// family's kind table and launch switch, and the four entry points on record_call.hpp's one path.  One launch per call (and per sub-launch of a large one): a lane compares its record's words with q, checks the curve
// equation and - G2 - runs the endomorphism subgroup test, so the _dev calls use no scratch and wait on nothing.
// Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>

#include "subgroup_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"
#include "record_call.hpp"

using namespace bn254;

namespace {
constexpr unsigned VAL_BLOCK = 64;

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

enum { VAL_G1, VAL_G2, VAL_KINDS };
constexpr BnRecordKind VAL_KIND[VAL_KINDS] = {{"g1_validate", 1, {sizeof(bn_g1)}, sizeof(int32_t), 0}, {"g2_validate", 1, {sizeof(bn_g2)}, sizeof(int32_t), 0}};
struct ValidateLaunch {
    int what;
    int operator()(const BnRecordArgs &a, size_t lo, size_t cnt, hipStream_t s) const {
        if (what == VAL_G1) return bn_lane_launch<VAL_BLOCK>(G1ValidateOp{(const uint32_t *)a.in[0], (int32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        return bn_lane_launch<VAL_BLOCK>(G2ValidateOp{(const uint32_t *)a.in[0], (int32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
    }
};
// the two forms of a call of kind `what` (record_call.hpp): checks, sub-launches, staging
int validate_host(bn254_ctx *ctx, int what, const BnRecordArgs &a, size_t n) { return bn_record_host(ctx, VAL_KIND[what], g_validate_launch_max, a, n, ValidateLaunch{what}); }
int validate_dev(bn254_ctx *ctx, int what, const BnRecordArgs &a, size_t n, void *stream) { return bn_record_dev(ctx, VAL_KIND[what], g_validate_launch_max, a, n, stream, ValidateLaunch{what}); }
}  // namespace

extern "C" {

int bn254_g1_validate_batch(bn254_ctx *ctx, const bn_g1 *p, int32_t *status, size_t n) { return validate_host(ctx, VAL_G1, {{p}, status}, n); }
int bn254_g2_validate_batch(bn254_ctx *ctx, const bn_g2 *p, int32_t *status, size_t n) { return validate_host(ctx, VAL_G2, {{p}, status}, n); }
int bn254_g1_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream) { return validate_dev(ctx, VAL_G1, {{d_p}, d_status}, n, stream); }
int bn254_g2_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream) { return validate_dev(ctx, VAL_G2, {{d_p}, d_status}, n, stream); }

// internal (not in the header; tests and tools/time_validate.py): an override of the sub-launch size of the four calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records
int bn254_validate_set_launch_max(size_t lanes) { return g_validate_launch_max.set(lanes); }

}  // extern "C"
