// Hash to G2 and cofactor clearing on the device (include/bn254_hip.h bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch,
// bn254_g2_hash_to_curve_uniform_batch, bn254_g2_hash_to_curve_batch and their _dev twins): the kernels - Ops of lane_launch.hpp's
// bn254_fr_decode_k like the other integer kernels, one lane of a body of hash_g2_ops.hpp each - and the eight entry points.  One launch per
// call (and per sub-launch of a large one): a lane reduces its field elements, runs both maps, adds, clears the cofactor and normalises, so the
// _dev calls use no scratch and wait on nothing.  Neither the constants nor the outputs are checked against gnark-crypto or any other library.
// Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>
#include <cstring>

#include "hash_g2_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned H2C_BLOCK = 64;
constexpr size_t H2C_N_MAX = (size_t)1 << 40, H2C_MSG_MAX = (size_t)1 << 20;

// lanes [lo, lo + n) of a call: a sub-launch, one record per lane
struct G2MapToCurveOp {
    const uint8_t *u; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * H2C_BLOCK + threadIdx.x;
        if (i < n) h2c_g2_map_body(u, out, lo + i);
    }
};
struct G2ClearCofactorOp {
    const uint32_t *p; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * H2C_BLOCK + threadIdx.x;
        if (i < n) h2c_g2_clear_body(p, out, lo + i);
    }
};
struct G2HashUniformOp {
    const uint8_t *uniform; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * H2C_BLOCK + threadIdx.x;
        if (i < n) h2c_g2_hash_uniform_body(uniform, out, lo + i);
    }
};
// the tag travels in the argument record: DST || len(DST), the same for every lane
struct G2HashMsgOp {
    const uint8_t *msgs; uint64_t msg_len; uint32_t *out; uint64_t lo; uint32_t n; uint32_t dst_prime_len; uint8_t dst_prime[H2C_DST_MAX + 1];
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * H2C_BLOCK + threadIdx.x;
        if (i < n) h2c_g2_hash_msg_body(msgs, (size_t)msg_len, dst_prime, dst_prime_len, out, lo + i);
    }
};

BnLaunchMax g_hash_g2_launch_max;      // tests only: the sub-launch size

enum { H2C_MAP = 0, H2C_UNIFORM = 1, H2C_MSG = 2, H2C_CLEAR = 3 };
// arguments only: nothing here touches a device.  1 = nothing to do
int hash_check(int which, const void *in, size_t msg_len, const void *dst, size_t dst_len, const void *out, size_t n) {
    if (which == H2C_MSG && (dst_len == 0 || dst_len > BN254_H2C_DST_MAX || msg_len > H2C_MSG_MAX)) return BN254_E_BAD_ARG;
    if (n == 0) return 1;
    if (n > H2C_N_MAX || (which == H2C_MSG && n * msg_len > H2C_N_MAX)) return BN254_E_BAD_ARG;        // (no overflow: both factors were bounded above)
    if (!out || (which == H2C_MSG && !dst) || (!in && !(which == H2C_MSG && msg_len == 0))) return BN254_E_BAD_ARG;
    return BN254_OK;
}
const char *hash_scope(int which) {
    return which == H2C_MAP ? "g2_map_to_curve" : which == H2C_CLEAR ? "g2_clear_cofactor" : which == H2C_UNIFORM ? "g2_hash_to_curve" : "g2_hash_to_curve_msg";
}
int hash_run(bn254_ctx *ctx, int which, const void *d_in, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out, size_t n, hipStream_t s) {
    G2HashMsgOp m = {};
    if (which == H2C_MSG) {
        m.msgs = (const uint8_t *)d_in; m.msg_len = msg_len; m.out = (uint32_t *)d_out; m.dst_prime_len = (uint32_t)dst_len + 1;
        memcpy(m.dst_prime, dst, dst_len);
        m.dst_prime[dst_len] = (uint8_t)dst_len;
    }
    return bn_for_parts(n, g_hash_g2_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(ctx, s, hash_scope(which));
        if (which == H2C_MAP) return bn_lane_launch<H2C_BLOCK>(G2MapToCurveOp{(const uint8_t *)d_in, (uint32_t *)d_out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        if (which == H2C_CLEAR) return bn_lane_launch<H2C_BLOCK>(G2ClearCofactorOp{(const uint32_t *)d_in, (uint32_t *)d_out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        if (which == H2C_UNIFORM) return bn_lane_launch<H2C_BLOCK>(G2HashUniformOp{(const uint8_t *)d_in, (uint32_t *)d_out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        m.lo = lo; m.n = (uint32_t)cnt;
        return bn_lane_launch<H2C_BLOCK>(m, cnt, s);
    });
}
// order of the checks: arguments, then context and device; nothing waits, nothing is read back
int hash_dev(bn254_ctx *ctx, int which, const void *d_in, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out, size_t n, void *stream) {
    int rc = hash_check(which, d_in, msg_len, dst, dst_len, d_out, n); if (rc) return rc == 1 ? BN254_OK : rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return hash_run(ctx, which, d_in, msg_len, dst, dst_len, d_out, n, s); });
}
int hash_host(bn254_ctx *ctx, int which, const void *in, size_t msg_len, const uint8_t *dst, size_t dst_len, bn_g2 *out, size_t n) {
    int rc = hash_check(which, in, msg_len, dst, dst_len, out, n); if (rc) return rc == 1 ? BN254_OK : rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    const size_t rec = which == H2C_MAP ? BN254_H2C_G2_FIELD_BYTES : which == H2C_UNIFORM ? BN254_H2C_G2_UNIFORM_BYTES : which == H2C_CLEAR ? sizeof(bn_g2) : msg_len;
    return bn_staged(ctx, {rec ? in : nullptr, n * rec}, {nullptr, 0}, out, n * sizeof(bn_g2), nullptr, 0,
                     [&](const BnStaged &d) { return hash_run(ctx, which, d.in[0], msg_len, dst, dst_len, d.out, n, ctx->stream); });
}
}  // namespace

extern "C" {

int bn254_g2_map_to_curve_batch(bn254_ctx *ctx, const uint8_t *u, bn_g2 *out, size_t n) { return hash_host(ctx, H2C_MAP, u, 0, nullptr, 0, out, n); }
int bn254_g2_clear_cofactor_batch(bn254_ctx *ctx, const bn_g2 *p, bn_g2 *out, size_t n) { return hash_host(ctx, H2C_CLEAR, p, 0, nullptr, 0, out, n); }
int bn254_g2_hash_to_curve_uniform_batch(bn254_ctx *ctx, const uint8_t *uniform, bn_g2 *out, size_t n) { return hash_host(ctx, H2C_UNIFORM, uniform, 0, nullptr, 0, out, n); }
int bn254_g2_hash_to_curve_batch(bn254_ctx *ctx, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, bn_g2 *out, size_t n) {
    return hash_host(ctx, H2C_MSG, msgs, msg_len, dst, dst_len, out, n);
}
int bn254_g2_map_to_curve_batch_dev(bn254_ctx *ctx, const void *d_u, void *d_out, size_t n, void *stream) { return hash_dev(ctx, H2C_MAP, d_u, 0, nullptr, 0, d_out, n, stream); }
int bn254_g2_clear_cofactor_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_out, size_t n, void *stream) { return hash_dev(ctx, H2C_CLEAR, d_p, 0, nullptr, 0, d_out, n, stream); }
int bn254_g2_hash_to_curve_uniform_batch_dev(bn254_ctx *ctx, const void *d_uniform, void *d_out, size_t n, void *stream) {
    return hash_dev(ctx, H2C_UNIFORM, d_uniform, 0, nullptr, 0, d_out, n, stream);
}
int bn254_g2_hash_to_curve_batch_dev(bn254_ctx *ctx, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out, size_t n, void *stream) {
    return hash_dev(ctx, H2C_MSG, d_msgs, msg_len, dst, dst_len, d_out, n, stream);
}

// internal (not in the header; tests and tools/time_hash_g2.py): an override of the sub-launch size of the eight calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records
int bn254_hash_g2_set_launch_max(size_t lanes) { return g_hash_g2_launch_max.set(lanes); }

}  // extern "C"
