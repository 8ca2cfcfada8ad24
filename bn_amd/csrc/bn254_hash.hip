// Hash to G1 on the device (include/bn254_hip.h bn254_g1_map_to_curve_batch, bn254_g1_hash_to_curve_uniform_batch, bn254_g1_hash_to_curve_batch
// and their _dev twins): the kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one lane of a body of
// hash_ops.hpp each -, the family's kind table and launch switch, and the six entry points on record_call.hpp's one path.  One launch per call
// (and per sub-launch of a large one): a lane reduces its field elements, runs both maps, adds and normalises, so the _dev calls use no
// scratch and wait on nothing.  Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>

#include "hash_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"
#include "record_call.hpp"

using namespace bn254;

namespace {
constexpr unsigned H2C_BLOCK = 64;

// lanes [lo, lo + n) of a call: a sub-launch, one record per lane
struct G1MapToCurveOp {
    const uint8_t *u; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * H2C_BLOCK + threadIdx.x;
        if (i < n) h2c_map_body<>(u, out, lo + i);
    }
};
struct G1HashUniformOp {
    const uint8_t *uniform; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * H2C_BLOCK + threadIdx.x;
        if (i < n) h2c_hash_uniform_body<>(uniform, out, lo + i);
    }
};
// the tag travels in the argument record: DST || len(DST), the same for every lane (record_call.hpp bn_h2c_call fills it in)
struct G1HashMsgOp {
    const uint8_t *msgs; uint64_t msg_len; uint32_t *out; uint64_t lo; uint32_t n; uint32_t dst_prime_len; uint8_t dst_prime[H2C_DST_MAX + 1];
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * H2C_BLOCK + threadIdx.x;
        if (i < n) h2c_hash_msg_body<>(msgs, (size_t)msg_len, dst_prime, dst_prime_len, out, lo + i);
    }
};

BnLaunchMax g_hash_launch_max;      // tests only: the sub-launch size

// the family's kinds (record_call.hpp): scope, the input and the bytes of one record of it, of the output.  The message kind's record is msg_len, a per-call value
enum { H2C_MAP, H2C_UNIFORM, H2C_MSG, H2C_KINDS };
constexpr BnRecordKind H2C_KIND[H2C_KINDS] = {{"g1_map_to_curve", 1, {BN254_H2C_FIELD_BYTES}, sizeof(bn_g1), 0}, {"g1_hash_to_curve", 1, {BN254_H2C_UNIFORM_BYTES}, sizeof(bn_g1), 0}, {"g1_hash_to_curve_msg", 1, {0}, sizeof(bn_g1), 0}};
struct HashLaunch {
    int which; G1HashMsgOp m;      // m: the message kind's Op with its tag filled in (bn_h2c_call)
    int operator()(const BnRecordArgs &a, size_t lo, size_t cnt, hipStream_t s) const {
        if (which == H2C_MAP) return bn_lane_launch<H2C_BLOCK>(G1MapToCurveOp{(const uint8_t *)a.in[0], (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        if (which == H2C_UNIFORM) return bn_lane_launch<H2C_BLOCK>(G1HashUniformOp{(const uint8_t *)a.in[0], (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        G1HashMsgOp op = m;
        op.msgs = (const uint8_t *)a.in[0]; op.out = (uint32_t *)a.out; op.lo = lo; op.n = (uint32_t)cnt;
        return bn_lane_launch<H2C_BLOCK>(op, cnt, s);
    }
};
// the two forms of a call of kind `which`; the message kind's rules, record size and tag are record_call.hpp's bn_h2c_call
int hash_dev(bn254_ctx *ctx, int which, const void *d_in, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out, size_t n, void *stream) {
    return bn_h2c_call(H2C_KIND[which], HashLaunch{which, {}}, which == H2C_MSG, msg_len, dst, dst_len, n, [&](const BnRecordKind &k, const HashLaunch &l) { return bn_record_dev(ctx, k, g_hash_launch_max, {{d_in}, d_out}, n, stream, l); });
}
int hash_host(bn254_ctx *ctx, int which, const void *in, size_t msg_len, const uint8_t *dst, size_t dst_len, bn_g1 *out, size_t n) {
    return bn_h2c_call(H2C_KIND[which], HashLaunch{which, {}}, which == H2C_MSG, msg_len, dst, dst_len, n, [&](const BnRecordKind &k, const HashLaunch &l) { return bn_record_host(ctx, k, g_hash_launch_max, {{in}, out}, n, l); });
}
}  // namespace

extern "C" {

int bn254_g1_map_to_curve_batch(bn254_ctx *ctx, const uint8_t *u, bn_g1 *out, size_t n) { return hash_host(ctx, H2C_MAP, u, 0, nullptr, 0, out, n); }
int bn254_g1_hash_to_curve_uniform_batch(bn254_ctx *ctx, const uint8_t *uniform, bn_g1 *out, size_t n) { return hash_host(ctx, H2C_UNIFORM, uniform, 0, nullptr, 0, out, n); }
int bn254_g1_hash_to_curve_batch(bn254_ctx *ctx, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, bn_g1 *out, size_t n) {
    return hash_host(ctx, H2C_MSG, msgs, msg_len, dst, dst_len, out, n);
}
int bn254_g1_map_to_curve_batch_dev(bn254_ctx *ctx, const void *d_u, void *d_out, size_t n, void *stream) { return hash_dev(ctx, H2C_MAP, d_u, 0, nullptr, 0, d_out, n, stream); }
int bn254_g1_hash_to_curve_uniform_batch_dev(bn254_ctx *ctx, const void *d_uniform, void *d_out, size_t n, void *stream) {
    return hash_dev(ctx, H2C_UNIFORM, d_uniform, 0, nullptr, 0, d_out, n, stream);
}
int bn254_g1_hash_to_curve_batch_dev(bn254_ctx *ctx, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out, size_t n, void *stream) {
    return hash_dev(ctx, H2C_MSG, d_msgs, msg_len, dst, dst_len, d_out, n, stream);
}

// internal (not in the header; tests and tools/time_hash.py): an override of the sub-launch size of the six calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records, and which form of inv0 was built
int bn254_hash_set_launch_max(size_t lanes) { return g_hash_launch_max.set(lanes); }
int bn254_hash_inv0_form(void) { return BN254_H2C_INV0; }

}  // extern "C"
