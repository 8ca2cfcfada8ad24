// Baby Jubjub and EdDSA-Poseidon on the device (include/bn254_hip.h bn254_bjj_validate_batch, bn254_bjj_add_batch, bn254_bjj_mul_batch,
// bn254_bjj_pack_batch, bn254_bjj_unpack_batch, bn254_eddsa_poseidon_challenge_batch, bn254_eddsa_poseidon_verify_batch,
// bn254_eddsa_poseidon_verify_packed_batch and their _dev twins): the kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other
// integer kernels, one lane of a body of babyjub_ops.hpp each -, the family's kind table and launch switch, and the sixteen entry points on
// record_call.hpp's one path.  One launch per call (and per sub-launch of a large one), the verifiers included: a lane (unpacks its two
// points,) hashes, runs its joint chain and compares, so the _dev calls use no scratch and wait on nothing.
// Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>

#include "babyjub_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"
#include "record_call.hpp"

using namespace bn254;

namespace {
constexpr unsigned BJJ_BLOCK = 64;
// (The verifier holds 258 VGPRs, one wave per SIMD.  In workgroups of 512 lanes the compiler keeps it within 256 - two waves - but spills two
// VGPRs, in both window widths: above the shell's ceiling of zero, so it runs in workgroups of 64 like the others.)

// lanes [lo, lo + n) of a call: a sub-launch, one record per lane
struct BjjValidateOp {
    const uint32_t *p; int32_t *status; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) bjj_validate_body(p, status, lo + i);
    }
};
struct BjjAddOp {
    const uint32_t *p, *q; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) bjj_add_body(p, q, out, lo + i);
    }
};
struct BjjMulOp {
    const uint32_t *p, *k; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) bjj_mul_body(p, k, out, lo + i);
    }
};
struct EddsaChallengeOp {
    const uint32_t *a, *r8, *msg; uint32_t *out; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) eddsa_challenge_body(a, r8, msg, out, lo + i);
    }
};
struct EddsaVerifyOp {
    const uint32_t *a, *r8, *s, *msg; int32_t *status; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) eddsa_verify_body<BN254_EDDSA_WINDOW>(a, r8, s, msg, status, lo + i);
    }
};
struct BjjPackOp {
    const uint32_t *p; uint32_t *out32; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) bjj_pack_body(p, out32, lo + i);
    }
};
template <int FORM>
struct BjjUnpackOp {
    const uint32_t *in32; uint32_t *out; int32_t *status; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) bjj_unpack_body<FORM>(in32, out, status, lo + i);
    }
};
struct EddsaVerifyPackedOp {
    const uint32_t *a32, *sig64, *msg; int32_t *status; uint64_t lo; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BJJ_BLOCK + threadIdx.x;
        if (i < n) eddsa_verify_packed_body<BN254_EDDSA_WINDOW, BN254_FR_SQRT_FORM>(a32, sig64, msg, status, lo + i);
    }
};

BnLaunchMax g_bjj_launch_max;          // tests only: the sub-launch size
BnOverride<unsigned> g_bjj_sqrt_form;  // tools/time_bjj_pack.py: form + 1 of the unpacking's square root (0 = the shipped BN254_FR_SQRT_FORM)

// the family's kinds (record_call.hpp): scope, inputs and the bytes of one record of each, of the output, of the second output of the kind that has one
enum { BJJ_VALIDATE, BJJ_ADD, BJJ_MUL, BJJ_CHALLENGE, BJJ_VERIFY, BJJ_PACK, BJJ_UNPACK, BJJ_VERIFY_PACKED, BJJ_KINDS };
constexpr BnRecordKind BJJ_KIND[BJJ_KINDS] = {
    {"bjj_validate", 1, {64}, sizeof(int32_t), 0},
    {"bjj_add", 2, {64, 64}, 64, 0},
    {"bjj_mul", 2, {64, 32}, 64, 0},
    {"eddsa_poseidon_challenge", 3, {64, 64, 32}, 32, 0},
    {"eddsa_poseidon_verify", 4, {64, 64, 32, 32}, sizeof(int32_t), 0},
    {"bjj_pack", 1, {64}, 32, 0},
    {"bjj_unpack", 1, {32}, 64, sizeof(int32_t)},
    {"eddsa_poseidon_verify_packed", 3, {32, 64, 32}, sizeof(int32_t), 0}};
struct BjjLaunch {
    int what;
    int operator()(const BnRecordArgs &a, size_t lo, size_t cnt, hipStream_t s) const {
        const uint32_t *const i0 = (const uint32_t *)a.in[0], *const i1 = (const uint32_t *)a.in[1], *const i2 = (const uint32_t *)a.in[2], *const i3 = (const uint32_t *)a.in[3];
        switch (what) {
        case BJJ_VALIDATE: return bn_lane_launch<BJJ_BLOCK>(BjjValidateOp{i0, (int32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        case BJJ_ADD: return bn_lane_launch<BJJ_BLOCK>(BjjAddOp{i0, i1, (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        case BJJ_MUL: return bn_lane_launch<BJJ_BLOCK>(BjjMulOp{i0, i1, (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        case BJJ_PACK: return bn_lane_launch<BJJ_BLOCK>(BjjPackOp{i0, (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        case BJJ_UNPACK:
            if (g_bjj_sqrt_form.get(BN254_FR_SQRT_FORM + 1) == 1) return bn_lane_launch<BJJ_BLOCK>(BjjUnpackOp<0>{i0, (uint32_t *)a.out, (int32_t *)a.out2, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
            return bn_lane_launch<BJJ_BLOCK>(BjjUnpackOp<1>{i0, (uint32_t *)a.out, (int32_t *)a.out2, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        case BJJ_VERIFY_PACKED: return bn_lane_launch<BJJ_BLOCK>(EddsaVerifyPackedOp{i0, i1, i2, (int32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        case BJJ_CHALLENGE: return bn_lane_launch<BJJ_BLOCK>(EddsaChallengeOp{i0, i1, i2, (uint32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        default: return bn_lane_launch<BJJ_BLOCK>(EddsaVerifyOp{i0, i1, i2, i3, (int32_t *)a.out, (uint64_t)lo, (uint32_t)cnt}, cnt, s);
        }
    }
};
// the two forms of a call of kind `what`: checks, sub-launches, staging (up to four inputs: EdDSA verification)
int bjj_host(bn254_ctx *ctx, int what, const BnRecordArgs &a, size_t n) { return bn_record_host(ctx, BJJ_KIND[what], g_bjj_launch_max, a, n, BjjLaunch{what}); }
int bjj_dev(bn254_ctx *ctx, int what, const BnRecordArgs &a, size_t n, void *stream) { return bn_record_dev(ctx, BJJ_KIND[what], g_bjj_launch_max, a, n, stream, BjjLaunch{what}); }
}  // namespace

extern "C" {

int bn254_bjj_validate_batch(bn254_ctx *ctx, const bn_fr *p, int32_t *status, size_t n) { return bjj_host(ctx, BJJ_VALIDATE, {{p}, status}, n); }
int bn254_bjj_add_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *q, bn_fr *out, size_t n) { return bjj_host(ctx, BJJ_ADD, {{p, q}, out}, n); }
int bn254_bjj_mul_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *k, bn_fr *out, size_t n) { return bjj_host(ctx, BJJ_MUL, {{p, k}, out}, n); }
int bn254_eddsa_poseidon_challenge_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *r8, const bn_fr *msg, bn_fr *out, size_t n) {
    return bjj_host(ctx, BJJ_CHALLENGE, {{a, r8, msg}, out}, n);
}
int bn254_eddsa_poseidon_verify_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *r8, const bn_fr *s, const bn_fr *msg, int32_t *status, size_t n) {
    return bjj_host(ctx, BJJ_VERIFY, {{a, r8, s, msg}, status}, n);
}
int bn254_bjj_pack_batch(bn254_ctx *ctx, const bn_fr *p, uint8_t *out32, size_t n) { return bjj_host(ctx, BJJ_PACK, {{p}, out32}, n); }
int bn254_bjj_unpack_batch(bn254_ctx *ctx, const uint8_t *in32, bn_fr *out, int32_t *status, size_t n) { return bjj_host(ctx, BJJ_UNPACK, {{in32}, out, status}, n); }
int bn254_eddsa_poseidon_verify_packed_batch(bn254_ctx *ctx, const uint8_t *a32, const uint8_t *sig64, const bn_fr *msg, int32_t *status, size_t n) {
    return bjj_host(ctx, BJJ_VERIFY_PACKED, {{a32, sig64, msg}, status}, n);
}
int bn254_bjj_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream) { return bjj_dev(ctx, BJJ_VALIDATE, {{d_p}, d_status}, n, stream); }
int bn254_bjj_add_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, void *d_out, size_t n, void *stream) { return bjj_dev(ctx, BJJ_ADD, {{d_p, d_q}, d_out}, n, stream); }
int bn254_bjj_mul_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, void *d_out, size_t n, void *stream) { return bjj_dev(ctx, BJJ_MUL, {{d_p, d_k}, d_out}, n, stream); }
int bn254_eddsa_poseidon_challenge_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_r8, const void *d_msg, void *d_out, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_CHALLENGE, {{d_a, d_r8, d_msg}, d_out}, n, stream);
}
int bn254_eddsa_poseidon_verify_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_r8, const void *d_s, const void *d_msg, void *d_status, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_VERIFY, {{d_a, d_r8, d_s, d_msg}, d_status}, n, stream);
}
int bn254_bjj_pack_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_out32, size_t n, void *stream) { return bjj_dev(ctx, BJJ_PACK, {{d_p}, d_out32}, n, stream); }
int bn254_bjj_unpack_batch_dev(bn254_ctx *ctx, const void *d_in32, void *d_out, void *d_status, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_UNPACK, {{d_in32}, d_out, d_status}, n, stream);
}
int bn254_eddsa_poseidon_verify_packed_batch_dev(bn254_ctx *ctx, const void *d_a32, const void *d_sig64, const void *d_msg, void *d_status, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_VERIFY_PACKED, {{d_a32, d_sig64, d_msg}, d_status}, n, stream);
}

// internal (not in the header; tests, tools/time_babyjub.py and tools/time_bjj_pack.py): an override of the sub-launch size of the calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records, and the joint window the library was built with
int bn254_bjj_set_launch_max(size_t lanes) { return g_bjj_launch_max.set(lanes); }
int bn254_eddsa_window(void) { return BN254_EDDSA_WINDOW; }
// the form of the square root bn254_bjj_unpack_batch runs: a process-wide override for the measurement that chose it (-1 restores the shipped one)
int bn254_bjj_set_sqrt_form(int form) { return form < -1 || form > 1 ? BN254_E_BAD_ARG : g_bjj_sqrt_form.set((unsigned)(form + 1)); }

}  // extern "C"
