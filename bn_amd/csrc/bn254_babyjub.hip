// Baby Jubjub and EdDSA-Poseidon on the device (include/bn254_hip.h bn254_bjj_validate_batch, bn254_bjj_add_batch, bn254_bjj_mul_batch,
// bn254_bjj_pack_batch, bn254_bjj_unpack_batch, bn254_eddsa_poseidon_challenge_batch, bn254_eddsa_poseidon_verify_batch,
// bn254_eddsa_poseidon_verify_packed_batch and their _dev twins): the kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other
// integer kernels, one lane of a body of babyjub_ops.hpp each - and the sixteen entry points.  One launch per call (and per sub-launch of a
// large one), the verifiers included: a lane (unpacks its two points,) hashes, runs its joint chain and compares, so the _dev calls use no
// scratch and wait on nothing.  Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>

#include "babyjub_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned BJJ_BLOCK = 64;
// (The verifier holds 258 VGPRs, one wave per SIMD.  In workgroups of 512 lanes the compiler keeps it within 256 - two waves - but spills two
// VGPRs, in both window widths: above the shell's ceiling of zero, so it runs in workgroups of 64 like the others.)
constexpr size_t BJJ_N_MAX = (size_t)1 << 40;

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

BnLaunchMax g_bjj_launch_max;
BnOverride<unsigned> g_bjj_sqrt_form;  // tools/time_bjj_pack.py: form + 1 of the unpacking's square root (0 = the shipped BN254_FR_SQRT_FORM)          // tests only: the sub-launch size

enum { BJJ_VALIDATE, BJJ_ADD, BJJ_MUL, BJJ_CHALLENGE, BJJ_VERIFY, BJJ_PACK, BJJ_UNPACK, BJJ_VERIFY_PACKED, BJJ_KINDS };
const char *const BJJ_SCOPE[] = {"bjj_validate", "bjj_add", "bjj_mul", "eddsa_poseidon_challenge", "eddsa_poseidon_verify", "bjj_pack", "bjj_unpack", "eddsa_poseidon_verify_packed"};
// inputs of a call (device or host pointers) and the bytes of one record of each; the output, and the second one of the calls that have one
struct BjjArgs { const void *in[4]; int n_in; void *out; void *out2; };
constexpr size_t BJJ_IN_BYTES[BJJ_KINDS][4] = {{64, 0, 0, 0}, {64, 64, 0, 0}, {64, 32, 0, 0}, {64, 64, 32, 0}, {64, 64, 32, 32}, {64, 0, 0, 0}, {32, 0, 0, 0}, {32, 64, 32, 0}};
constexpr size_t BJJ_OUT_BYTES[BJJ_KINDS] = {sizeof(int32_t), 64, 64, 32, sizeof(int32_t), 32, 64, sizeof(int32_t)};
constexpr size_t BJJ_OUT2_BYTES[BJJ_KINDS] = {0, 0, 0, 0, 0, 0, sizeof(int32_t), 0};

// arguments only: nothing here touches a device.  1 = nothing to do
int bjj_check(int what, const BjjArgs &a, size_t n) {
    if (n == 0) return 1;
    if (!a.out || (BJJ_OUT2_BYTES[what] && !a.out2) || n > BJJ_N_MAX) return BN254_E_BAD_ARG;
    for (int j = 0; j < a.n_in; ++j)
        if (!a.in[j]) return BN254_E_BAD_ARG;
    return BN254_OK;
}
int bjj_run(bn254_ctx *ctx, int what, const BjjArgs &a, size_t n, hipStream_t s) {
    const uint32_t *const i0 = (const uint32_t *)a.in[0], *const i1 = (const uint32_t *)a.in[1], *const i2 = (const uint32_t *)a.in[2], *const i3 = (const uint32_t *)a.in[3];
    return bn_for_parts(n, g_bjj_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(ctx, s, BJJ_SCOPE[what]);
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
    });
}
// order of the checks: arguments, then context and device; nothing waits, nothing is read back
int bjj_dev(bn254_ctx *ctx, int what, const BjjArgs &a, size_t n, void *stream) {
    int rc = bjj_check(what, a, n); if (rc) return rc == 1 ? BN254_OK : rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return bjj_run(ctx, what, a, n, s); });
}
// The host-buffer form: up to four inputs, so not bn_staged's shape (three).  Every input is staged in ONE buffer (ctx->stage[0]; each record
// size is a multiple of 32 bytes, so every part stays aligned), the output in ctx->stage[2] and a second one in ctx->stage[3]; on the
// context's stream under a BnHost, drained on an error like bn_staged
int bjj_host(bn254_ctx *ctx, int what, const BjjArgs &a, size_t n) {
    int rc = bjj_check(what, a, n); if (rc) return rc == 1 ? BN254_OK : rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    const hipStream_t s = ctx->stream;
    auto run = [&]() -> int {
        size_t total = 0;
        for (int j = 0; j < a.n_in; ++j) total += n * BJJ_IN_BYTES[what][j];
        int r;
        if ((r = ctx->stage[0].reserve(total)) || (r = ctx->stage[2].reserve(n * BJJ_OUT_BYTES[what]))) return r;
        if (BJJ_OUT2_BYTES[what] && (r = ctx->stage[3].reserve(n * BJJ_OUT2_BYTES[what]))) return r;
        BjjArgs d = {{nullptr, nullptr, nullptr, nullptr}, a.n_in, ctx->stage[2].p, BJJ_OUT2_BYTES[what] ? ctx->stage[3].p : nullptr};
        size_t off = 0;
        for (int j = 0; j < a.n_in; ++j) {
            d.in[j] = (const char *)ctx->stage[0].p + off;
            HIP_TRY(hipMemcpyAsync((char *)ctx->stage[0].p + off, a.in[j], n * BJJ_IN_BYTES[what][j], hipMemcpyHostToDevice, s));
            off += n * BJJ_IN_BYTES[what][j];
        }
        if ((r = bjj_run(ctx, what, d, n, s))) return r;
        HIP_TRY(hipMemcpyAsync(a.out, d.out, n * BJJ_OUT_BYTES[what], hipMemcpyDeviceToHost, s));
        if (BJJ_OUT2_BYTES[what]) HIP_TRY(hipMemcpyAsync(a.out2, d.out2, n * BJJ_OUT2_BYTES[what], hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    };
    rc = bn_no_throw(run);
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}
}  // namespace

extern "C" {

int bn254_bjj_validate_batch(bn254_ctx *ctx, const bn_fr *p, int32_t *status, size_t n) { return bjj_host(ctx, BJJ_VALIDATE, {{p}, 1, status}, n); }
int bn254_bjj_add_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *q, bn_fr *out, size_t n) { return bjj_host(ctx, BJJ_ADD, {{p, q}, 2, out}, n); }
int bn254_bjj_mul_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *k, bn_fr *out, size_t n) { return bjj_host(ctx, BJJ_MUL, {{p, k}, 2, out}, n); }
int bn254_eddsa_poseidon_challenge_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *r8, const bn_fr *msg, bn_fr *out, size_t n) {
    return bjj_host(ctx, BJJ_CHALLENGE, {{a, r8, msg}, 3, out}, n);
}
int bn254_eddsa_poseidon_verify_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *r8, const bn_fr *s, const bn_fr *msg, int32_t *status, size_t n) {
    return bjj_host(ctx, BJJ_VERIFY, {{a, r8, s, msg}, 4, status}, n);
}
int bn254_bjj_pack_batch(bn254_ctx *ctx, const bn_fr *p, uint8_t *out32, size_t n) { return bjj_host(ctx, BJJ_PACK, {{p}, 1, out32}, n); }
int bn254_bjj_unpack_batch(bn254_ctx *ctx, const uint8_t *in32, bn_fr *out, int32_t *status, size_t n) { return bjj_host(ctx, BJJ_UNPACK, {{in32}, 1, out, status}, n); }
int bn254_eddsa_poseidon_verify_packed_batch(bn254_ctx *ctx, const uint8_t *a32, const uint8_t *sig64, const bn_fr *msg, int32_t *status, size_t n) {
    return bjj_host(ctx, BJJ_VERIFY_PACKED, {{a32, sig64, msg}, 3, status}, n);
}
int bn254_bjj_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream) { return bjj_dev(ctx, BJJ_VALIDATE, {{d_p}, 1, d_status}, n, stream); }
int bn254_bjj_add_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, void *d_out, size_t n, void *stream) { return bjj_dev(ctx, BJJ_ADD, {{d_p, d_q}, 2, d_out}, n, stream); }
int bn254_bjj_mul_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, void *d_out, size_t n, void *stream) { return bjj_dev(ctx, BJJ_MUL, {{d_p, d_k}, 2, d_out}, n, stream); }
int bn254_eddsa_poseidon_challenge_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_r8, const void *d_msg, void *d_out, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_CHALLENGE, {{d_a, d_r8, d_msg}, 3, d_out}, n, stream);
}
int bn254_eddsa_poseidon_verify_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_r8, const void *d_s, const void *d_msg, void *d_status, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_VERIFY, {{d_a, d_r8, d_s, d_msg}, 4, d_status}, n, stream);
}
int bn254_bjj_pack_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_out32, size_t n, void *stream) { return bjj_dev(ctx, BJJ_PACK, {{d_p}, 1, d_out32}, n, stream); }
int bn254_bjj_unpack_batch_dev(bn254_ctx *ctx, const void *d_in32, void *d_out, void *d_status, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_UNPACK, {{d_in32}, 1, d_out, d_status}, n, stream);
}
int bn254_eddsa_poseidon_verify_packed_batch_dev(bn254_ctx *ctx, const void *d_a32, const void *d_sig64, const void *d_msg, void *d_status, size_t n, void *stream) {
    return bjj_dev(ctx, BJJ_VERIFY_PACKED, {{d_a32, d_sig64, d_msg}, 3, d_status}, n, stream);
}

// internal (not in the header; tests, tools/time_babyjub.py and tools/time_bjj_pack.py): an override of the sub-launch size of the calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records, and the joint window the library was built with
int bn254_bjj_set_launch_max(size_t lanes) { return g_bjj_launch_max.set(lanes); }
int bn254_eddsa_window(void) { return BN254_EDDSA_WINDOW; }
// the form of the square root bn254_bjj_unpack_batch runs: a process-wide override for the measurement that chose it (-1 restores the shipped one)
int bn254_bjj_set_sqrt_form(int form) { return form < -1 || form > 1 ? BN254_E_BAD_ARG : g_bjj_sqrt_form.set((unsigned)(form + 1)); }

}  // extern "C"
