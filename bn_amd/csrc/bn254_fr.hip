// The scalar field on the device (include/bn254_hip.h bn254_fr_{add,mul,inverse,pow,interpret}_batch and their _dev twins): the kernels -
// Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one element (inverse: one run of elements) per lane over the
// bodies of fr_ops.hpp -, their sub-launches, and the ten entry points.
#include <algorithm>

#include "fr_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned FR_BLOCK = 256;

struct FrAddOp {
    const uint32_t *a, *b; uint32_t *out; uint32_t n; int negate_b;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * FR_BLOCK + threadIdx.x;
        if (i < n) fr_add_body(a, b, out, i, negate_b);
    }
};
struct FrMulOp {
    const uint32_t *a, *b; uint32_t *out; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * FR_BLOCK + threadIdx.x;
        if (i < n) fr_mul_body(a, b, out, i);
    }
};
template <int WB>
struct FrPowOp {
    const uint32_t *a, *e; uint32_t *out; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * FR_BLOCK + threadIdx.x;
        if (i < n) fr_pow_body<WB>(a, e, out, i);
    }
};
struct FrInterpretOp {
    const uint8_t *in; uint32_t *out; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * FR_BLOCK + threadIdx.x;
        if (i < n) fr_interpret_body(in, out, i);
    }
};
// lane i owns the run of K elements from i * K on
struct FrInverseOp {
    const uint32_t *a; uint32_t *out; int32_t *ok; uint32_t *prefix; uint32_t n, lanes, K;
    __device__ __forceinline__ void operator()() const {
        fr_inverse_body<FR_POW_WINDOW>(a, out, ok, prefix, n, blockIdx.x * FR_BLOCK + threadIdx.x, lanes, K);
    }
};
// tests and tools/time_fr.py only: the sub-launch size, and the variants the sweep times
BnLaunchMax g_fr_launch_max;
BnOverride<unsigned> g_fr_inverse_run, g_fr_pow_window;

enum FrKind { FR_ADD, FR_SUB, FR_MUL, FR_POW };
const char *const FR_SCOPE[] = {"fr_add", "fr_add", "fr_mul", "fr_pow"};
// out[i] = a[i] op b[i]: sub-launches of at most g_fr_launch_max.step() elements
int fr_launch_binary(bn254_ctx *c, FrKind kind, const void *d_a, const void *d_b, void *d_out, size_t n, hipStream_t s) {
    const unsigned wb = g_fr_pow_window.get(FR_POW_WINDOW);
    return bn_for_parts(n, g_fr_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        const uint32_t *a = (const uint32_t *)d_a + 8 * lo, *b = (const uint32_t *)d_b + 8 * lo;
        uint32_t *out = (uint32_t *)d_out + 8 * lo;
        BnScope sc(c, s, FR_SCOPE[kind]);
        switch (kind) {
        case FR_ADD: case FR_SUB: return bn_lane_launch<FR_BLOCK>(FrAddOp{a, b, out, (uint32_t)cnt, kind == FR_SUB}, cnt, s);
        case FR_MUL: return bn_lane_launch<FR_BLOCK>(FrMulOp{a, b, out, (uint32_t)cnt}, cnt, s);
        default:
            if (wb == 1) return bn_lane_launch<FR_BLOCK>(FrPowOp<1>{a, b, out, (uint32_t)cnt}, cnt, s);
            if (wb == 4) return bn_lane_launch<FR_BLOCK>(FrPowOp<4>{a, b, out, (uint32_t)cnt}, cnt, s);
            return bn_lane_launch<FR_BLOCK>(FrPowOp<2>{a, b, out, (uint32_t)cnt}, cnt, s);
        }
    });
}
int fr_launch_interpret(bn254_ctx *c, const void *d_in, void *d_out, size_t n, hipStream_t s) {
    return bn_for_parts(n, g_fr_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, "fr_interpret");
        return bn_lane_launch<FR_BLOCK>(FrInterpretOp{(const uint8_t *)d_in + 64 * lo, (uint32_t *)d_out + 8 * lo, (uint32_t)cnt}, cnt, s);
    });
}
// scratch guard held by the caller: the prefix products of one sub-launch (K * lanes records of 32 bytes) are context-owned
int fr_launch_inverse(bn254_ctx *c, const void *d_a, void *d_out, void *d_ok, size_t n, hipStream_t s) {
    const size_t step = g_fr_launch_max.step(), K = g_fr_inverse_run.get(FR_INV_RUN), most = std::min(n, step);
    int rc = c->fr_prefix.reserve(((most + K - 1) / K) * K * sizeof(bn_fr)); if (rc) return rc;
    return bn_for_parts(n, step, [&](size_t lo, size_t cnt) -> int {
        const size_t lanes = (cnt + K - 1) / K;
        BnScope sc(c, s, "fr_inverse");
        return bn_lane_launch<FR_BLOCK>(FrInverseOp{(const uint32_t *)d_a + 8 * lo, (uint32_t *)d_out + 8 * lo, d_ok ? (int32_t *)d_ok + lo : nullptr, (uint32_t *)c->fr_prefix.p,
                                     (uint32_t)cnt, (uint32_t)lanes, (uint32_t)K}, lanes, s);
    });
}

// order of the checks: empty batch, arguments, then context and device
int fr_binary_dev(bn254_ctx *ctx, FrKind kind, const void *d_a, const void *d_b, void *d_out, size_t n, void *stream) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !d_a || !d_b || !d_out) return BN254_E_BAD_ARG;            // before any device lookup
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return fr_launch_binary(ctx, kind, d_a, d_b, d_out, n, s); });
}
int fr_binary_host(bn254_ctx *ctx, FrKind kind, const bn_fr *a, const bn_fr *b, bn_fr *out, size_t n) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !a || !b || !out) return BN254_E_BAD_ARG;                  // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {a, n * sizeof(bn_fr)}, {b, n * sizeof(bn_fr)}, out, n * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return fr_binary_dev(ctx, kind, d.in[0], d.in[1], d.out, n, ctx->stream); });
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------- device-resident API
int bn254_fr_add_batch_dev(bn254_ctx *c, const void *a, const void *b, void *o, size_t n, int negate_b, void *s) { return fr_binary_dev(c, negate_b ? FR_SUB : FR_ADD, a, b, o, n, s); }
int bn254_fr_mul_batch_dev(bn254_ctx *c, const void *a, const void *b, void *o, size_t n, void *s) { return fr_binary_dev(c, FR_MUL, a, b, o, n, s); }
int bn254_fr_pow_batch_dev(bn254_ctx *c, const void *a, const void *e, void *o, size_t n, void *s) { return fr_binary_dev(c, FR_POW, a, e, o, n, s); }
int bn254_fr_inverse_batch_dev(bn254_ctx *ctx, const void *d_a, void *d_out, void *d_ok, size_t n, void *stream) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !d_a || !d_out) return BN254_E_BAD_ARG;                    // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return fr_launch_inverse(ctx, d_a, d_out, d_ok, n, s); });
}
int bn254_fr_interpret_batch_dev(bn254_ctx *ctx, const void *d_in, void *d_out, size_t n, void *stream) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !d_in || !d_out) return BN254_E_BAD_ARG;                   // before any device lookup
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return fr_launch_interpret(ctx, d_in, d_out, n, s); });
}

// ---------------------------------------------------------------------------------------------- host-buffer API (BnHost: the context's mutex for the call)
int bn254_fr_add_batch(bn254_ctx *c, const bn_fr *a, const bn_fr *b, bn_fr *o, size_t n, int negate_b) { return fr_binary_host(c, negate_b ? FR_SUB : FR_ADD, a, b, o, n); }
int bn254_fr_mul_batch(bn254_ctx *c, const bn_fr *a, const bn_fr *b, bn_fr *o, size_t n) { return fr_binary_host(c, FR_MUL, a, b, o, n); }
int bn254_fr_pow_batch(bn254_ctx *c, const bn_fr *a, const bn_fr *e, bn_fr *o, size_t n) { return fr_binary_host(c, FR_POW, a, e, o, n); }
int bn254_fr_inverse_batch(bn254_ctx *ctx, const bn_fr *a, bn_fr *out, int32_t *ok, size_t n) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !a || !out) return BN254_E_BAD_ARG;                        // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {a, n * sizeof(bn_fr)}, {nullptr, 0}, out, n * sizeof(bn_fr), ok, n * sizeof(int32_t),
                     [&](const BnStaged &d) { return bn254_fr_inverse_batch_dev(ctx, d.in[0], d.out, d.out2, n, ctx->stream); });
}
int bn254_fr_interpret_batch(bn254_ctx *ctx, const uint8_t *in, bn_fr *out, size_t n) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !in || !out) return BN254_E_BAD_ARG;                       // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {in, n * 64}, {nullptr, 0}, out, n * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_interpret_batch_dev(ctx, d.in[0], d.out, n, ctx->stream); });
}

// internal (not in the header; tests and tools/time_fr.py): the shipped run length of the inversion and window width of pow, an override of
// the sub-launch size (0 restores BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of elements, and -
// for the sweep only - process-wide overrides of the run length and the width (0 restores the shipped one; same bytes whatever is set)
unsigned bn254_fr_inverse_run(void) { return FR_INV_RUN; }
unsigned bn254_fr_pow_window(void) { return FR_POW_WINDOW; }
int bn254_fr_set_launch_max(size_t elements) { return g_fr_launch_max.set(elements); }
size_t bn254_fr_launch_step(void) { return g_fr_launch_max.step(); }          // bn254_fr_sqrt.hip: the square roots cut their sub-launches by the same override
int bn254_fr_set_inverse_run(unsigned K) { return K > 64 ? BN254_E_BAD_ARG : g_fr_inverse_run.set(K); }
int bn254_fr_set_pow_window(unsigned bits) { return bits != 0 && bits != 1 && bits != 2 && bits != 4 ? BN254_E_BAD_ARG : g_fr_pow_window.set(bits); }

}  // extern "C"
