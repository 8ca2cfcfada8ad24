// Square roots in the scalar field on the device (include/bn254_hip.h bn254_fr_sqrt_batch and its _dev twin): the kernel - an Op of
// lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one element per lane over the body of fr_sqrt_ops.hpp, both forms of the
// correction instantiated -, its sub-launches and the two entry points.  A unit of its own beside bn254_fr.hip, whose sub-launch override it
// shares (bn254_fr_set_launch_max).  No scratch, no LDS, no atomics.  Compiled like every unit (bn254_hip.hip: the flags).
#include "fr_sqrt_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

extern "C" size_t bn254_fr_launch_step(void);          // bn254_fr.hip

namespace {
// in workgroups of 64 like the other callers of fr_sqrt_ratio (bn254_babyjub.hip)
constexpr unsigned FR_SQRT_BLOCK = 64;
template <int FORM>
struct FrSqrtOp {
    const uint32_t *a; uint32_t *out; int32_t *ok; uint32_t n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * FR_SQRT_BLOCK + threadIdx.x;
        if (i < n) fr_sqrt_body<FORM>(a, out, ok, i);
    }
};
BnOverride<unsigned> g_fr_sqrt_form;       // tools/time_bjj_pack.py: form + 1 (0 = the shipped BN254_FR_SQRT_FORM)

int fr_launch_sqrt(bn254_ctx *c, const void *d_a, void *d_out, void *d_ok, size_t n, hipStream_t s) {
    const unsigned form = g_fr_sqrt_form.get(BN254_FR_SQRT_FORM + 1) - 1;
    return bn_for_parts(n, bn254_fr_launch_step(), [&](size_t lo, size_t cnt) -> int {
        const uint32_t *a = (const uint32_t *)d_a + 8 * lo;
        uint32_t *out = (uint32_t *)d_out + 8 * lo;
        int32_t *ok = d_ok ? (int32_t *)d_ok + lo : nullptr;
        BnScope sc(c, s, "fr_sqrt");
        if (form == 0) return bn_lane_launch<FR_SQRT_BLOCK>(FrSqrtOp<0>{a, out, ok, (uint32_t)cnt}, cnt, s);
        return bn_lane_launch<FR_SQRT_BLOCK>(FrSqrtOp<1>{a, out, ok, (uint32_t)cnt}, cnt, s);
    });
}
}  // namespace

extern "C" {

// order of the checks: empty batch, arguments, then context and device.  d_ok may be NULL, d_out may be d_a
int bn254_fr_sqrt_batch_dev(bn254_ctx *ctx, const void *d_a, void *d_out, void *d_ok, size_t n, void *stream) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !d_a || !d_out) return BN254_E_BAD_ARG;                    // before any device lookup
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return fr_launch_sqrt(ctx, d_a, d_out, d_ok, n, s); });
}
int bn254_fr_sqrt_batch(bn254_ctx *ctx, const bn_fr *a, bn_fr *out, int32_t *ok, size_t n) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !a || !out) return BN254_E_BAD_ARG;                        // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {a, n * sizeof(bn_fr)}, {nullptr, 0}, out, n * sizeof(bn_fr), ok, n * sizeof(int32_t),
                     [&](const BnStaged &d) { return bn254_fr_sqrt_batch_dev(ctx, d.in[0], d.out, d.out2, n, ctx->stream); });
}

// internal (not in the header; tests and tools/time_bjj_pack.py): the form of the correction the library was built with, and a process-wide
// override for the measurement of the two (-1 restores the shipped one; same bytes whatever is set)
int bn254_fr_sqrt_form(void) { return BN254_FR_SQRT_FORM; }
int bn254_fr_set_sqrt_form(int form) { return form < -1 || form > 1 ? BN254_E_BAD_ARG : g_fr_sqrt_form.set((unsigned)(form + 1)); }

}  // extern "C"
