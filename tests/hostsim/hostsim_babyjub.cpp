// TEST INFRASTRUCTURE - host simulation of bn254_bjj_{validate,add,mul}_batch and bn254_eddsa_poseidon_{challenge,verify}_batch: the bodies of
// bn_amd/csrc/babyjub_ops.hpp and the width-6 permutation of poseidon_ops.hpp compiled with g++ for the CPU - the very code the kernels run, one
// loop over lanes per launch, over host arrays.  Built with -DBN_BOUNDS (fe.hpp: a violated bound aborts; fr_dot checks its operands and its
// running value), once with -DBN254_POSEIDON_ROW6_SPLIT=0 and once with =1; both joint windows of the verifier are in each library.  Never
// loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // host_plan.hpp reaches the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/babyjub_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hsb_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
EXPORT int hsb_row6_split() { return BN254_POSEIDON_ROW6_SPLIT; }
EXPORT int hsb_shipped_window() { return BN254_EDDSA_WINDOW; }

// the device forms: sub-launches of at most `step` lanes, each lane through the body; `launches` counts them
template <class Lane>
static int parts(size_t n, size_t step, size_t *launches, Lane lane) {
    *launches = 0;
    if (n == 0) return 0;
    return bn_for_parts(n, step, [&](size_t lo, size_t cnt) -> int { ++*launches; for (size_t i = 0; i < cnt; ++i) lane(lo + i); return 0; });
}
EXPORT int hsb_validate(const uint32_t *p, int32_t *status, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { bjj_validate_body(p, status, i); });
}
EXPORT int hsb_add(const uint32_t *p, const uint32_t *q, uint32_t *out, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { bjj_add_body(p, q, out, i); });
}
EXPORT int hsb_mul(const uint32_t *p, const uint32_t *k, uint32_t *out, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { bjj_mul_body(p, k, out, i); });
}
// the chain alone on a plain 256-bit integer (eight words, least significant first): scalars at and above r, such as 8 l
EXPORT int hsb_mul_raw(const uint32_t *p, const uint32_t *k_raw, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const BjjExt pt = bjj_from_affine(fr_load(p, 2 * i), fr_load(p, 2 * i + 1));
        BjjExt r;
        bjj_mul_chain(pt, fr_load(k_raw, i), r);
        bjj_store_affine(r, out, i);
    }
    return 0;
}
EXPORT int hsb_challenge(const uint32_t *a, const uint32_t *r8, const uint32_t *msg, uint32_t *out, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { eddsa_challenge_body(a, r8, msg, out, i); });
}
EXPORT int hsb_verify(int w, const uint32_t *a, const uint32_t *r8, const uint32_t *s, const uint32_t *msg, int32_t *status, size_t n, size_t step, size_t *launches) {
    if (w != 1 && w != 2) return BN254_E_BAD_ARG;
    return parts(n, step, launches, [&](size_t i) { if (w == 1) eddsa_verify_body<1>(a, r8, s, msg, status, i); else eddsa_verify_body<2>(a, r8, s, msg, status, i); });
}
// the permutation of width 6 on n states; out may be in
EXPORT int hsb_permute6(const uint32_t *in, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) fr_poseidon_permute_body<6>(in, out, i);
    return 0;
}
