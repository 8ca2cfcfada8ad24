// TEST INFRASTRUCTURE - host simulation of the bodies of bn254_fr_{add,mul,inverse,pow,interpret}_batch and of the synthetic-scalar generator
// (bn_amd/csrc/fr_ops.hpp over the arithmetic of fr.hpp) compiled
// with g++ for the CPU: the very code the kernels run, one loop over lanes per launch, over host arrays, for ANY run length K of the
// inversion and every window width of pow the library carries.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "../../bn_amd/csrc/fr_ops.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT uint32_t hsf_shipped_run() { return FR_INV_RUN; }
EXPORT uint32_t hsf_shipped_window() { return FR_POW_WINDOW; }
// one launch over n elements; out may be a or b
EXPORT void hsf_add(const uint32_t *a, const uint32_t *b, uint32_t n, int negate_b, uint32_t *out) {
    for (uint32_t i = 0; i < n; ++i) fr_add_body(a, b, out, i, negate_b);
}
EXPORT void hsf_mul(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out) {
    for (uint32_t i = 0; i < n; ++i) fr_mul_body(a, b, out, i);
}
EXPORT int hsf_pow(const uint32_t *a, const uint32_t *e, uint32_t n, uint32_t wb, uint32_t *out) {
    if (wb != 1 && wb != 2 && wb != 4) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        if (wb == 1) fr_pow_body<1>(a, e, out, i);
        else if (wb == 2) fr_pow_body<2>(a, e, out, i);
        else fr_pow_body<4>(a, e, out, i);
    }
    return 0;
}
EXPORT void hsf_interpret(const uint8_t *in, uint32_t n, uint32_t *out) {
    for (uint32_t i = 0; i < n; ++i) fr_interpret_body(in, out, i);
}
// one launch of bn254_synthetic_scalars_k: elements lo .. lo + n of stream `which`
EXPORT void hsf_synthetic(uint64_t seed, uint64_t lo, uint32_t n, uint32_t which, uint32_t *out) {
    for (uint32_t j = 0; j < n; ++j) fr_synthetic_body(seed, lo, j, which, out);
}
// runs of K: ceil(n / K) lanes and one more, which must retire; the prefix scratch holds exactly K * lanes records (std::vector::at would
// throw past them) and is filled with a pattern no product can be; ok may be NULL
EXPORT int hsf_inverse(const uint32_t *a, uint32_t n, uint32_t K, uint32_t wb, uint32_t *out, int32_t *ok) {
    if (wb != 1 && wb != 2 && wb != 4) return -1;
    const uint32_t lanes = (n + K - 1) / K;
    std::vector<uint32_t> prefix((size_t)K * lanes * 8, 0xffffffffu);
    for (uint32_t i = 0; i < lanes + 1; ++i) {
        if (wb == 1) fr_inverse_body<1>(a, out, ok, prefix.data(), n, i, lanes, K);
        else if (wb == 2) fr_inverse_body<2>(a, out, ok, prefix.data(), n, i, lanes, K);
        else fr_inverse_body<4>(a, out, ok, prefix.data(), n, i, lanes, K);
    }
    return 0;
}
