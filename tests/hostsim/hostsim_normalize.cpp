// TEST INFRASTRUCTURE - host simulation of the bodies of bn254_g{1,2}_normalize_batch and bn254_g{1,2}_eq_batch (bn_amd/csrc/group_ops.hpp
// normalize_body, eq_body) compiled with g++ for the CPU: the very code the kernels run, one loop over lanes (G1) or simulated lane pairs
// (G2) per launch, over host arrays, for ANY run length K.  Built with -DBN_BOUNDS by tests/test_hostsim_normalize.py: every limb / value
// bound of the lazy number system is enforced at run time.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "lanequad.hpp"
#include "../../bn_amd/csrc/group_ops.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))
typedef FqField G1S;
typedef Fq2Field<Fq2B<FeP>> G2S;

EXPORT int hsn_bounds_enabled() {
#ifdef BN_BOUNDS
    return 1;
#else
    return 0;
#endif
}
EXPORT uint32_t hsn_shipped_run() { return NORM_RUN; }
// a simulated lane pair holds both components of a prefix product: it keeps both records (the kernel's lanes one each, PrefixMem)
struct PrefixPair {
    uint4 *base;
    void put(uint32_t j, const Fq2B<FeP> &a) const {
        prefix_record_put(a.v.v[0], base + (size_t)j * 2 * NORM_PREFIX_U4); prefix_record_put(a.v.v[1], base + ((size_t)j * 2 + 1) * NORM_PREFIX_U4);
    }
    Fq2B<FeP> get(uint32_t j) const {
        return {{{prefix_record_get(base + (size_t)j * 2 * NORM_PREFIX_U4), prefix_record_get(base + ((size_t)j * 2 + 1) * NORM_PREFIX_U4)}}};
    }
};
// one launch over n points in runs of K: ceil(n / K) lanes and one more, which must retire; the prefix scratch is filled with a pattern no
// product can be, so a record read before it was written trips the bound check.  out may be p.
EXPORT void hsn_normalize(int g, const uint32_t *p, uint32_t n, uint32_t K, uint32_t *out) {
    std::vector<uint4> prefix((size_t)n * (g == 1 ? 1 : 2) * NORM_PREFIX_U4 + 1, uint4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu});
    const NormalizeArgs a = {p, out, prefix.data(), n};
    const uint32_t lanes = (n + K - 1) / K;
    for (uint32_t i = 0; i < lanes + 1; ++i) {
        if (g == 1) normalize_body<G1S>(a, i, K, PrefixMem<G1S>{a.prefix, 0u}, PointIo<G1S>());
        else normalize_body<G2S>(a, i, K, PrefixPair{a.prefix}, PointIo<G2S>());
    }
}
EXPORT void hsn_eq(int g, const uint32_t *a, const uint32_t *b, uint32_t n, int32_t *out) {
    for (uint32_t i = 0; i < n; ++i) {
        if (g == 1) { const PointIo<G1S> io; out[i] = eq_body<G1S>(io(a + (size_t)i * io.WORDS), io(b + (size_t)i * io.WORDS)); }
        else { const PointIo<G2S> io; out[i] = eq_body<G2S>(io(a + (size_t)i * io.WORDS), io(b + (size_t)i * io.WORDS)); }
    }
}
