// TEST INFRASTRUCTURE - host simulation of point validation and of the two membership tests of G2: the bodies of bn_amd/csrc/subgroup_ops.hpp and the
// G2 decoders of io_wire.hpp / io_compress.hpp compiled with g++ for the CPU - the very code the kernels run, one call per lane.  Built with
// -DBN_BOUNDS (fe.hpp: a violated bound aborts).  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "../../bn_amd/csrc/subgroup_ops.hpp"
#include "../../bn_amd/csrc/io_wire.hpp"
#include "../../bn_amd/csrc/io_compress.hpp"

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hss_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
// which membership test g2_in_subgroup (the decoders') is compiled to
EXPORT int hss_decoders_use_endo() { return BN254_G2_SUBGROUP_ENDO; }
EXPORT void hss_g1_validate(const uint32_t *p, int32_t *status, size_t n) {
    for (size_t i = 0; i < n; ++i) g1_validate_body(p, status, i);
}
EXPORT void hss_g2_validate(const uint32_t *p, int32_t *status, size_t n) {
    for (size_t i = 0; i < n; ++i) g2_validate_body(p, status, i);
}
// the endomorphism test on one Jacobian record (48 words, below q)
EXPORT int hss_endo(const uint32_t *p) {
    const H2cJac2 a = PointIo<H2cF2>()(p);
    return g2_in_subgroup_endo(a) ? 1 : 0;
}
// the two forms behind the decoders on an affine pair (x, y) (32 words): the r - 1 chain, and g2_in_subgroup as compiled
EXPORT int hss_chain(const uint32_t *xy) {
    return g2_in_subgroup_chain(f2_load((const Fq2A *)nullptr, xy), f2_load((const Fq2A *)nullptr, xy + 16)) ? 1 : 0;
}
EXPORT int hss_decoder_test(const uint32_t *xy) {
    return g2_in_subgroup(f2_load((const Fq2A *)nullptr, xy), f2_load((const Fq2A *)nullptr, xy + 16)) ? 1 : 0;
}
EXPORT int hss_g2_decode(const uint8_t *in, uint32_t *out) { return g2_decode_record(in, out); }
EXPORT int hss_g2_decompress(int form, const uint8_t *in, int format, uint32_t *out) {
    return form ? g2_decompress_record<1>(in, format, out) : g2_decompress_record<0>(in, format, out);
}
