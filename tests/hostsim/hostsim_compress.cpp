// TEST INFRASTRUCTURE - host simulation of the compressed encodings: the square roots of bn_amd/csrc/sqrt_ops.hpp and the record bodies of
// io_compress.hpp compiled with g++ for the CPU - the very code the kernels run, one call per lane.  Built with -DBN_BOUNDS (fe.hpp: a violated
// bound aborts).  Both forms of the exponentiation chain are instantiated here, whichever of the two the library ships.  Never loaded by the
// product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "../../bn_amd/csrc/io_compress.hpp"

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hsc_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
// a, t, y, chi: the ABI's Montgomery images (8 words)
EXPORT void hsc_fe_sqrt_cand(int form, const uint32_t *a, uint32_t *t, uint32_t *y, uint32_t *chi) {
    const Fe x = fe_from_u32x8(a);
    const FeSqrtCand c = form ? fe_sqrt_cand<1>(x) : fe_sqrt_cand<0>(x);
    fe_to_u32x8(c.t, t); fe_to_u32x8(c.y, y); fe_to_u32x8(c.chi, chi);
}
// a, root: (c0, c1), 16 words.  Returns is_square
EXPORT int hsc_f2_sqrt(int form, const uint32_t *a, uint32_t *root) {
    const Fq2A x = f2_load((const Fq2A *)nullptr, a);
    const F2Sqrt r = form ? f2_sqrt<1>(x) : f2_sqrt<0>(x);
    f2_store(r.root, root);
    return r.is_square ? 1 : 0;
}
EXPORT int hsc_fe_sign(const uint32_t *a) { return fe_sign(fe_from_u32x8(a)) ? 1 : 0; }
EXPORT int hsc_f2_sign(const uint32_t *a) { return f2_sign(f2_load((const Fq2A *)nullptr, a)) ? 1 : 0; }
EXPORT void hsc_g1_compress(const uint32_t *p, int format, uint8_t *out) { g1_compress_record(p, format, out); }
EXPORT void hsc_g2_compress(const uint32_t *p, int format, uint8_t *out) { g2_compress_record(p, format, out); }
EXPORT int hsc_g1_decompress(int form, const uint8_t *in, int format, uint32_t *out) {
    return form ? g1_decompress_record<1>(in, format, out) : g1_decompress_record<0>(in, format, out);
}
EXPORT int hsc_g2_decompress(int form, const uint8_t *in, int format, uint32_t *out) {
    return form ? g2_decompress_record<1>(in, format, out) : g2_decompress_record<0>(in, format, out);
}
