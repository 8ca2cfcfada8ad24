// TEST INFRASTRUCTURE - host simulation of hash-to-curve for G2 and of the cofactor clearing: the bodies of bn_amd/csrc/hash_g2_ops.hpp compiled
// with g++ for the CPU - the very code the kernels run, one call per lane.  Built with -DBN_BOUNDS (fe.hpp: a violated bound aborts).  Never
// loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "../../bn_amd/csrc/hash_g2_ops.hpp"

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hsg_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
// 96 big-endian bytes -> the ABI's Montgomery image of (c0 mod q, c1 mod q) (16 words) and sgn0 of it
EXPORT uint32_t hsg_field(const uint8_t *in, uint32_t *out) {
    uint32_t w[24];
    h2c_load_be_words(in, w, 24);
    const Fq2A a = h2c_f2_from_be_words(w);
    f2_store(a, out);
    return h2c_sgn0(a);
}
// a -> inv0(a) and is_square(a), Montgomery images
EXPORT int hsg_inv0(const uint32_t *a, uint32_t *out) {
    const Fq2A x = f2_load((const Fq2A *)nullptr, a);
    f2_store(h2c_f2_inv0(x), out);
    return h2c_f2_is_square(x) ? 1 : 0;
}
EXPORT void hsg_map(const uint8_t *u, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) h2c_g2_map_body(u, out, i);
}
EXPORT void hsg_clear(const uint32_t *p, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) h2c_g2_clear_body(p, out, i);
}
// psi^j on Jacobian coordinates, j = 1, 2, 3 (as they stand: not normalised)
EXPORT void hsg_psi(int j, const uint32_t *p, uint32_t *out) {
    const PointIo<H2cF2> io;
    const H2cJac2 a = io(p);
    io(j == 1 ? h2c_psi(a) : j == 2 ? h2c_psi2(a) : h2c_psi3(a), out);
}
EXPORT void hsg_hash_uniform(const uint8_t *uniform, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) h2c_g2_hash_uniform_body(uniform, out, i);
}
EXPORT void hsg_hash_msg(const uint8_t *msgs, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) h2c_g2_hash_msg_body(msgs, msg_len, dst_prime, dst_prime_len, out, i);
}
EXPORT void hsg_expand(const uint8_t *msg, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint8_t *out) {
    h2c_g2_expand_body(msg, msg_len, dst_prime, dst_prime_len, out);
}
