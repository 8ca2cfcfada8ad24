// TEST INFRASTRUCTURE - host simulation of hash-to-curve for G1: the bodies of bn_amd/csrc/hash_ops.hpp compiled with g++ for the CPU - the very
// code the kernels run, one call per lane.  Built with -DBN_BOUNDS (fe.hpp: a violated bound aborts).  Both forms of inv0 are instantiated here,
// whichever of the two the library ships.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "../../bn_amd/csrc/hash_ops.hpp"

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hsh_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
// 48 big-endian bytes -> the ABI's Montgomery image of the value mod q (8 words)
EXPORT void hsh_field(const uint8_t *in, uint32_t *out) {
    uint32_t w[12];
    h2c_load_be_words(in, w, 12);
    fe_to_u32x8(h2c_fe_from_be_words(w), out);
}
// a -> inv0(a), Montgomery images
EXPORT void hsh_inv0(int inv0, const uint32_t *a, uint32_t *out) {
    const Fe x = fe_from_u32x8(a);
    fe_to_u32x8(inv0 ? h2c_inv0<1>(x) : h2c_inv0<0>(x), out);
}
EXPORT void hsh_map(int inv0, const uint8_t *u, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) { if (inv0) h2c_map_body<1>(u, out, i); else h2c_map_body<0>(u, out, i); }
}
EXPORT void hsh_hash_uniform(int inv0, const uint8_t *uniform, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) { if (inv0) h2c_hash_uniform_body<1>(uniform, out, i); else h2c_hash_uniform_body<0>(uniform, out, i); }
}
EXPORT void hsh_hash_msg(int inv0, const uint8_t *msgs, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (inv0) h2c_hash_msg_body<1>(msgs, msg_len, dst_prime, dst_prime_len, out, i);
        else h2c_hash_msg_body<0>(msgs, msg_len, dst_prime, dst_prime_len, out, i);
    }
}
EXPORT void hsh_expand(const uint8_t *msg, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint8_t *out) {
    h2c_expand_body(msg, msg_len, dst_prime, dst_prime_len, out);
}
