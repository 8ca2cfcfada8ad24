// Hash to G1 on the GPU (include/bn254_hip.h bn254_g1_map_to_curve_batch, bn254_g1_hash_to_curve_uniform_batch, bn254_g1_hash_to_curve_batch):
// the per-lane bodies.  RFC 9380: the Shallue-van de Woestijne map (the only standard map for this curve: A = 0 and q = 1 mod 3 rule out SSWU
// without an isogeny), hash_to_curve = map(u0) + map(u1) (random-oracle variant; cofactor 1, nothing to clear), hash_to_field with L = 48 and
// expand_message_xmd over SHA-256.  Z = 1 and c1 .. c4 come from tools/gen_device_constants.py, derived from the RFC's formulas and not checked
// against gnark-crypto or any other library.  sgn0(a) is the canonical integer of a mod 2 - not the y > -y rule of io_compress.hpp.
//
// Every exponentiation is the same chain in all lanes and every case a select: fe_sqrt_cand (sqrt_ops.hpp) gives the two character tests and
// the root; inv0 has two forms behind one compile-time switch, BN254_H2C_INV0:
//     0   fe_inverse_fermat (fe.hpp): a^(q-2) bit by bit, 0 for a = 0
//     1   the candidate chain itself: t = a^((q-3)/4), chi = a^((q-1)/2), a^-1 = chi t^2 = a^(q-2), 0 for a = 0
// Both are templates over the form, so the host simulation runs the two under -DBN_BOUNDS whichever one the library ships.  Everything here is
// pure and takes plain pointers and a lane index (tests/hostsim/hostsim_hash.cpp runs the very same bodies over host arrays).
#pragma once
#include <stddef.h>
#include "group_ops.hpp"
#include "io_wire.hpp"
#include "sqrt_ops.hpp"

#ifndef BN254_H2C_INV0
#define BN254_H2C_INV0 1               // the faster of the two on map_to_curve of 2^20 elements (profiles/r22_hash.txt); 0 stays buildable: tools/build_variant.sh
#endif

namespace bn254 {

constexpr uint32_t H2C_FIELD_BYTES = 48, H2C_UNIFORM_BYTES = 96, H2C_DST_MAX = 255;

// ---- a field element from 12 words of a big-endian byte string (word 0 = bytes 0 .. 3): any value below 2^384, taken mod q.  The low 256
// bits are below 2^256 < 6 q, the high 128 bits below q; one dual product against 2^522 and 2^778 (raw) leaves v * 2^261 as a product (1, 2).
BN_FN Fe h2c_fe_from_be_words(const uint32_t *w) {
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { lo[i] = w[11 - i]; hi[i] = i < 4 ? w[3 - i] : 0u; }
    Fe l = fe_unpack_u32x8(lo), h = fe_unpack_u32x8(hi);
    BN_IFB(l.vb = 6;)                                   // claimed, then checked against the limbs: not assumed
    BN_VERIFY(l, "h2c_fe_from_be_words lo"); BN_VERIFY(h, "h2c_fe_from_be_words hi");
    return fe_mul2(l, fe_const(k::C_RAW_IN), h, fe_const(k::C_RAW_HI));
}
BN_FN void h2c_load_be_words(const uint8_t *in, uint32_t *w, int n) {
    for (int i = 0; i < n; ++i) w[i] = ((uint32_t)in[4 * i] << 24) | ((uint32_t)in[4 * i + 1] << 16) | ((uint32_t)in[4 * i + 2] << 8) | (uint32_t)in[4 * i + 3];
}
BN_FN uint32_t h2c_sgn0(const Fe &a) {
    uint32_t w[8];
    fe_to_raw_words(a, w);
    return w[0] & 1u;
}
// a: a product or a fused reduction (1, 2)
template <int INV0>
BN_FN Fe h2c_inv0(const Fe &a) {
    if (INV0 == 0) return fe_inverse_fermat(a);
    const FeSqrtCand c = fe_sqrt_cand<>(a);
    return fe_mul(c.chi, fe_sqr(c.t));
}
BN_FN Fe h2c_g(const Fe &x) { return fe_lc3<1, 1, 0>(fe_mul(fe_sqr(x), x), fe_const(k::G1_B), x); }
BN_FN bool h2c_is_square(const FeSqrtCand &c) { return !fe_is_zero(fe_add(c.chi, fe_one())); }      // chi is 0, 1 or -1; zero counts as a square

// map_to_curve(u) in the RFC's order; u is a product (1, 2).  The point is never at infinity.
template <int INV0>
BN_FN void h2c_map(const Fe &u, Fe &x, Fe &y) {
    const Fe one = fe_one();
    const Fe usq = fe_sqr(u);
    const Fe tv1c = fe_lc3<4, 0, 0>(usq, usq, usq);                          // u^2 c1, c1 = g(Z) = 4
    const Fe tv2 = fe_norm(fe_add(one, tv1c));                               // (1, 3)
    const Fe tv1 = fe_lc3<1, -1, 0>(one, tv1c, tv1c);
    const Fe tv3 = h2c_inv0<INV0>(fe_mul(tv1, tv2));
    const Fe tv4 = fe_mul(fe_mul(u, tv1), fe_mul(tv3, fe_const(k::H2C_C3)));
    const Fe c2 = fe_const(k::H2C_C2);
    const Fe x1 = fe_lc3<1, -1, 0>(c2, tv4, tv4), x2 = fe_lc3<1, 1, 0>(c2, tv4, tv4);
    const Fe t = fe_mul(fe_sqr(tv2), tv3);
    const Fe x3 = fe_lc3<1, 1, 0>(fe_mul(fe_sqr(t), fe_const(k::H2C_C4)), one, one);       // + Z, Z = 1
    const bool e1 = h2c_is_square(fe_sqrt_cand<>(h2c_g(x1)));
    const bool e2 = h2c_is_square(fe_sqrt_cand<>(h2c_g(x2))) && !e1;
    x = fe_select(e1, fe_select(e2, x3, x2), x1);
    const Fe r = fe_sqrt_cand<>(h2c_g(x)).y;                                 // g(x) is a square: the candidate is the root
    y = fe_select(h2c_sgn0(r) != h2c_sgn0(u), r, fe_lc3<-1, 0, 0>(r, r, r));
}

// ---- the bodies: record i of a launch
// 48 bytes -> (x, y, 1)
template <int INV0 = BN254_H2C_INV0>
BN_FN void h2c_map_body(const uint8_t *in, uint32_t *out, size_t i) {
    uint32_t w[12];
    h2c_load_be_words(in + H2C_FIELD_BYTES * i, w, 12);
    Fe x, y;
    h2c_map<INV0>(h2c_fe_from_be_words(w), x, y);
    uint32_t o[24];
    fe_to_u32x8(x, o); fe_to_u32x8(y, o + 8); fe_to_u32x8(fe_one(), o + 16);
    for (int j = 0; j < 24; ++j) out[24 * i + j] = o[j];
}
// 24 words of the uniform string -> map(u0) + map(u1), normalised: the complete addition (equal points double, opposite points give
// G::zero() = (0, 1, 0)) and one inversion
template <int INV0>
BN_FN void h2c_hash_words(const uint32_t *w, uint32_t *out) {
    Jac<FqField> p[2];
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        Fe x, y;
        h2c_map<INV0>(h2c_fe_from_be_words(w + 12 * j), x, y);
        if (j == 0) p[0] = {x, y, fe_one()}; else p[1] = {x, y, fe_one()};
    }
    const Jac<FqField> r = jac_normalize<FqField>(add_body<FqField>(p[0], p[1], 0));
    uint32_t o[24];
    PointIo<FqField>()(r, o);
    for (int j = 0; j < 24; ++j) out[j] = o[j];
}
template <int INV0 = BN254_H2C_INV0>
BN_FN void h2c_hash_uniform_body(const uint8_t *in, uint32_t *out, size_t i) {
    uint32_t w[24];
    h2c_load_be_words(in + H2C_UNIFORM_BYTES * i, w, 24);
    h2c_hash_words<INV0>(w, out + 24 * i);
}

// ---- SHA-256 in plain 32-bit arithmetic, one message per lane, streamed byte by byte through a 16-word block buffer
BN254_CONSTANT uint32_t SHA256_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
    0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
    0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
struct Sha256 {
    uint32_t h[8], w[16];
    uint32_t fill;                     // bytes in the block buffer
    uint64_t total;                    // bytes taken so far
};
BN_FN uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
BN_FN void sha256_init(Sha256 &s) {
    const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    for (int i = 0; i < 8; ++i) s.h[i] = iv[i];
    for (int i = 0; i < 16; ++i) s.w[i] = 0;
    s.fill = 0; s.total = 0;
}
// the block buffer into the state; the buffer comes back cleared
BN_FN void sha256_block(Sha256 &s) {
    uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], hh = s.h[7];
#pragma unroll 1
    for (int r = 0; r < 64; ++r) {
        if (r >= 16) {
            const uint32_t w15 = s.w[(r + 1) & 15], w2 = s.w[(r + 14) & 15];
            s.w[r & 15] += (sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3)) + s.w[(r + 9) & 15] + (sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = hh + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) + SHA256_K[r] + s.w[r & 15];
        const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    s.h[0] += a; s.h[1] += b; s.h[2] += c; s.h[3] += d; s.h[4] += e; s.h[5] += f; s.h[6] += g; s.h[7] += hh;
    for (int i = 0; i < 16; ++i) s.w[i] = 0;
    s.fill = 0;
}
BN_FN void sha256_byte(Sha256 &s, uint32_t b) {
    s.w[s.fill >> 2] |= (b & 0xffu) << (24 - 8 * (s.fill & 3u));
    ++s.total;
    if (++s.fill == 64) sha256_block(s);
}
BN_FN void sha256_bytes(Sha256 &s, const uint8_t *p, size_t n) {
#pragma unroll 1
    for (size_t i = 0; i < n; ++i) sha256_byte(s, p[i]);
}
BN_FN void sha256_word(Sha256 &s, uint32_t v) {           // four bytes, most significant first
#pragma unroll 1
    for (int k = 24; k >= 0; k -= 8) sha256_byte(s, v >> k);
}
// padding and the last block(s); the digest is s.h
BN_FN void sha256_finish(Sha256 &s) {
    const uint64_t bits = s.total * 8;
    sha256_byte(s, 0x80);
    if (s.fill > 56) sha256_block(s);                     // no room for the length: it goes into a block of its own
    s.w[14] = (uint32_t)(bits >> 32); s.w[15] = (uint32_t)bits;
    sha256_block(s);
}
// expand_message_xmd(msg, DST, 32 ELL) as 8 ELL words, ELL <= 7 blocks (the length fits l_i_b_str's low byte: 96 for G1, 192 for G2).
// dst_prime = DST || len(DST), dst_prime_len = len(DST) + 1 <= 256
template <uint32_t ELL>
BN_FN void h2c_expand_xmd(const uint8_t *msg, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint32_t *out) {
    static_assert(ELL >= 1 && 32 * ELL <= 255, "h2c_expand_xmd length");
    Sha256 s;
    sha256_init(s);
    sha256_block(s);                                      // Z_pad: 64 zero bytes are one block
    s.total = 64;
    sha256_bytes(s, msg, msg_len);
    sha256_byte(s, 0); sha256_byte(s, 32 * ELL); sha256_byte(s, 0);               // l_i_b_str, then the index 0
    sha256_bytes(s, dst_prime, dst_prime_len);
    sha256_finish(s);
    uint32_t b0[8], prev[8];
    for (int i = 0; i < 8; ++i) { b0[i] = s.h[i]; prev[i] = 0; }
#pragma unroll 1
    for (uint32_t j = 1; j <= ELL; ++j) {
        sha256_init(s);
#pragma unroll 1
        for (int i = 0; i < 8; ++i) sha256_word(s, b0[i] ^ prev[i]);
        sha256_byte(s, j);
        sha256_bytes(s, dst_prime, dst_prime_len);
        sha256_finish(s);
        for (int i = 0; i < 8; ++i) { prev[i] = s.h[i]; out[8 * (j - 1) + i] = s.h[i]; }
    }
}
BN_FN void h2c_expand_xmd96(const uint8_t *msg, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint32_t *out) {
    h2c_expand_xmd<H2C_UNIFORM_BYTES / 32>(msg, msg_len, dst_prime, dst_prime_len, out);
}
// message i of msg_len bytes -> hash_to_curve
template <int INV0 = BN254_H2C_INV0>
BN_FN void h2c_hash_msg_body(const uint8_t *msgs, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint32_t *out, size_t i) {
    uint32_t w[24];
    h2c_expand_xmd96(msgs + msg_len * i, msg_len, dst_prime, dst_prime_len, w);
    h2c_hash_words<INV0>(w, out + 24 * i);
}
// the expansion alone (host simulation)
BN_FN void h2c_expand_body(const uint8_t *msg, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint8_t *out) {
    uint32_t w[24];
    h2c_expand_xmd96(msg, msg_len, dst_prime, dst_prime_len, w);
    for (int i = 0; i < 24; ++i) { out[4 * i] = (uint8_t)(w[i] >> 24); out[4 * i + 1] = (uint8_t)(w[i] >> 16); out[4 * i + 2] = (uint8_t)(w[i] >> 8); out[4 * i + 3] = (uint8_t)w[i]; }
}

}  // namespace bn254
