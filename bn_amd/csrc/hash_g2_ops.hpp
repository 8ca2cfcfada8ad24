// Hash to G2 on the GPU (include/bn254_hip.h bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch, bn254_g2_hash_to_curve_uniform_batch,
// bn254_g2_hash_to_curve_batch): the per-lane bodies.  RFC 9380 as for G1 (hash_ops.hpp), over Fq2 and the twist E': y^2 = x^3 + b':
//   * a field element is 96 bytes, c0 then c1, each half reduced by h2c_fe_from_be_words; sgn0 is the RFC's for m = 2;
//   * the Shallue-van de Woestijne map with Z = 1, c1 = g(Z) = 1 + b', c2 = -1/2 (an element of Fq: G1's H2C_C2), c3, c4 from
//     tools/gen_device_constants.py.  inv0 and is_square go through the norm a0^2 + a1^2, an element of Fq: ONE fe_sqrt_cand chain on it gives
//     its inverse (chi t^2 = n^(q-2), 0 for 0) or its character (a is a square in Fq2 exactly when its norm is one in Fq); the root is f2_sqrt
//     (sqrt_ops.hpp, two chains).  Five Fq chains per map, every case a select, the same chain in every lane;
//   * hash_to_curve = clear(map(u0) + map(u1)), uniform bytes u0.c0 | u0.c1 | u1.c0 | u1.c1, expand_message_xmd to 192 bytes;
//   * cofactor clearing, the one step the RFC defines no suite for.  The twist has the 254-bit cofactor 2q - r and a mapped point is NOT in G2.
//         clear(P) = [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P)           (Fuentes-Castaneda, Knapp, Rodriguez-Henriquez, section 6.1)
//     with psi(X, Y, Z) = (conj(X) gx, conj(Y) gy, conj(Z)) on Jacobian coordinates.  It is NOT [2q - r]P (a different multiple of the
//     cofactor), so the formula is part of the interface; on a point Q of G2 it is [k]Q, k = u + 3u lambda + u lambda^2 + lambda^3 mod r.
//     [u]P is plain double-and-add over the 63 fixed bits of u (scalar branches, like fe_sqrt_cand) with the COMPLETE addition: the input is
//     off the subgroup, where psi is not the scalar lambda - scalar_mul_gls (curve.hpp) would be wrong here - and may have small order, so
//     any partial sum may be infinity.  Four additions (one of them [3u]P = [2u]P + [u]P) and one normalisation.
// Neither the constants nor the outputs are checked against gnark-crypto or any other library.
// Everything here is pure and takes plain pointers and a lane index (tests/hostsim/hostsim_hash_g2.cpp runs the very same bodies over host arrays).
#pragma once
#include "hash_ops.hpp"
#include "subgroup_ops.hpp"

namespace bn254 {

constexpr uint32_t H2C_G2_FIELD_BYTES = 96, H2C_G2_UNIFORM_BYTES = 192;

// 24 words of a big-endian byte string: c0 then c1
BN_FN Fq2A h2c_f2_from_be_words(const uint32_t *w) { return {h2c_fe_from_be_words(w), h2c_fe_from_be_words(w + 12)}; }
// sign_0 | (zero_0 & sign_1) on the canonical integers
BN_FN uint32_t h2c_sgn0(const Fq2A &a) {
    uint32_t w0[8], w1[8];
    fe_to_raw_words(a.c0, w0); fe_to_raw_words(a.c1, w1);
    return (w0[0] & 1u) | ((words_all_zero(w0, 8) ? 1u : 0u) & (w1[0] & 1u));
}
BN_FN Fe h2c_f2_norm(const Fq2A &a) { return fe_lc3<1, 1, 0>(fe_sqr(a.c0), fe_sqr(a.c1), a.c1); }
// a in standard form; 1 / a = conj(a) / norm(a), and inv0(0) = 0
BN_FN Fq2A h2c_f2_inv0(const Fq2A &a) {
    const FeSqrtCand c = fe_sqrt_cand<>(h2c_f2_norm(a));
    const Fe ni = fe_mul(c.chi, fe_sqr(c.t));
    const Fe m = fe_mul(a.c1, ni);
    return {fe_mul(a.c0, ni), fe_lc3<-1, 0, 0>(m, m, m)};
}
BN_FN bool h2c_f2_is_square(const Fq2A &a) { return h2c_is_square(fe_sqrt_cand<>(h2c_f2_norm(a))); }
BN_FN Fq2A h2c_g2(const Fq2A &x) { return f2_lc3<1, 1, 0>(f2_mul(f2_sqr(x), x), f2_const((const Fq2A *)nullptr, k::G2_B), x); }

// map_to_curve(u) in the RFC's order; u in standard form.  The point is on the twist, never at infinity, and NOT in G2.
BN_FN void h2c_g2_map(const Fq2A &u, Fq2A &x, Fq2A &y) {
    const Fq2A one = H2cF2::one();
    const Fq2A tv1c = f2_mul(f2_sqr(u), f2_const((const Fq2A *)nullptr, k::H2C_G2_C1));       // u^2 c1
    const Fq2A tv2 = f2_lc3<1, 1, 0>(one, tv1c, tv1c);
    const Fq2A tv1 = f2_lc3<1, -1, 0>(one, tv1c, tv1c);
    const Fq2A tv3 = h2c_f2_inv0(f2_mul(tv1, tv2));
    const Fq2A tv4 = f2_mul(f2_mul(u, tv1), f2_mul(tv3, f2_const((const Fq2A *)nullptr, k::H2C_G2_C3)));
    const Fq2A c2 = {fe_const(k::H2C_C2), fe_zero()};
    const Fq2A x1 = f2_lc3<1, -1, 0>(c2, tv4, tv4), x2 = f2_lc3<1, 1, 0>(c2, tv4, tv4);
    const Fq2A t = f2_mul(f2_sqr(tv2), tv3);
    const Fq2A x3 = f2_lc3<1, 1, 0>(f2_mul(f2_sqr(t), f2_const((const Fq2A *)nullptr, k::H2C_G2_C4)), one, one);       // + Z, Z = 1
    const bool e1 = h2c_f2_is_square(h2c_g2(x1));
    const bool e2 = h2c_f2_is_square(h2c_g2(x2)) && !e1;
    x = f2_select(e1, f2_select(e2, x3, x2), x1);
    const Fq2A r = f2_sqrt<>(h2c_g2(x)).root;                                    // g(x) is a square: the root exists
    y = f2_select(h2c_sgn0(r) != h2c_sgn0(u), r, f2_neg(r));
}

// ---- psi, psi^2, psi^3 on Jacobian coordinates (the constants k::TWIST_MUL_BY_Q_X, k::TWIST_MUL_BY_Q_Y, k::GLS_W, k::GLS_WGX) and [u]P over the
// bits of k::BN_U, h2c_mul_u, live in subgroup_ops.hpp: the membership test of G2 runs the same chain
// clear(P), not normalised.  Out of line with P handed over by reference, so that P lives in private memory through the 62 steps of the
// chain: inlined into the clearing kernel, the allocation kept P, the running point and an addition's values in registers and spilled 45 of them
BN_OUTER H2cJac2 h2c_clear(const H2cJac2 &p) {
    const H2cJac2 up = h2c_mul_u(p);
    H2cJac2 acc = add_body<H2cF2>(h2c_psi3(p), h2c_psi2(up), 0);                 // ordered for short live ranges: P is dead from here on
    acc = add_body<H2cF2>(acc, up, 0);
    const H2cJac2 u3 = add_body<H2cF2>(jac_double(up), up, 0);                   // [3u]P
    return add_body<H2cF2>(acc, h2c_psi(u3), 0);
}

// ---- the bodies: record i of a launch
// 96 bytes -> (x, y, 1) on the twist
BN_FN void h2c_g2_map_body(const uint8_t *in, uint32_t *out, size_t i) {
    uint32_t w[24];
    h2c_load_be_words(in + H2C_G2_FIELD_BYTES * i, w, 24);
    Fq2A x, y;
    h2c_g2_map(h2c_f2_from_be_words(w), x, y);
    uint32_t o[48];
    f2_store(x, o); f2_store(y, o + 16); f2_store(H2cF2::one(), o + 32);
    for (int j = 0; j < 48; ++j) out[48 * i + j] = o[j];
}
// any Jacobian point of the twist (Z = 0: infinity) -> clear(P), normalised; infinity comes back as G2::zero() = (0, 1, 0).  out may be p.
BN_FN void h2c_g2_clear_body(const uint32_t *p, uint32_t *out, size_t i) {
    const PointIo<H2cF2> io;
    const H2cJac2 r = jac_normalize<H2cF2>(h2c_clear(io(p + 48 * i)));
    uint32_t o[48];
    io(r, o);
    for (int j = 0; j < 48; ++j) out[48 * i + j] = o[j];
}
// 48 words of the uniform string -> clear(map(u0) + map(u1)), normalised
BN_FN void h2c_g2_hash_words(const uint32_t *w, uint32_t *out) {
    H2cJac2 p[2];
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        Fq2A x, y;
        h2c_g2_map(h2c_f2_from_be_words(w + 24 * j), x, y);
        if (j == 0) p[0] = {x, y, H2cF2::one()}; else p[1] = {x, y, H2cF2::one()};
    }
    const H2cJac2 r = jac_normalize<H2cF2>(h2c_clear(add_body<H2cF2>(p[0], p[1], 0)));
    uint32_t o[48];
    PointIo<H2cF2>()(r, o);
    for (int j = 0; j < 48; ++j) out[j] = o[j];
}
BN_FN void h2c_g2_hash_uniform_body(const uint8_t *in, uint32_t *out, size_t i) {
    uint32_t w[48];
    h2c_load_be_words(in + H2C_G2_UNIFORM_BYTES * i, w, 48);
    h2c_g2_hash_words(w, out + 48 * i);
}
// message i of msg_len bytes -> hash_to_curve
BN_FN void h2c_g2_hash_msg_body(const uint8_t *msgs, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint32_t *out, size_t i) {
    uint32_t w[48];
    h2c_expand_xmd<H2C_G2_UNIFORM_BYTES / 32>(msgs + msg_len * i, msg_len, dst_prime, dst_prime_len, w);
    h2c_g2_hash_words(w, out + 48 * i);
}
// the expansion alone (host simulation)
BN_FN void h2c_g2_expand_body(const uint8_t *msg, size_t msg_len, const uint8_t *dst_prime, uint32_t dst_prime_len, uint8_t *out) {
    uint32_t w[48];
    h2c_expand_xmd<H2C_G2_UNIFORM_BYTES / 32>(msg, msg_len, dst_prime, dst_prime_len, w);
    for (int i = 0; i < 48; ++i) { out[4 * i] = (uint8_t)(w[i] >> 24); out[4 * i + 1] = (uint8_t)(w[i] >> 16); out[4 * i + 2] = (uint8_t)(w[i] >> 8); out[4 * i + 3] = (uint8_t)w[i]; }
}

}  // namespace bn254
