// Membership of G2 by the endomorphism, and the validation of raw points (include/bn254_hip.h bn254_g1_validate_batch,
// bn254_g2_validate_batch): the per-lane bodies.  The twist E'(Fq2) has the 254-bit cofactor 2q - r, so "on the curve" is not "in G2".
//   * psi(X, Y, Z) = (conj(X) gx, conj(Y) gy, conj(Z)) on Jacobian coordinates and its powers, and [u]P by plain double-and-add over the 63
//     fixed bits of u = BN_U with the COMPLETE addition: valid for every point of the twist, never the GLS multiplication (scalar_mul_gls,
//     curve.hpp, replaces psi by the scalar lambda, which is only right ON the subgroup).  The cofactor clearing of hash_g2_ops.hpp uses the same.
//   * the test (the criterion gnark-crypto's bn254 uses):
//         P in G2   <=>   [u + 1]P + psi([u]P) + psi^2([u]P) == psi^3([2u]P)
//     Soundness: psi satisfies X^2 - tX + q = 0 on E'(Fq2), t = 6u^2 + 1.  g(X) = (u + 1) + uX + uX^2 - 2uX^3 reduces modulo that polynomial
//     to a + bX, and a point g(psi) kills is killed by the integer N = a^2 + abt + b^2 q; r divides N and gcd(N, 2q - r) = 1, so the order of
//     such a point divides gcd(N, r (2q - r)) = r.  Completeness: on G2 psi is the scalar lambda = 6u^2 mod r and g(lambda) = 0 mod r.
//     (tests/subgroup_cases.py asserts the three facts on integers.)  One [u] chain (62 doublings, 27 additions), one doubling, four additions
//     and three psi maps against the 253 doublings and 127 additions of [r - 1]P + P == 0 (io_wire.hpp g2_in_subgroup_chain).
//     A point of small order may make any partial sum infinity: every addition is the complete one, and the two sides are compared by a
//     complete subtraction, so infinity on both sides counts as equal.
//   * validation: one ABI record (x, y, z), Montgomery words, any z, gives one status with the wire format's numbers (io_wire.hpp WIRE_*), in the
//     order of the compressed decoders: 1 a coordinate's words are not below q (compared as they stand, before any field conversion), 0 for
//     z == 0 (infinity, whatever x and y hold), 4 unless Y^2 == X^3 + b Z^6, 5 (G2 only) unless the test above accepts.  G1 has cofactor 1.
//     Every lane runs the same chain and every case is a select.
// Everything here is pure and takes plain pointers and a lane index (tests/hostsim/hostsim_subgroup.cpp runs the very same bodies over host arrays).
#pragma once
#include <stddef.h>
#include "group_ops.hpp"

namespace bn254 {

using H2cF2 = Fq2Field<Fq2A>;
using H2cJac2 = Jac<H2cF2>;

// ---- psi and its powers on Jacobian coordinates (psi^2 = (w X, -Y, Z), psi^3 = (conj(X) w gx, -conj(Y) gy, conj(Z)): the constants of GLS)
BN_FN H2cJac2 h2c_psi(const H2cJac2 &p) {
    return {f2_mul_const(f2_conj_lazy(p.x), k::TWIST_MUL_BY_Q_X), f2_mul_const(f2_conj_lazy(p.y), k::TWIST_MUL_BY_Q_Y), f2_conj(p.z)};
}
BN_FN H2cJac2 h2c_psi2(const H2cJac2 &p) { return {f2_scale(p.x, fe_const(k::GLS_W)), f2_neg(p.y), p.z}; }
BN_FN H2cJac2 h2c_psi3(const H2cJac2 &p) {
    return {f2_mul_const(f2_conj_lazy(p.x), k::GLS_WGX), f2_neg(f2_mul_const(f2_conj_lazy(p.y), k::TWIST_MUL_BY_Q_Y)), f2_conj(p.z)};
}
// [u]P for any point of the twist, infinity (Z = 0) included: 62 doublings and the additions of the set bits of u below its top one
BN_FN H2cJac2 h2c_mul_u(const H2cJac2 &p) {
    H2cJac2 acc = p;
#pragma unroll 1
    for (int i = 61; i >= 0; --i) {                                              // u has 63 bits; the top one is consumed by acc = p
        acc = jac_double(acc);
        if ((k::BN_U >> i) & 1) acc = add_body<H2cF2>(acc, p, 0);
    }
    return acc;
}

// ---- P in G2, for any Jacobian point of the twist (Z = 0: infinity, a member).  Out of line with P handed over by reference, like
// h2c_clear (hash_g2_ops.hpp): P lives in private memory through the 62 steps of the chain instead of in registers next to the running point
BN_OUTER bool g2_in_subgroup_endo(const H2cJac2 &p) {
    const H2cJac2 up = h2c_mul_u(p);
    H2cJac2 lhs = add_body<H2cF2>(up, p, 0);                                     // [u + 1]P: P is dead from here on
    lhs = add_body<H2cF2>(lhs, h2c_psi(up), 0);
    lhs = add_body<H2cF2>(lhs, h2c_psi2(up), 0);
    const H2cJac2 rhs = h2c_psi3(jac_double(up));                                // psi^3([2u]P)
    return H2cF2::is_zero(add_body<H2cF2>(lhs, rhs, 1).z);                       // lhs - rhs == 0; both at infinity: equal
}

// ---- validation: record i of a launch
// 8 words as they stand -> the field element of their value mod q (a coordinate that is not below q is reported, not trusted: any 256-bit value is below 6q)
BN_FN Fe val_fe_load(const uint32_t *w) {
    Fe u = fe_unpack_u32x8(w);
    BN_IFB(u.vb = 6;)
    return fe_mul(u, fe_const(k::C_IN));
}
BN_FN int32_t val_status(bool in_range, bool inf, bool on_curve, bool in_subgroup) {
    return !in_range ? 1 : inf ? 0 : !on_curve ? 4 : !in_subgroup ? 5 : 0;
}
BN_FN void g1_validate_body(const uint32_t *p, int32_t *status, size_t i) {
    uint32_t w[24];
    for (int j = 0; j < 24; ++j) w[j] = p[24 * i + j];
    const bool in_range = words_lt_q(w) & words_lt_q(w + 8) & words_lt_q(w + 16);
    const bool inf = words_all_zero(w + 16, 8);
    const Fe x = val_fe_load(w), y = val_fe_load(w + 8), z = val_fe_load(w + 16);
    const Fe z2 = fe_sqr(z);
    const Fe rhs = fe_lc3<1, 3, 0>(fe_mul(fe_sqr(x), x), fe_mul(fe_sqr(z2), z2), x);      // X^3 + 3 Z^6
    const bool on_curve = fe_is_zero(fe_lc3<1, -1, 0>(fe_sqr(y), rhs, y));
    status[i] = val_status(in_range, inf, on_curve, true);
}
BN_FN void g2_validate_body(const uint32_t *p, int32_t *status, size_t i) {
    uint32_t w[48];
    for (int j = 0; j < 48; ++j) w[j] = p[48 * i + j];
    bool in_range = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) in_range &= words_lt_q(w + 8 * j);
    const bool inf = words_all_zero(w + 32, 16);
    const H2cJac2 pt = {{val_fe_load(w), val_fe_load(w + 8)}, {val_fe_load(w + 16), val_fe_load(w + 24)}, {val_fe_load(w + 32), val_fe_load(w + 40)}};
    const Fq2A z2 = f2_sqr(pt.z);
    const Fq2A bz6 = f2_mul(f2_mul(f2_sqr(z2), z2), f2_const((const Fq2A *)nullptr, k::G2_B));
    const Fq2A rhs = f2_lc3<1, 1, 0>(f2_mul(f2_sqr(pt.x), pt.x), bz6, pt.x);              // X^3 + b' Z^6
    const bool on_curve = f2_is_zero(f2_lc3<1, -1, 0>(f2_sqr(pt.y), rhs, pt.y));
    status[i] = val_status(in_range, inf, on_curve, g2_in_subgroup_endo(pt));
}

}  // namespace bn254
