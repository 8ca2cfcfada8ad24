// Baby Jubjub and EdDSA-Poseidon on the device (include/bn254_hip.h bn254_bjj_{validate,add,mul}_batch, bn254_eddsa_poseidon_{challenge,verify}_batch):
// the per-lane bodies.  The curve is the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr (a = 168700 a square, d = 168696 not one), so
// it is the first group over fr.hpp: everything goes through fr_mul / fr_add / fr_sub on canonical values - fr_mul's precondition holds
// everywhere and the bytes are those of the integer model.
//   * a point in memory: two consecutive Fr, x then y, Montgomery words, affine.  In a lane: extended coordinates (X : Y : Z : T), x = X / Z,
//     y = Y / Z, T = X Y / Z (Hisil-Wong-Carter-Dawson 2008).  O = (0 : 1 : 1 : 0), -(X : Y : Z : T) = (-X : Y : Z : -T).
//   * addition, unified and a-general:  A = X1 X2, B = Y1 Y2, C = d T1 T2, D = Z1 Z2, E = (X1 + Y1)(X2 + Y2) - A - B, F = D - C, G = D + C,
//     H = B - a A;  X3 = E F, Y3 = G H, T3 = E H, Z3 = F G - 9 products and the products by a and d.  Because a is a square and d is not it
//     is COMPLETE: no exceptional inputs, O and the points of small order included, and Z3 is never zero for points of the curve.
//   * doubling, dedicated:  A = X1^2, B = Y1^2, C = 2 Z1^2, D = a A, E = (X1 + Y1)^2 - A - B, G = D + B, F = G - C, H = D - B;  X3 = E F,
//     Y3 = G H, T3 = E H, Z3 = F G - 4 squarings, 4 products and the product by a.
//   * [k]P: one fixed-window chain over the 256 bits of the canonical integer k (fr_from_mont; the top two are zero), BJJ_MUL_WINDOW = 4 bits
//     a window: the table O, P, .. [15]P in private memory (14 additions), then 4 doublings and ONE addition per window whatever the digit -
//     the entry is picked by its address, the digit 0 adds O.  No data-dependent branch, every lane runs the same instruction stream.  Valid
//     for every point of the curve, cofactor components included, because the additions are the complete ones.
//   * affine outputs: one Fermat inversion of Z per lane (fr_pow_raw, fr_ops.hpp).
//   * validation: 1 a coordinate's words are not below r (compared as they stand), 4 not on the curve, 5 [l]P != O (the chain above over the
//     constant l), 0 otherwise; a rejected record is replaced by O in the arithmetic, never trusted.
//   * the challenge hm = Poseidon5(R8.x, R8.y, A.x, A.y, M): element 0 of the width-6 permutation of [0, ...] (poseidon_ops.hpp).
//   * verification (circomlib's verifyPoseidon): [S]B8 == R8 + [8 hm]A, the scalar the INTEGER 8 hm, no subgroup check.  One lane hashes,
//     forms A8 = [8]A with three doublings ([8 hm]A = [hm]([8]A) holds as integers, so off the subgroup too), and runs ONE joint doubling
//     chain (Straus) for [S]B8 + [hm](-A8) over 254 bits with a window of W = BN254_EDDSA_WINDOW bits per scalar: the table
//     [i]B8 + [j](-A8), i, j < 2^W, of 4^W entries in private memory, its B8 half the constants of babyjub_constants.hpp.  The result is
//     compared with R8 projectively (X == x_R Z, Y == y_R Z), without an inversion.
// Everything here is pure and takes plain pointers and a lane index (tests/hostsim/hostsim_babyjub.cpp runs the very same bodies over host arrays).
#pragma once
#include <stddef.h>
#include "poseidon_ops.hpp"
#include "fr_sqrt_ops.hpp"
#include "babyjub_constants.hpp"

// The joint window of the verifier, 1 or 2 bits per scalar.  The rule was fixed before measuring: the smaller median of five
// bn254_eddsa_poseidon_verify_batch_dev runs over 2^18 valid signatures in one process ships (tools/time_babyjub.py; profiles/r25_babyjub.txt);
// the other stays buildable: UNITS=bn254_babyjub tools/build_variant.sh eddsa_w1 -DBN254_EDDSA_WINDOW=1.
#ifndef BN254_EDDSA_WINDOW
#define BN254_EDDSA_WINDOW 2
#endif

namespace bn254 {

constexpr int BJJ_MUL_WINDOW = 4;                // bits per window of [k]P: a table of 16 points (2 KB of private memory per lane)
constexpr int BJJ_SCALAR_BITS = 256;             // the windows cover the whole eight words; a canonical scalar has no bit above 253
constexpr int BJJ_JOINT_BITS = 254;              // S < l < 2^251 and hm < r < 2^254

struct BjjExt { Fr x, y, z, t; };

BN_FN BjjExt bjj_identity() { return {fr_zero(), fr_one(), fr_one(), fr_zero()}; }
BN_FN BjjExt bjj_const(const uint32_t (*c)[8]) { return {fr_const(c[0]), fr_const(c[1]), fr_const(c[2]), fr_const(c[3])}; }
BN_FN BjjExt bjj_from_affine(const Fr &x, const Fr &y) { return {x, y, fr_one(), fr_mul(x, y)}; }
BN_FN BjjExt bjj_neg(const BjjExt &p) { return {fr_sub(fr_zero(), p.x), p.y, p.z, fr_sub(fr_zero(), p.t)}; }
BN_FN BjjExt bjj_select(bool take_b, const BjjExt &a, const BjjExt &b) {
    return {fr_select(take_b, a.x, b.x), fr_select(take_b, a.y, b.y), fr_select(take_b, a.z, b.z), fr_select(take_b, a.t, b.t)};
}
BN_FN BjjExt bjj_add(const BjjExt &p, const BjjExt &q) {
    const Fr a = fr_mul(p.x, q.x), b = fr_mul(p.y, q.y);
    const Fr c = fr_mul(fr_mul(p.t, q.t), fr_const(bjj::D_M)), d = fr_mul(p.z, q.z);
    const Fr e = fr_sub(fr_sub(fr_mul(fr_add(p.x, p.y), fr_add(q.x, q.y)), a), b);
    const Fr f = fr_sub(d, c), g = fr_add(d, c), h = fr_sub(b, fr_mul(a, fr_const(bjj::A_M)));
    return {fr_mul(e, f), fr_mul(g, h), fr_mul(f, g), fr_mul(e, h)};
}
BN_FN BjjExt bjj_double(const BjjExt &p) {
    const Fr a = fr_mul(p.x, p.x), b = fr_mul(p.y, p.y), zz = fr_mul(p.z, p.z);
    const Fr c = fr_add(zz, zz), d = fr_mul(a, fr_const(bjj::A_M));
    const Fr xy = fr_add(p.x, p.y);
    const Fr e = fr_sub(fr_sub(fr_mul(xy, xy), a), b);
    const Fr g = fr_add(d, b), f = fr_sub(g, c), h = fr_sub(d, b);
    return {fr_mul(e, f), fr_mul(g, h), fr_mul(f, g), fr_mul(e, h)};
}
// a x^2 + y^2 == 1 + d x^2 y^2
BN_FN bool bjj_on_curve(const Fr &x, const Fr &y) {
    const Fr xx = fr_mul(x, x), yy = fr_mul(y, y);
    const Fr lhs = fr_add(fr_mul(xx, fr_const(bjj::A_M)), yy);
    const Fr rhs = fr_add(fr_one(), fr_mul(fr_mul(xx, yy), fr_const(bjj::D_M)));
    return fr_eq(lhs, rhs);
}
// (X : Y : Z : T) == O: X == 0 and Y == Z (Z is never zero; (0 : -Z : Z : 0) is the point of order 2)
BN_FN bool bjj_is_identity(const BjjExt &p) { return fr_is_zero(p.x) & fr_eq(p.y, p.z); }
// x = X / Z, y = Y / Z with one Fermat inversion (Z != 0 for points of the curve; Z == 0 - garbage in - gives (0, 0), never a fault)
BN_FN void bjj_store_affine(const BjjExt &p, uint32_t *out, size_t i) {
    const Fr zi = fr_pow_raw<FR_POW_WINDOW>(p.z, fr_const(FR_MINUS_2_32));
    fr_store(fr_mul(p.x, zi), out, 2 * i);
    fr_store(fr_mul(p.y, zi), out, 2 * i + 1);
}

// [k]P for the 256-bit integer k (eight words, least significant first) and any point of the curve.  Out of line with P by reference: one
// copy of the chain serves bn254_bjj_mul_batch and the [l]P of the validation, and its 2 KB table is the callee's own frame
BN_OUTER void bjj_mul_chain(const BjjExt &p, const Fr &k, BjjExt &out) {
    constexpr int T = 1 << BJJ_MUL_WINDOW, NW = BJJ_SCALAR_BITS / BJJ_MUL_WINDOW;
    BjjExt tbl[T];
    tbl[0] = bjj_identity();
    tbl[1] = p;
#pragma unroll 1
    for (int i = 2; i < T; ++i) tbl[i] = bjj_add(tbl[i - 1], p);
    BjjExt acc = tbl[fr_digit<BJJ_MUL_WINDOW>(k, NW - 1)];
#pragma unroll 1
    for (int b = (NW - 1) * BJJ_MUL_WINDOW - 1; b >= 0; --b) {
        acc = bjj_double(acc);
        if (b % BJJ_MUL_WINDOW == 0) acc = bjj_add(acc, tbl[fr_digit<BJJ_MUL_WINDOW>(k, b / BJJ_MUL_WINDOW)]);      // uniform: the loop counter decides
    }
    out = acc;
}

// [s]B8 + [h]NA for the integers s, h < 2^254 and any point NA of the curve: one joint chain, W bits of each scalar per window
template <int W>
BN_OUTER void bjj_joint_chain(const BjjExt &na, const Fr &s, const Fr &h, BjjExt &out) {
    static_assert(W == 1 || W == 2, "the table has 4^W entries; the constants hold [0 .. 3]B8");
    constexpr int D = 1 << W, NW = (BJJ_JOINT_BITS + W - 1) / W;
    BjjExt tbl[D * D];                                                            // tbl[D i + j] = [i]B8 + [j]NA
    tbl[0] = bjj_identity();
    tbl[1] = na;
    if constexpr (W == 2) { tbl[2] = bjj_double(na); tbl[3] = bjj_add(tbl[2], na); }
#pragma unroll 1
    for (int i = D; i < D * D; ++i) tbl[i] = bjj_add(bjj_const(bjj::B8_MUL[i / D]), tbl[i % D]);
    BjjExt acc = tbl[D * fr_digit<W>(s, NW - 1) + fr_digit<W>(h, NW - 1)];
#pragma unroll 1
    for (int b = (NW - 1) * W - 1; b >= 0; --b) {
        acc = bjj_double(acc);
        if (b % W == 0) acc = bjj_add(acc, tbl[D * fr_digit<W>(s, b / W) + fr_digit<W>(h, b / W)]);
    }
    out = acc;
}

// the 256-bit integer a is below the 256-bit integer b (eight words each, least significant first)
BN_FN bool bjj_lt(const uint32_t *a, const uint32_t *b) {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int64_t v = (int64_t)a[i] - (int64_t)b[i] + br; br = v >> 32; }
    return br != 0;
}
// hm: element 0 of the width-6 permutation of [0, r8.x, r8.y, a.x, a.y, m]
BN_FN Fr eddsa_challenge(const Fr &ax, const Fr &ay, const Fr &rx, const Fr &ry, const Fr &m) {
    Fr s[6] = {fr_zero(), rx, ry, ax, ay, m};
    fr_poseidon_permute<6>(s);
    return s[0];
}

// ---- the bodies: record i of a launch
BN_FN void bjj_validate_body(const uint32_t *p, int32_t *status, size_t i) {
    Fr x = fr_load(p, 2 * i), y = fr_load(p, 2 * i + 1);
    const bool in_range = fr_lt_r(x.w) & fr_lt_r(y.w);
    x = fr_select(in_range, fr_zero(), x); y = fr_select(in_range, fr_one(), y);
    const bool on_curve = bjj_on_curve(x, y);
    x = fr_select(on_curve, fr_zero(), x); y = fr_select(on_curve, fr_one(), y);
    const BjjExt pt = bjj_from_affine(x, y);
    BjjExt lp;
    bjj_mul_chain(pt, fr_const(bjj::L_RAW), lp);
    status[i] = !in_range ? 1 : !on_curve ? 4 : !bjj_is_identity(lp) ? 5 : 0;
}
// out may be p or q: the lane reads its two records before it writes its one and touches no other lane's
BN_FN void bjj_add_body(const uint32_t *p, const uint32_t *q, uint32_t *out, size_t i) {
    const BjjExt a = bjj_from_affine(fr_load(p, 2 * i), fr_load(p, 2 * i + 1)), b = bjj_from_affine(fr_load(q, 2 * i), fr_load(q, 2 * i + 1));
    bjj_store_affine(bjj_add(a, b), out, i);
}
// out may be p
BN_FN void bjj_mul_body(const uint32_t *p, const uint32_t *k, uint32_t *out, size_t i) {
    const BjjExt pt = bjj_from_affine(fr_load(p, 2 * i), fr_load(p, 2 * i + 1));
    const Fr kr = fr_raw(fr_load(k, i));
    BjjExt r;
    bjj_mul_chain(pt, kr, r);
    bjj_store_affine(r, out, i);
}
BN_FN void eddsa_challenge_body(const uint32_t *a, const uint32_t *r8, const uint32_t *msg, uint32_t *out, size_t i) {
    fr_store(eddsa_challenge(fr_load(a, 2 * i), fr_load(a, 2 * i + 1), fr_load(r8, 2 * i), fr_load(r8, 2 * i + 1), fr_load(msg, i)), out, i);
}
// statuses in the order of the checks: 1 range (a word array of a, r8, s or msg is not below r, or the integer of s is not below l), 4 R8 or A
// is not on the curve, 6 the equation fails, 0 valid.  A row that fails a check computes on O and zeros from there on: every lane runs the
// whole chain, every case is a select
// the core both verifiers share, on inputs that passed (or were replaced by O and zeros after) every check: hash, [8]A, the joint chain, the
// projective comparison.  sr is the integer S, m a Montgomery image
template <int W>
BN_FN bool eddsa_verify_core(const Fr &ax, const Fr &ay, const Fr &rx, const Fr &ry, const Fr &sr, const Fr &m) {
    const Fr hr = fr_raw(eddsa_challenge(ax, ay, rx, ry, m));
    const BjjExt na8 = bjj_neg(bjj_double(bjj_double(bjj_double(bjj_from_affine(ax, ay)))));
    BjjExt v;
    bjj_joint_chain<W>(na8, sr, hr, v);                                           // [S]B8 - [hm][8]A, to be R8
    return fr_eq(v.x, fr_mul(rx, v.z)) & fr_eq(v.y, fr_mul(ry, v.z));
}
template <int W>
BN_FN void eddsa_verify_body(const uint32_t *a, const uint32_t *r8, const uint32_t *s, const uint32_t *msg, int32_t *status, size_t i) {
    Fr ax = fr_load(a, 2 * i), ay = fr_load(a, 2 * i + 1), rx = fr_load(r8, 2 * i), ry = fr_load(r8, 2 * i + 1), sm = fr_load(s, i), m = fr_load(msg, i);
    const bool words_ok = fr_lt_r(ax.w) & fr_lt_r(ay.w) & fr_lt_r(rx.w) & fr_lt_r(ry.w) & fr_lt_r(sm.w) & fr_lt_r(m.w);
    sm = fr_select(words_ok, fr_zero(), sm);
    Fr sr = fr_raw(sm);
    const bool in_range = words_ok & bjj_lt(sr.w, bjj::L_RAW);
    sr = fr_select(in_range, fr_zero(), sr); m = fr_select(in_range, fr_zero(), m);
    ax = fr_select(in_range, fr_zero(), ax); ay = fr_select(in_range, fr_one(), ay);
    rx = fr_select(in_range, fr_zero(), rx); ry = fr_select(in_range, fr_one(), ry);
    const bool on_curve = bjj_on_curve(rx, ry) & bjj_on_curve(ax, ay);
    ax = fr_select(on_curve, fr_zero(), ax); ay = fr_select(on_curve, fr_one(), ay);
    rx = fr_select(on_curve, fr_zero(), rx); ry = fr_select(on_curve, fr_one(), ry);
    const bool eq = eddsa_verify_core<W>(ax, ay, rx, ry, sr, m);
    status[i] = !in_range ? 1 : !on_curve ? 4 : !eq ? 6 : 0;
}

// ---- packed points (circomlib's packPoint): 32 bytes, the canonical integer of y little endian, bit 7 of byte 31 set iff the canonical
// integer of x is above (r - 1) / 2.  On a little-endian device the record is the eight words of that integer
BN_FN void bjj_pack_body(const uint32_t *p, uint32_t *out32, size_t i) {
    const Fr xr = fr_raw(fr_load(p, 2 * i));
    Fr yr = fr_raw(fr_load(p, 2 * i + 1));
    yr.w[7] |= fr_raw_above_half(xr) ? 0x80000000u : 0u;
    fr_store(yr, out32, i);
}
// what a record holds: in_range the integer of y (the sign bit cleared) is below r; has_x some point has this y:
// x^2 = (1 - y^2) / (a - d y^2) is a square (the denominator is never zero: a / d is a non-residue); canonical not (x == 0 and the sign bit
// set).  (x, y) is the point when all three hold and O = (0, 1) otherwise.  The flags are computed in that order, each on O once one failed
struct BjjUnpacked { Fr x, y; bool in_range, has_x, canonical; };
template <int FORM>
BN_FN BjjUnpacked bjj_unpack_point(Fr rec) {
    BjjUnpacked o;
    const bool sign = (rec.w[7] >> 31) != 0;
    rec.w[7] &= 0x7fffffffu;
    o.in_range = fr_lt_r(rec.w);
    const Fr y = fr_select(o.in_range, fr_one(), fr_mul(rec, fr_const(k::FR_R2_32)));        // R^2 is the canonical operand
    const Fr yy = fr_mul(y, y);
    FrSqrt r;
    fr_sqrt_ratio<FORM>(fr_sub(fr_one(), yy), fr_sub(fr_const(bjj::A_M), fr_mul(yy, fr_const(bjj::D_M))), r);
    o.has_x = r.is_square;
    o.canonical = !(fr_is_zero(r.root) & sign);
    const bool ok = o.in_range & o.has_x & o.canonical;
    o.x = fr_select(ok, fr_zero(), fr_select(sign, r.root, fr_sub(fr_zero(), r.root)));
    o.y = fr_select(ok, fr_one(), y);
    return o;
}
// statuses in the order of the checks: 1 range, 4 no point has this y, 3 a non-canonical sign, 0 otherwise; a rejected record is O.
// out may not be in32 (the records differ in size)
template <int FORM>
BN_FN void bjj_unpack_body(const uint32_t *in32, uint32_t *out, int32_t *status, size_t i) {
    const BjjUnpacked u = bjj_unpack_point<FORM>(fr_load(in32, i));
    fr_store(u.x, out, 2 * i);
    fr_store(u.y, out, 2 * i + 1);
    status[i] = !u.in_range ? 1 : !u.has_x ? 4 : !u.canonical ? 3 : 0;
}
// The verifier on the wire bytes: a32 the packed key, sig64 the packed R8 followed by the integer S as 32 little-endian bytes (its top bit
// is no flag), msg as in eddsa_verify_body.  Statuses in the order of the checks: 1 a y, S or msg out of range, 4 a point has no x, 3 a
// non-canonical sign in either point, 6 the equation fails, 0 valid.  A row that fails computes on O and zeros from there on
template <int W, int FORM>
BN_FN void eddsa_verify_packed_body(const uint32_t *a32, const uint32_t *sig64, const uint32_t *msg, int32_t *status, size_t i) {
    const BjjUnpacked a = bjj_unpack_point<FORM>(fr_load(a32, i)), r8 = bjj_unpack_point<FORM>(fr_load(sig64, 2 * i));
    Fr sr = fr_load(sig64, 2 * i + 1), m = fr_load(msg, i);
    const bool in_range = a.in_range & r8.in_range & bjj_lt(sr.w, bjj::L_RAW) & fr_lt_r(m.w);
    const bool has_x = a.has_x & r8.has_x, canonical = a.canonical & r8.canonical, ok = in_range & has_x & canonical;
    sr = fr_select(ok, fr_zero(), sr); m = fr_select(ok, fr_zero(), m);
    const Fr ax = fr_select(ok, fr_zero(), a.x), ay = fr_select(ok, fr_one(), a.y), rx = fr_select(ok, fr_zero(), r8.x), ry = fr_select(ok, fr_one(), r8.y);
    const bool eq = eddsa_verify_core<W>(ax, ay, rx, ry, sr, m);
    status[i] = !in_range ? 1 : !has_x ? 4 : !canonical ? 3 : !eq ? 6 : 0;
}

}  // namespace bn254
