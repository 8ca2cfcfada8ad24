// Grumpkin on the device (include/bn254_hip.h bn254_grumpkin_{validate,add,mul,msm}_batch): the per-lane bodies.  The curve is y^2 = x^3 - 17 over
// Fr, the other half of the BN254 cycle: its order is q, the base field modulus of BN254, a prime - the cofactor is 1.  Like Baby Jubjub it is a
// group over fr.hpp: everything goes through fr_mul / fr_add / fr_sub on canonical values - fr_mul's precondition holds everywhere and the bytes
// are those of the integer model.
//   * a point in memory: two consecutive Fr, x then y, Montgomery words, affine, 64 bytes.  Infinity is (0, 0): -17 is a non-residue mod r, so
//     no point of the curve has x = 0 and (0, 0) is free.
//   * a point in a lane: homogeneous projective (X : Y : Z), x = X / Z, y = Y / Z, O = (0 : 1 : 0).  A load maps (0, 0) to (0 : 1 : 0).  A store
//     runs one Fermat inversion of Z (fr_pow_raw by r - 2), which gives 0 for Z = 0: O comes out as (0, 0) without a branch.
//   * a scalar: 32 bytes, the little-endian integer k, any value below 2^256 - NOT a Montgomery image (the scalar field is Fq, which has no type
//     here).  The result is [k]P for that integer, which is [k mod q]P.
//   * the group law: the complete formulas of Renes-Costello-Batina 2016 for a = 0 with b3 = 3 b = -51 (a Montgomery constant, a full fr_mul).
//     Addition (algorithm 7):  t0 = X1 X2, t1 = Y1 Y2, t2 = Z1 Z2, t3 = (X1 + Y1)(X2 + Y2) - t0 - t1, t4 = (Y1 + Z1)(Y2 + Z2) - t1 - t2,
//     t5 = (X1 + Z1)(X2 + Z2) - t0 - t2, x3 = 3 t0, u = b3 t2, z3 = t1 + u, w = t1 - u, y3 = b3 t5;  X3 = t3 w - t4 y3, Y3 = w z3 + y3 x3,
//     Z3 = z3 t4 + x3 t3 - 12 products and 2 by b3.  No exceptional inputs: P + P, P + O, O + O and P + (-P) included (the order is odd).
//     Doubling (algorithm 9):  t0 = Y^2, z8 = 8 t0, t1 = Y Z, t2 = b3 Z^2;  X3' = t2 z8, Y3' = t0 + t2, Z3 = t1 z8, t0' = t0 - 3 t2;
//     Y3 = X3' + t0' Y3', X3 = 2 t0' (X Y) - 6 products, 2 squarings and 1 by b3.
//   * [k]P: one fixed-window chain over the 256 bits of k, GRK_MUL_WINDOW = 4 bits a window (BN254_GRUMPKIN_MUL_WINDOW; 5 is buildable): the
//     table O, P, .. [15]P in private memory (14 additions), then 4 doublings and ONE addition per window whatever the digit - the entry is
//     picked by its address, the digit 0 adds O.  No data-dependent branch, every lane runs the same instruction stream.
//   * validation: 1 a coordinate's words are not below r (compared as they stand), 4 not on the curve ((0, 0) excepted), 0 otherwise.  There
//     is no subgroup status: the cofactor is 1.  The arithmetic bodies trust their caller: an off-curve point gives garbage, never a fault.
//   * the segmented sum (bn254_grumpkin_msm_batch): the work list of host_plan.hpp's bn_dot_plan(offsets, m, 1, GRK_MSM_FAN).  Level 0: a lane owns
//     one term (or an empty segment), runs the chain and either normalises into out[j] - a segment of at most one term - or stores (X, Y, Z),
//     96 bytes, to its scratch slot.  A fold level: a lane adds its at most GRK_MSM_FAN slots with the complete addition; the piece that completes a
//     segment normalises and stores out[j].  No slot is written twice.
// Everything here is pure and takes plain pointers and a lane index (tests/hostsim/hostsim_grumpkin.cpp runs the very same bodies over host arrays).
#pragma once
#include <stddef.h>
#include "fr_ops.hpp"
#include "io.hpp"
#include "grumpkin_constants.hpp"

// The window of [k]P, 4 or 5 bits.  The rule was fixed before measuring: 4 stays unless the [min, max] of five bn254_grumpkin_mul_batch_dev runs
// at 2^20 with a window of 5 lies wholly below, at zero spilled VGPRs (tools/time_grumpkin.py --variants; profiles/r30_grumpkin.txt); the
// other stays buildable: UNITS=bn254_grumpkin tools/build_variant.sh grk_w5 -DBN254_GRUMPKIN_MUL_WINDOW=5.
#ifndef BN254_GRUMPKIN_MUL_WINDOW
#define BN254_GRUMPKIN_MUL_WINDOW 4
#endif

namespace bn254 {

constexpr int GRK_MUL_WINDOW = BN254_GRUMPKIN_MUL_WINDOW;    // bits per window of [k]P: a table of 16 points (1.5 KB of private memory per lane)
static_assert(GRK_MUL_WINDOW == 4 || GRK_MUL_WINDOW == 5, "a table of 16 or 32 points");
constexpr int GRK_SCALAR_BITS = 256;             // the windows cover the whole eight words
constexpr uint32_t GRK_MSM_FAN = 16;             // slots per lane of a fold level of the segmented sum

struct GrkPt { Fr x, y, z; };

BN_FN GrkPt grk_identity() { return {fr_zero(), fr_one(), fr_zero()}; }
// (0, 0) -> (0 : 1 : 0), every other pair -> (x : y : 1)
BN_FN GrkPt grk_from_affine(const Fr &x, const Fr &y) {
    const bool inf = fr_is_zero(x) & fr_is_zero(y);
    return {x, fr_select(inf, y, fr_one()), fr_select(inf, fr_one(), fr_zero())};
}
BN_FN GrkPt grk_load_affine(const uint32_t *p, size_t i) { return grk_from_affine(fr_load(p, 2 * i), fr_load(p, 2 * i + 1)); }
BN_FN GrkPt grk_add(const GrkPt &p, const GrkPt &q) {
    const Fr b3 = fr_const(grk::B3_M);
    const Fr t0 = fr_mul(p.x, q.x), t1 = fr_mul(p.y, q.y), t2 = fr_mul(p.z, q.z);
    const Fr t3 = fr_sub(fr_sub(fr_mul(fr_add(p.x, p.y), fr_add(q.x, q.y)), t0), t1);
    const Fr t4 = fr_sub(fr_sub(fr_mul(fr_add(p.y, p.z), fr_add(q.y, q.z)), t1), t2);
    const Fr t5 = fr_sub(fr_sub(fr_mul(fr_add(p.x, p.z), fr_add(q.x, q.z)), t0), t2);
    const Fr x3 = fr_add(fr_add(t0, t0), t0), u = fr_mul(t2, b3);
    const Fr z3 = fr_add(t1, u), w = fr_sub(t1, u), y3 = fr_mul(t5, b3);
    return {fr_sub(fr_mul(t3, w), fr_mul(t4, y3)), fr_add(fr_mul(w, z3), fr_mul(y3, x3)), fr_add(fr_mul(z3, t4), fr_mul(x3, t3))};
}
BN_FN GrkPt grk_double(const GrkPt &p) {
    const Fr t0 = fr_mul(p.y, p.y);
    Fr z8 = fr_add(t0, t0); z8 = fr_add(z8, z8); z8 = fr_add(z8, z8);
    const Fr t1 = fr_mul(p.y, p.z), t2 = fr_mul(fr_mul(p.z, p.z), fr_const(grk::B3_M));
    const Fr xa = fr_mul(t2, z8), ya = fr_add(t0, t2), z3 = fr_mul(t1, z8);
    const Fr t0b = fr_sub(t0, fr_add(fr_add(t2, t2), t2));
    const Fr y3 = fr_add(xa, fr_mul(t0b, ya));
    const Fr xh = fr_mul(t0b, fr_mul(p.x, p.y));
    return {fr_add(xh, xh), y3, z3};
}
// y^2 == x^3 + b
BN_FN bool grk_on_curve(const Fr &x, const Fr &y) {
    return fr_eq(fr_mul(y, y), fr_add(fr_mul(fr_mul(x, x), x), fr_const(grk::B_M)));
}
// (X1 : Y1 : Z1) == (X2 : Y2 : Z2) as points: the cross products agree (both are points, so neither is (0 : 0 : 0))
BN_FN bool grk_eq(const GrkPt &p, const GrkPt &q) {
    return fr_eq(fr_mul(p.x, q.y), fr_mul(q.x, p.y)) & fr_eq(fr_mul(p.x, q.z), fr_mul(q.x, p.z)) & fr_eq(fr_mul(p.y, q.z), fr_mul(q.y, p.z));
}
// x = X / Z, y = Y / Z with one Fermat inversion; Z == 0 - O - gives (0, 0)
BN_FN void grk_store_affine(const GrkPt &p, uint32_t *out, size_t i) {
    const Fr zi = fr_pow_raw<FR_POW_WINDOW>(p.z, fr_const(FR_MINUS_2_32));
    fr_store(fr_mul(p.x, zi), out, 2 * i);
    fr_store(fr_mul(p.y, zi), out, 2 * i + 1);
}
// a scratch slot of the segmented sum: (X, Y, Z), three consecutive records of 32 bytes
BN_FN GrkPt grk_load_slot(const uint32_t *part, size_t i) { return {fr_load(part, 3 * i), fr_load(part, 3 * i + 1), fr_load(part, 3 * i + 2)}; }
BN_FN void grk_store_slot(const GrkPt &p, uint32_t *part, size_t i) {
    fr_store(p.x, part, 3 * i); fr_store(p.y, part, 3 * i + 1); fr_store(p.z, part, 3 * i + 2);
}

// digit w (WB bits) of the integer e; a width that does not divide 32 reads across two words (the word above the eighth is zero)
template <int WB>
BN_FN uint32_t grk_digit(const Fr &e, int w) {
    if constexpr (32 % WB == 0) return fr_digit<WB>(e, w);
    const int bit = w * WB;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { lo = (bit >> 5) == i ? e.w[i] : lo; hi = (bit >> 5) + 1 == i ? e.w[i] : hi; }
    return (uint32_t)((((uint64_t)hi << 32 | lo) >> (bit & 31)) & ((1u << WB) - 1u));
}
// [k]P for the 256-bit integer k (eight words, least significant first).  Out of line with P by reference: one copy of the chain serves
// bn254_grumpkin_mul_batch and level 0 of the segmented sum, and its 1.5 KB table is the callee's own frame
BN_OUTER void grk_mul_chain(const GrkPt &p, const Fr &k, GrkPt &out) {
    constexpr int T = 1 << GRK_MUL_WINDOW, NW = (GRK_SCALAR_BITS + GRK_MUL_WINDOW - 1) / GRK_MUL_WINDOW;
    GrkPt tbl[T];
    tbl[0] = grk_identity();
    tbl[1] = p;
#pragma unroll 1
    for (int i = 2; i < T; ++i) tbl[i] = grk_add(tbl[i - 1], p);
    GrkPt acc = tbl[grk_digit<GRK_MUL_WINDOW>(k, NW - 1)];
#pragma unroll 1
    for (int b = (NW - 1) * GRK_MUL_WINDOW - 1; b >= 0; --b) {
        acc = grk_double(acc);
        if (b % GRK_MUL_WINDOW == 0) acc = grk_add(acc, tbl[grk_digit<GRK_MUL_WINDOW>(k, b / GRK_MUL_WINDOW)]);      // uniform: the loop counter decides
    }
    out = acc;
}

// ---- the bodies: record i of a launch
// a record out of range is replaced by (0, 0) before any arithmetic, so every product has a canonical operand
BN_FN void grk_validate_body(const uint32_t *p, int32_t *status, size_t i) {
    Fr x = fr_load(p, 2 * i), y = fr_load(p, 2 * i + 1);
    const bool in_range = fr_lt_r(x.w) & fr_lt_r(y.w);
    x = fr_select(in_range, fr_zero(), x); y = fr_select(in_range, fr_zero(), y);
    const bool on_curve = grk_on_curve(x, y) | (fr_is_zero(x) & fr_is_zero(y));
    status[i] = !in_range ? 1 : !on_curve ? 4 : 0;
}
// out may be p or q: the lane reads its two records before it writes its one and touches no other lane's
BN_FN void grk_add_body(const uint32_t *p, const uint32_t *q, uint32_t *out, size_t i) {
    const GrkPt a = grk_load_affine(p, i), b = grk_load_affine(q, i);
    grk_store_affine(grk_add(a, b), out, i);
}
// out may be p
BN_FN void grk_mul_body(const uint32_t *p, const uint32_t *k, uint32_t *out, size_t i) {
    const GrkPt pt = grk_load_affine(p, i);
    const Fr kr = fr_load(k, i);
    GrkPt r;
    grk_mul_chain(pt, kr, r);
    grk_store_affine(r, out, i);
}
// piece `lane` of level 0 of the segmented sum: its one term [k]P, or O for a piece of no terms (an empty segment)
BN_FN void grk_msm_piece_body(const uint32_t *p, const uint32_t *k, const BnDotPiece *list, uint32_t *part, uint32_t *out, size_t lane) {
    const BnDotPiece pc = list[lane];
    const uint64_t first = dot_piece_first(pc);
    GrkPt acc = grk_identity();
    if (dot_piece_len(pc)) {
        const GrkPt pt = grk_load_affine(p, first);
        const Fr kr = fr_load(k, first);
        grk_mul_chain(pt, kr, acc);
    }
    if (dot_piece_to_out(pc)) grk_store_affine(acc, out, pc.dst);
    else grk_store_slot(acc, part, pc.dst);
}
// piece `lane` of a fold level: the sum of its slots (complete additions only).  A level reads slots only earlier levels wrote and writes slots
// of its own, so the lanes of one launch never meet.
BN_FN void grk_msm_fold_body(const BnDotPiece *list, uint32_t *part, uint32_t *out, size_t lane) {
    const BnDotPiece pc = list[lane];
    const uint64_t first = dot_piece_first(pc);
    const uint32_t len = dot_piece_len(pc);
    GrkPt acc = grk_identity();
#pragma unroll 1
    for (uint32_t j = 0; j < len; ++j) acc = grk_add(acc, grk_load_slot(part, first + j));
    if (dot_piece_to_out(pc)) grk_store_affine(acc, out, pc.dst);
    else grk_store_slot(acc, part, pc.dst);
}

}  // namespace bn254
