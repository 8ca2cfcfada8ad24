// Square roots in Fr (include/bn254_hip.h bn254_fr_sqrt_batch in bn254_fr_sqrt.hip, and the point unpacking of babyjub_ops.hpp):
// fr_sqrt_ratio, the root of u / v without an inversion.  r - 1 = 2^s t with s = 28 and t odd (226 bits), so the single exponentiation of sqrt_ops.hpp (q = 3 mod 4) does not
// apply, and the textbook Tonelli-Shanks loops on the data, which a lane must not: here every lane runs the same instruction stream, every
// case is a fr_select and every loop bound a constant.  c = 5^t generates the subgroup of order 2^s (5 is a non-residue).
//   * the ratio:  V = v^(2^s - 1),  W = (u V^2 v)^((t-1)/2) V = u^((t-1)/2) v^(-(t+1)/2)  (the exponent of v is 2^s t - (t+1)/2 = r - 1 - (t+1)/2).
//     With a = u / v:  w = W v = a^((t-1)/2),  x = W u = a^((t+1)/2),  b = x w = a^t,  so x^2 = a b and b lies in the subgroup of order 2^s.
//     Only (.)^((t-1)/2) is long: 225 bits, a fixed 4-bit window with its table in private memory (14 products), 56 windows of 4 squarings and a
//     product where the digit is not zero.  The exponent is a constant: its digits drive uniform branches.
//   * the correction of x by a power of c, in two forms behind one compile switch BN254_FR_SQRT_FORM (both templates: the host simulation
//     runs the two whichever ships):
//       0  constant-flow Tonelli-Shanks: z = x, tt = b, cc = c; for i = s .. 2: e = (tt^(2^(i-2)) == 1), z = e ? z : z cc, cc = cc^2,
//          tt = e ? tt : tt cc.  A square ends with tt == 1.  351 squarings and 81 products.
//       1  the logarithm of b to base c, 7 digits of 4 bits, least significant first: with g = c^(-(digits so far)), (b g)^(2^(24 - 4 j)) lies in
//          the subgroup of order 16 and equals ROOT16_M[digit j]; g and the root's factor h = c^(-(digits so far) / 2) are updated from two
//          constant tables picked by address.  A square has an even logarithm e, and the root is x c^(-e/2).  84 squarings, 22 products and
//          7 x 15 compares.
//   * u == 0 gives (0, true) by a select; a non-square gives root 0; the root returned is the one whose canonical integer is not above
//     (r - 1) / 2.  v == 0 is outside the contract: some value comes out, never a fault.
// Everything here is pure (tests/hostsim/hostsim_bjj_pack.cpp runs the very same bodies over host arrays).
#pragma once
#include <stddef.h>
#include "fr_ops.hpp"
#include "fr_sqrt_constants.hpp"

// The rule was fixed before measuring: the smaller median of five bn254_bjj_unpack_batch_dev runs over 2^20 valid packed points in one process
// ships (tools/time_bjj_pack.py; profiles/r26_bjj_pack.txt: form 1 took 5.4573 ms against 8.8567 ms for form 0); the other stays buildable:
// UNITS="bn254_fr_sqrt bn254_babyjub" tools/build_variant.sh fr_sqrt_form0 -DBN254_FR_SQRT_FORM=0.
#ifndef BN254_FR_SQRT_FORM
#define BN254_FR_SQRT_FORM 1
#endif

namespace bn254 {

struct FrSqrt { Fr root; bool is_square; };

// the 256-bit integer a (eight words) is above (r - 1) / 2
BN_FN bool fr_raw_above_half(const Fr &a) {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int64_t v = (int64_t)frsqrt::HALF_RAW[i] - (int64_t)a.w[i] + br; br = v >> 32; }
    return br != 0;
}
// a^((t-1)/2)
BN_FN Fr fr_sqrt_chain(const Fr &a) {
    constexpr int NW = (frsqrt::EXP_BITS + 3) / 4;
    Fr tab[16];
    tab[0] = fr_one(); tab[1] = a;
#pragma unroll 1
    for (int i = 2; i < 16; ++i) tab[i] = fr_mul(tab[i - 1], a);
    Fr r = tab[(frsqrt::EXP_RAW[(4 * (NW - 1)) >> 5] >> ((4 * (NW - 1)) & 31)) & 15u];
#pragma unroll 1
    for (int w = NW - 2; w >= 0; --w) {
        r = fr_mul(r, r); r = fr_mul(r, r); r = fr_mul(r, r); r = fr_mul(r, r);
        const uint32_t d = (frsqrt::EXP_RAW[(4 * w) >> 5] >> ((4 * w) & 31)) & 15u;       // uniform: a constant's digit
        if (d) r = fr_mul(r, tab[d]);
    }
    return r;
}
// x = a^((t+1)/2) and b = a^t -> x c^k with (x c^k)^2 == a, and whether there is one
template <int FORM>
BN_FN FrSqrt fr_sqrt_correct(const Fr &x, const Fr &b) {
    static_assert(FORM == 0 || FORM == 1, "two forms");
    const Fr one = fr_one();
    if constexpr (FORM == 0) {
        Fr z = x, tt = b, cc = fr_const(frsqrt::C_M);
#pragma unroll 1
        for (int i = frsqrt::TWO_ADICITY; i >= 2; --i) {
            Fr bb = tt;
#pragma unroll 1
            for (int j = 0; j < i - 2; ++j) bb = fr_mul(bb, bb);
            const bool e = fr_eq(bb, one);
            z = fr_select(e, fr_mul(z, cc), z);
            cc = fr_mul(cc, cc);
            tt = fr_select(e, fr_mul(tt, cc), tt);
        }
        return {z, fr_eq(tt, one)};
    } else {
        Fr g = one, h = one;
        uint32_t odd = 0;
#pragma unroll 1
        for (int j = 0; j < 7; ++j) {
            Fr y = fr_mul(b, g);
#pragma unroll 1
            for (int q = 0; q < 24 - 4 * j; ++q) y = fr_mul(y, y);
            uint32_t d = 0;                                                        // y == 1, or (u == 0) nothing matches
#pragma unroll 1
            for (uint32_t k = 1; k < 16; ++k) d = fr_eq(y, fr_const(frsqrt::ROOT16_M[k])) ? k : d;
            if (j == 0) odd = d & 1u;
            g = fr_mul(g, fr_const(frsqrt::NEG_M[j][d]));
            h = fr_mul(h, fr_const(frsqrt::NEG_HALF_M[j][d]));
        }
        return {fr_mul(x, h), odd == 0};
    }
}
// (root, is_square) with root^2 == u / v for canonical Montgomery u and v != 0.  Out of line, operands by reference: one copy serves every
// caller of a kernel, and the chain's table is the callee's own frame
template <int FORM = BN254_FR_SQRT_FORM>
BN_OUTER void fr_sqrt_ratio(const Fr &u, const Fr &v, FrSqrt &out) {
    Fr V = v;
#pragma unroll 1
    for (int i = 1; i < frsqrt::TWO_ADICITY; ++i) V = fr_mul(fr_mul(V, V), v);        // v^(2^s - 1)
    const Fr W = fr_mul(fr_sqrt_chain(fr_mul(fr_mul(fr_mul(V, V), u), v)), V);
    const Fr x = fr_mul(W, u);
    FrSqrt r = fr_sqrt_correct<FORM>(x, fr_mul(x, fr_mul(W, v)));
    r.is_square |= fr_is_zero(u);
    r.root = fr_select(r.is_square, fr_zero(), r.root);
    r.root = fr_select(fr_raw_above_half(fr_raw(r.root)), r.root, fr_sub(fr_zero(), r.root));
    out = r;
}

// ---- the body: element i of a launch.  Option<Fr>: ok = 1 and the smaller root, or ok = 0 and zero; ok may be NULL, out may be a
template <int FORM>
BN_FN void fr_sqrt_body(const uint32_t *a, uint32_t *out, int32_t *ok, size_t i) {
    FrSqrt r;
    fr_sqrt_ratio<FORM>(fr_load(a, i), fr_one(), r);
    fr_store(r.root, out, i);
    if (ok) ok[i] = r.is_square ? 1 : 0;
}

}  // namespace bn254
