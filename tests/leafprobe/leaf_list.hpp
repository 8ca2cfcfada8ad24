// TEST INFRASTRUCTURE - the leaves of bn_amd/csrc/fe.hpp that run as inline-asm chains on the GPU, as ONE list read by the CPU twins
// (tests/hostsim/hostsim_leaf.cpp) and by the GPU probe (bn254_leafprobe.hip), so that both call the same expression on the same operands.
//
//   LEAF(id, name, output limbs, operand kinds, expression)
//   LEAF_HOST(id, name, output limbs, operand kinds, host statement, expression)      the CPU twin runs the statement, the GPU the expression
//
// operand kinds: one character per operand, 'f' = Fe (9 limbs), 'w' = FeW (18 limbs).  Inside the expression F(i) / W(i) is operand i and FLAG
// the per-case boolean (fe_wred's `neg`, the fused reductions' `neg2`).  The includer defines LEAF, LEAF_HOST, F, W and FLAG.
// tests/leaf_cases.py holds the same ids, names and kinds (the tests compare them with what the two libraries export).
//
// The fused reductions: fe_lc4_core picks one of nine asm chains (BN_LC_CHAIN in fe.hpp) by NWIDE - the terms that enter the 64-bit chain on
// their own - and by whether a 32-bit "narrow" sum exists.  The branch of every entry is written next to it as (NWIDE, N) or (NWIDE, -).
// (4, N) cannot be instantiated: four wide terms leave no operand for a narrow sum, the `t += nsum` of that branch is dead code.
// Three branches are reached by no instantiation of the product and have an invented entry: (0, -), (3, N), and (2, N) outside the SIGN2 form.
// clang-format off
LEAF( 0, fe_mul,       9, "ff",           (fe_mul(F(0), F(1))))
LEAF( 1, fe_sqr,       9, "f",            (fe_sqr(F(0))))
LEAF( 2, fe_mul2,      9, "ffff",         (fe_mul2(F(0), F(1), F(2), F(3))))
LEAF( 3, fe_mul2s,     9, "ffff",         (fe_mul2s(F(0), F(1), F(2), F(3))))
LEAF( 4, fe_mul6,      9, "ffffffffffff", (fe_mul6(F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), F(8), F(9), F(10), F(11))))
LEAF( 5, fe_mul5,      9, "ffffffffff",   (fe_mul5(F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), F(8), F(9))))
LEAF_HOST( 6, fe_wmul2,  18, "ffff", raw_wmul2(0, P(0), P(1), P(2), P(3), B2, O), (fe_wmul2(F(0), F(1), F(2), F(3))))
LEAF_HOST( 7, fe_wmul2s, 18, "ffff", raw_wmul2(1, P(0), P(1), P(2), P(3), B2, O), (fe_wmul2s(F(0), F(1), F(2), F(3))))
LEAF_HOST( 8, fe_wred_ff, 9, "wwwf", raw_wred(0, 0, P(0), P(1), P(2), FLAG, P(3), B2, O), (fe_wred<false, false>(W(0), W(1), W(2), FLAG, F(3))))
LEAF_HOST( 9, fe_wred_ft, 9, "wwwf", raw_wred(0, 1, P(0), P(1), P(2), FLAG, P(3), B2, O), (fe_wred<false, true>(W(0), W(1), W(2), FLAG, F(3))))
LEAF_HOST(10, fe_wred_tf, 9, "wwwf", raw_wred(1, 0, P(0), P(1), P(2), FLAG, P(3), B2, O), (fe_wred<true, false>(W(0), W(1), W(2), FLAG, F(3))))
LEAF_HOST(11, fe_wred_tt, 9, "wwwf", raw_wred(1, 1, P(0), P(1), P(2), FLAG, P(3), B2, O), (fe_wred<true, true>(W(0), W(1), W(2), FLAG, F(3))))
// ---- fe_lc3<C1, C2, C3>: the public leaf (a real function outside the forced-inline units)
LEAF(12, lc3_1_1_0,    9, "fff", (fe_lc3<1, 1, 0>(F(0), F(1), F(2))))        // (0, N)  Karatsuba sums, f2_sum_for_mul
LEAF(13, lc3_1_m1_0,   9, "fff", (fe_lc3<1, -1, 0>(F(0), F(1), F(2))))       // (0, N)  every difference of the curve and tower formulas
LEAF(14, lc3_1_m1_m2,  9, "fff", (fe_lc3<1, -1, -2>(F(0), F(1), F(2))))      // (0, N)  curve.hpp; the narrow part AT its limit of 4
LEAF(15, lc3_1_0_0,    9, "fff", (fe_lc3<1, 0, 0>(F(0), F(1), F(2))))        // (0, N)  fe_std: a lone term with coefficient +1 stays narrow
LEAF(16, lc3_0_0_0,    9, "fff", (fe_lc3<0, 0, 0>(F(0), F(1), F(2))))        // (0, -)  INVENTED: no term at all, only kq q (the product never does this)
LEAF(17, lc3_m1_0_0,   9, "fff", (fe_lc3<-1, 0, 0>(F(0), F(1), F(2))))       // (1, -)  negation: a lone term with another coefficient goes wide
LEAF(18, lc3_9_0_0,    9, "fff", (fe_lc3<9, 0, 0>(F(0), F(1), F(2))))        // (1, -)  pairing.hpp
LEAF(19, lc3_4_0_0,    9, "fff", (fe_lc3<4, 0, 0>(F(0), F(1), F(2))))        // (1, -)  hash_ops.hpp
LEAF(20, lc3_9_m1_1,   9, "fff", (fe_lc3<9, -1, 1>(F(0), F(1), F(2))))       // (1, N)  f2_lc_xi<1, 1>, real part
LEAF(21, lc3_9_1_1,    9, "fff", (fe_lc3<9, 1, 1>(F(0), F(1), F(2))))        // (1, N)  f2_lc_xi<1, 1>, imaginary part
LEAF(22, lc3_1_m3_0,   9, "fff", (fe_lc3<1, -3, 0>(F(0), F(1), F(2))))       // (1, N)  pairing.hpp: the narrow part is the lone +1 term
LEAF(23, lc3_27_3_0,   9, "fff", (fe_lc3<27, 3, 0>(F(0), F(1), F(2))))       // (2, -)  f2_mul_iso3b
LEAF(24, lc3_27_m3_0,  9, "fff", (fe_lc3<27, -3, 0>(F(0), F(1), F(2))))      // (2, -)  f2_mul_iso3b
LEAF(25, lc3_9_m1_0,   9, "fff", (fe_lc3<9, -1, 0>(F(0), F(1), F(2))))       // (2, -)  f2_mul_xi: the lone -1 goes wide
LEAF(26, lc3_54_m6_2,  9, "fff", (fe_lc3<54, -6, 2>(F(0), F(1), F(2))))      // (3, -)  f2_lc_xi<6, 2> (tower.hpp)
// ---- fe_lc3_core / fe_lc4_core with the run-time sign of the middle term
LEAF(27, lc3c_m1_1_0_s,   9, "fff",  (fe_lc3_core<-1, 1, 0, true>(F(0), F(1), F(2), FLAG)))               // (2, -)  SIGN2; curve.hpp's conditional negation
LEAF(28, lc3c_9_1_1_s,    9, "fff",  (fe_lc3_core<9, 1, 1, true>(F(0), F(1), F(2), FLAG)))                // (2, N)  SIGN2; the body of fe_lc3_par<9, 1, 1>
LEAF(29, lc4c_9_1_1_0_s,  9, "ffff", (fe_lc4_core<9, 1, 1, 0, false, true>(F(0), F(1), F(2), F(3), FLAG)))    // (2, N)  SIGN2; the body of fe_lc4_par<9, 1, 1, 0>
LEAF(30, lc4c_27_3_3_2_s, 9, "ffff", (fe_lc4_core<27, 3, 3, 2, false, true>(F(0), F(1), F(2), F(3), FLAG)))   // (4, -)  SIGN2; the body of fe_lc4_par<27, 3, 3, 2>
LEAF(31, lc4c_27_m3_1_1,  9, "ffff", (fe_lc4_core<27, -3, 1, 1>(F(0), F(1), F(2), F(3), FLAG)))           // (2, N)  INVENTED: two wide terms and a narrow pair without SIGN2
LEAF(32, lc4c_27_3_3_1,   9, "ffff", (fe_lc4_core<27, 3, 3, 1>(F(0), F(1), F(2), F(3), FLAG)))            // (3, N)  INVENTED: no real instantiation has three wide terms and a narrow one
LEAF(33, lc4c_m27_3_3_m2, 9, "ffff", (fe_lc4_core<-27, 3, 3, -2>(F(0), F(1), F(2), F(3), FLAG)))          // (4, -)  f2_lc_xi2<-3, 3, -2>, real part
LEAF(34, lc4c_m27_m3_3_m2, 9, "ffff", (fe_lc4_core<-27, -3, 3, -2>(F(0), F(1), F(2), F(3), FLAG)))        // (4, -)  f2_lc_xi2<-3, 3, -2>, imaginary part
LEAF(35, lc4w_9_m1_1_m1,  9, "ffff", (fe_lc4_core<9, -1, 1, -1, true>(F(0), F(1), F(2), F(3), FLAG)))     // (4, -)  WIDE; f2_lc_xi2w<1, 1, -1>, real part
LEAF(36, lc4w_9_1_1_m1,   9, "ffff", (fe_lc4_core<9, 1, 1, -1, true>(F(0), F(1), F(2), F(3), FLAG)))      // (4, -)  WIDE; f2_lc_xi2w<1, 1, -1>, imaginary part
LEAF(37, lc4w_1_m1_0_0,   9, "ffff", (fe_lc4_core<1, -1, 0, 0, true>(F(0), F(1), F(2), F(3), FLAG)))      // (2, -)  WIDE; f2_lc3sw<1, -1, 0>: small coefficients kept out of the narrow sum
// ---- fe_lc3w: the all-64-bit form for unsigned inputs with limbs beyond 31 bits (plain C++ on the GPU too: no asm chain, kept for completeness)
LEAF(38, lc3w_9_m1_3,  9, "fff", (fe_lc3w<9, -1, 3>(F(0), F(1), F(2))))
LEAF(39, lc3w_1_m1_m1, 9, "fff", (fe_lc3w<1, -1, -1>(F(0), F(1), F(2))))
// clang-format on
#define LEAF_COUNT 40
