// Square roots in Fq and Fq2 for the compressed point encodings (io_compress.hpp).  q = 3 mod 4, so one exponentiation by the fixed
// exponent e = (q - 3) / 4 gives a root candidate, its inverse square and the quadratic character together:
//     t = a^e,   y = t a = a^((q+1)/4),   chi = t y = a^((q-1)/2)   =>   y^2 = chi a
// y is a root of a when chi == 1, a root of -a when chi == -1, and a == 0 gives (0, 0, 0).  The exponent is the same for every lane: its bits
// drive scalar branches, like fe_inverse_fermat (fe.hpp).  Two forms of the chain behind one compile-time switch, BN254_SQRT_WINDOW:
//     0   square-and-multiply over the 252 bits of e (251 squarings, 108 products: 109 bits are set)
//     1   a fixed 4-bit window: a^1 .. a^15 (14 products), then 63 windows of 4 squarings and one table product (56 in all: six windows are zero)
// Both are templates over the form, so the host simulation runs the two under -DBN_BOUNDS whichever one the library ships.
#pragma once
#include "fq2.hpp"

#ifndef BN254_SQRT_WINDOW
#define BN254_SQRT_WINDOW 1            // the faster of the two on G1 decompression of 2^20 records (profiles/r21_compress.txt); 0 stays buildable: tools/build_variant.sh
#endif

namespace bn254 {

constexpr int SQRT_EXP_BITS = 252;                  // e = (q - 3) / 4 = (q - 2) >> 2: bit i of e is bit i + 2 of k::Q_MINUS_2
BN_FN uint32_t sqrt_exp_bits(int lo, int n) {       // n <= 4 bits of e from bit lo upwards
    const int at = lo + 2;
    uint64_t v = k::Q_MINUS_2[at >> 6] >> (at & 63);
    if ((at & 63) > 60 && (at >> 6) < 3) v |= k::Q_MINUS_2[(at >> 6) + 1] << (64 - (at & 63));
    return (uint32_t)v & ((1u << n) - 1u);
}

struct FeSqrtCand { Fe t, y, chi; };

// a: lb <= 2, vb <= 6.  Every output is a Montgomery product: (1, 2)
template <int FORM = BN254_SQRT_WINDOW>
BN_FN FeSqrtCand fe_sqrt_cand(const Fe &a) {
    BN_REQUIRE(!a.sg && a.lb <= 2 && a.vb <= 6, "fe_sqrt_cand input");
    Fe r;
    if (FORM == 0) {
        r = a;                                      // the top bit of e
#pragma unroll 1
        for (int i = SQRT_EXP_BITS - 2; i >= 0; --i) {
            r = fe_sqr(r);
            if (sqrt_exp_bits(i, 1)) r = fe_mul(r, a);
        }
    } else {
        Fe tab[16];
        tab[0] = fe_one(); tab[1] = a;
#pragma unroll 1
        for (int i = 2; i < 16; ++i) tab[i] = fe_mul(tab[i - 1], a);
        r = tab[sqrt_exp_bits(SQRT_EXP_BITS - 4, 4)];   // 252 = 63 * 4: the top window is full (and not zero)
#pragma unroll 1
        for (int i = SQRT_EXP_BITS - 8; i >= 0; i -= 4) {
            r = fe_sqr(fe_sqr(fe_sqr(fe_sqr(r))));
            const uint32_t w = sqrt_exp_bits(i, 4);
            if (w) r = fe_mul(r, tab[w]);
        }
    }
    FeSqrtCand c;
    c.t = r;
    c.y = fe_mul(r, a);
    c.chi = fe_mul(r, c.y);
    return c;
}

// a == b (mod q) for Montgomery products / standard-form values
BN_FN bool fe_equal(const Fe &a, const Fe &b) { return fe_is_zero(fe_sub<1, 4>(a, b)); }

struct F2Sqrt { Fq2A root; bool is_square; };

// a in standard form.  Two candidate chains and no inversion; every case is a select, so all lanes run the same instructions:
//     n = a0^2 + a1^2,  s = a root candidate of n,  d = (a0 + s) / 2,  (t, w, chi_d) = cand(d)  =>  w^2 = chi_d d,  1 / w = w t^2,
//     h = a1 / (2 w);   the root is (w, h) for chi_d = 1 and (h, w) for chi_d = -1, because (a0 - s) / 2 = -a1^2 / (4 d).
// d == 0 forces a1 == 0; the second chain then runs on a0 itself and the same two forms are the roots (h = 0).
// `is_square` is decided by squaring the result: for a non-square (the norm n is a non-residue) the chains return something whose square is not a.
template <int FORM = BN254_SQRT_WINDOW>
BN_FN F2Sqrt f2_sqrt(const Fq2A &a) {
    const Fe n = fe_lc3<1, 1, 0>(fe_sqr(a.c0), fe_sqr(a.c1), a.c1);
    const FeSqrtCand cn = fe_sqrt_cand<FORM>(n);
    const Fe d = fe_norm(fe_half(fe_add(a.c0, cn.y)));
    const FeSqrtCand cd = fe_sqrt_cand<FORM>(fe_select(fe_is_zero(d), d, a.c0));
    const Fe winv = fe_mul(cd.y, fe_sqr(cd.t));
    const Fe h = fe_norm(fe_half(fe_mul(a.c1, winv)));
    const bool swap = fe_is_zero(fe_add(cd.chi, fe_one()));               // chi_d == -1
    F2Sqrt r;
    r.root = {fe_select(swap, cd.y, h), fe_select(swap, h, cd.y)};
    const Fq2A sq = f2_sqr(r.root);
    r.is_square = fe_equal(sq.c0, a.c0) & fe_equal(sq.c1, a.c1);
    return r;
}

}  // namespace bn254
