// The scalar field Fr on the device: one Fr as eight u32 words in Montgomery radix 2^256 (the bytes of the C ABI), and the ONE word-serial
// Montgomery arithmetic mod r every route of a scalar into a kernel goes through - the Fr kernels (fr_ops.hpp), the wire records
// (io_wire.hpp), the scalar extraction of the point and Gt kernels (curve.hpp: fr_from_mont) and the synthetic benchmark scalars.  Only
// arithmetic: nothing here knows a memory layout or a kernel.  Everything is pure, so the host simulation (tests/hostsim/) runs the very same
// code.  The Fq machinery (fe.hpp's 29-bit limbs, generated for q) is not used: fe.hpp is included for BN_FN and k:: only.
#pragma once
#include "fe.hpp"

namespace bn254 {

BN254_CONSTANT uint32_t FR_ONE_32[8] = {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};     // 2^256 mod r: Fr::one()
BN254_CONSTANT uint32_t FR_R3_32[8] = {0xb4bf0040u, 0x5e94d8e1u, 0x1cfbb6b8u, 0x2a489cbeu, 0xa19fcfedu, 0x893cc664u, 0x7fcc657cu, 0x0cf8594bu};      // 2^768 mod r

struct Fr { uint32_t w[8]; };

BN_FN Fr fr_const(const uint32_t *c) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = c[i];
    return r;
}
BN_FN Fr fr_zero() {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = 0u;
    return r;
}
BN_FN Fr fr_one() { return fr_const(FR_ONE_32); }
BN_FN bool fr_is_zero(const Fr &a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.w[i];
    return o == 0;
}
BN_FN bool fr_eq(const Fr &a, const Fr &b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.w[i] ^ b.w[i];
    return o == 0;
}
BN_FN Fr fr_select(bool take_b, const Fr &a, const Fr &b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = take_b ? b.w[i] : a.w[i];
    return r;
}
// the 256-bit integer w (eight words, least significant first) is below r
BN_FN bool fr_lt_r(const uint32_t *w) {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { int64_t v = (int64_t)w[i] - (int64_t)k::FR_MOD32[i] + br; br = v >> 32; }
    return br != 0;
}
// t (eight words and a carry word) -> t - r when t >= r.  For t < 2 r the result is canonical.
BN_FN Fr fr_reduce_once(const uint32_t *t, uint32_t top) {
    uint32_t d[8];
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t v = (int64_t)t[i] - (int64_t)k::FR_MOD32[i] + br;
        d[i] = (uint32_t)v; br = v >> 32;
    }
    const bool ge = top != 0 || br == 0;
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = ge ? d[i] : t[i];
    return r;
}
// a + b mod r
BN_FN Fr fr_add(const Fr &a, const Fr &b) {
    uint32_t t[8];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { c += (uint64_t)a.w[i] + b.w[i]; t[i] = (uint32_t)c; c >>= 32; }
    return fr_reduce_once(t, (uint32_t)c);
}
// a - b mod r: r is added back when the difference borrows
BN_FN Fr fr_sub(const Fr &a, const Fr &b) {
    uint32_t t[8];
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int64_t v = (int64_t)a.w[i] - (int64_t)b.w[i] + br; t[i] = (uint32_t)v; br = v >> 32; }
    const uint32_t mask = br ? 0xffffffffu : 0u;
    Fr r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { c += (uint64_t)t[i] + (k::FR_MOD32[i] & mask); r.w[i] = (uint32_t)c; c >>= 32; }
    return r;
}
// a * b / 2^256 mod r, word-serial (CIOS): per word of a, one row of eight products into t and one row of eight products m * r that
// clears the low word - 128 multiply-adds of the shape (uint64_t)x * y + z, and eight low products for m.
// PRECONDITION: one operand is canonical (< r); the other may be any 256-bit value.  The rows leave (a b + M r) / 2^256 with M < 2^256,
// which is below 2 r as soon as a b < 2^256 r, so the one conditional subtraction gives the canonical result (on the way t < b + r < 2^257:
// the carry word holds it).  With neither operand below r the result need not be canonical.
BN_FN Fr fr_mul(const Fr &a, const Fr &b) {
    uint32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t x = (uint64_t)a.w[i] * b.w[j] + t[j] + c;
            t[j] = (uint32_t)x; c = x >> 32;
        }
        const uint64_t top = (uint64_t)t[8] + c;                          // < 2^33
        const uint32_t m = t[0] * k::FR_INV32;
        c = ((uint64_t)m * k::FR_MOD32[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            const uint64_t y = (uint64_t)m * k::FR_MOD32[j] + t[j] + c;
            t[j - 1] = (uint32_t)y; c = y >> 32;
        }
        const uint64_t y = top + c;
        t[7] = (uint32_t)y; t[8] = (uint32_t)(y >> 32);
    }
    return fr_reduce_once(t, t[8]);
}
// sum_k a[k] * b[k] / 2^256 mod r for T <= 5 pairs with ONE reduction: per word, T rows of eight products into t and then the one row m * r
// that clears the low word - 8 T + 8 multiply-adds per word where T calls of fr_mul take 16 T.
// PRECONDITION: every a[k] and every b[k] is canonical (< r).  Then sum a b <= 5 (r - 1)^2 < 2^256 r because 5 r < 2^256, so the rows leave
// (sum a b + M r) / 2^256 < 2 r and the one conditional subtraction gives the canonical result.  On the way, after every word,
// t < t_before / 2^32 + 5 r + r, which stays below 6 r (1 + 2^-31) < 2^257: the carry word holds 0 or 1; inside a word the carries of
// the T rows are summed in 64 bits.  The bound-enforcing host simulation (BN_BOUNDS) checks the precondition, the carry word after every word and
// t < 2 r at the end.
template <int T>
BN_FN Fr fr_dot(const Fr (&a)[T], const uint32_t (*b)[8]) {
    static_assert(T >= 1 && T <= 5, "5 r < 2^256 < 6 r");
#if defined(BN_BOUNDS)
    for (int q = 0; q < T; ++q) BN_REQUIRE(fr_lt_r(a[q].w) && fr_lt_r(b[q]), "fr_dot takes canonical operands");
#endif
    uint32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t top = t[8];
#pragma unroll
        for (int q = 0; q < T; ++q) {
            uint64_t c = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint64_t x = (uint64_t)a[q].w[i] * b[q][j] + t[j] + c;
                t[j] = (uint32_t)x; c = x >> 32;
            }
            top += c;                                                       // < 1 + 5 * 2^32
        }
        const uint32_t m = t[0] * k::FR_INV32;
        uint64_t c = ((uint64_t)m * k::FR_MOD32[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            const uint64_t y = (uint64_t)m * k::FR_MOD32[j] + t[j] + c;
            t[j - 1] = (uint32_t)y; c = y >> 32;
        }
        const uint64_t y = top + c;
        t[7] = (uint32_t)y; t[8] = (uint32_t)(y >> 32);
#if defined(BN_BOUNDS)
        BN_REQUIRE((y >> 32) <= 1, "fr_dot: the running value left 2^257");
#endif
    }
#if defined(BN_BOUNDS)
    {   // t < 2 r: t - r < r
        uint32_t d[8]; int64_t br = 0;
        for (int i = 0; i < 8; ++i) { const int64_t v = (int64_t)t[i] - (int64_t)k::FR_MOD32[i] + br; d[i] = (uint32_t)v; br = v >> 32; }
        BN_REQUIRE(t[8] == 0 ? (br != 0 || fr_lt_r(d)) : (br != 0 && fr_lt_r(d)), "fr_dot: the sum before the subtraction is not below 2 r");
    }
#endif
    return fr_reduce_once(t, t[8]);
}
// Fr out of Montgomery form (fields/fp.rs:15-22: multiply by 1): 8 x u32 words, word-serial Montgomery reduction mod r
BN_FN void fr_from_mont(const uint32_t *km, uint32_t *raw) {
    uint32_t t[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = km[i];
    t[8] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t m = t[0] * k::FR_INV32;
        uint64_t c = ((uint64_t)m * k::FR_MOD32[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            uint64_t x = (uint64_t)m * k::FR_MOD32[j] + t[j] + c;
            t[j - 1] = (uint32_t)x;
            c = x >> 32;
        }
        uint64_t x = (uint64_t)t[8] + c;
        t[7] = (uint32_t)x;
        t[8] = (uint32_t)(x >> 32);
    }
    // t < 2r; one conditional subtraction
    uint32_t d[8];
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int64_t s = (int64_t)t[i] - (int64_t)k::FR_MOD32[i] + br;
        d[i] = (uint32_t)s;
        br = s >> 32;
    }
    bool ge = (t[8] != 0) || (br == 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) raw[i] = ge ? d[i] : t[i];
}
// the 512-bit integer hi * 2^256 + lo, mod r, as a Montgomery image: lo * R^2 / R = lo * R and hi * R^3 / R = (hi * 2^256) * R.  Neither
// half need be below r: R^2 and R^3 are the canonical operands of the two products, so both are canonical and their sum needs one subtraction.
BN_FN Fr fr_from_wide(const Fr &lo, const Fr &hi) { return fr_add(fr_mul(lo, fr_const(k::FR_R2_32)), fr_mul(hi, fr_const(FR_R3_32))); }

}  // namespace bn254
