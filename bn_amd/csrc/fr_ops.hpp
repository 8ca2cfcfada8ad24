// The per-lane bodies of the scalar-field kernels (bn254_fr.hip): bn254_fr_{add,mul,inverse,pow,interpret}_batch.  One Fr per lane as eight
// u32 words in Montgomery radix 2^256 - the bytes of the C ABI, so nothing is converted on the way in or out - and every result canonical
// (< r), hence unique: the bytes are the reference's whichever algorithm computes them (fields/fp.rs, arith.rs:183-279).  Everything here is
// pure and takes plain pointers and an element (inverse: run) index, so the host simulation (tests/hostsim/hostsim_fr.cpp) runs the very same
// bodies over host arrays.  The Fq machinery (fe.hpp's 29-bit limbs, generated for q) is not used: fe.hpp is included for BN_FN and k:: only.
#pragma once
#include <stddef.h>
#include "fe.hpp"

namespace bn254 {

BN254_CONSTANT uint32_t FR_ONE_32[8] = {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};     // 2^256 mod r: Fr::one()
BN254_CONSTANT uint32_t FR_R3_32[8] = {0xb4bf0040u, 0x5e94d8e1u, 0x1cfbb6b8u, 0x2a489cbeu, 0xa19fcfedu, 0x893cc664u, 0x7fcc657cu, 0x0cf8594bu};      // 2^768 mod r
BN254_CONSTANT uint32_t FR_MINUS_2_32[8] = {0xefffffffu, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}; // r - 2 (raw): the Fermat exponent
constexpr int FR_BITS = 254;                 // bits of r: a canonical exponent has no bit above
// The shipped choices (plain constants - the library has no compile switch for them; bn254_fr.hip carries a run-time override for the
// sweep of tools/time_fr.py only).  Window width of pow, one of 1 / 2 / 4; elements per lane that share one inversion, one of 1 / 4 / 8 / 16.
constexpr int FR_POW_WINDOW = 2;
constexpr uint32_t FR_INV_RUN = 8;

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
// record `i` of an array of 32-byte records, as two 16-byte moves
BN_FN Fr fr_load(const uint32_t *p, size_t i) {
    Fr r;
#if defined(BN_HOSTSIM)
    for (int j = 0; j < 8; ++j) r.w[j] = p[8 * i + j];
#else
    const uint4 lo = ((const uint4 *)p)[2 * i], hi = ((const uint4 *)p)[2 * i + 1];
    r.w[0] = lo.x; r.w[1] = lo.y; r.w[2] = lo.z; r.w[3] = lo.w; r.w[4] = hi.x; r.w[5] = hi.y; r.w[6] = hi.z; r.w[7] = hi.w;
#endif
    return r;
}
BN_FN void fr_store(const Fr &a, uint32_t *p, size_t i) {
#if defined(BN_HOSTSIM)
    for (int j = 0; j < 8; ++j) p[8 * i + j] = a.w[j];
#else
    ((uint4 *)p)[2 * i] = make_uint4(a.w[0], a.w[1], a.w[2], a.w[3]);
    ((uint4 *)p)[2 * i + 1] = make_uint4(a.w[4], a.w[5], a.w[6], a.w[7]);
#endif
}
BN_FN bool fr_is_zero(const Fr &a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.w[i];
    return o == 0;
}
BN_FN Fr fr_select(bool take_b, const Fr &a, const Fr &b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = take_b ? b.w[i] : a.w[i];
    return r;
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
// clears the low word - 128 multiply-adds of the shape (uint64_t)x * y + z, and eight low products for m.  One operand canonical (< r)
// keeps t below 2 r, so the one conditional subtraction gives the canonical result; the other may be any 256-bit value.
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
// the canonical integer of a Montgomery image: a / 2^256 mod r
BN_FN Fr fr_raw(const Fr &a) {
    Fr one = fr_zero();
    one.w[0] = 1u;
    return fr_mul(a, one);
}
// digit w (WB bits, WB divides 32) of the integer e
template <int WB>
BN_FN uint32_t fr_digit(const Fr &e, int w) {
    const int bit = w * WB;
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) word = (bit >> 5) == i ? e.w[i] : word;
    return (word >> (bit & 31)) & ((1u << WB) - 1u);
}
// a^e for the INTEGER e < 2^254 (fields/mod.rs:35-46 computes the same value bit by bit): a fixed window of WB bits, most significant
// first, over all ceil(254 / WB) windows whatever e holds - WB squarings and ONE product per window, by Fr::one() where the digit is zero.
// The table 1, a, .. a^(2^WB - 1) stays in registers: an entry is picked by a chain of selects, never by an address.  0^0 = 1 (every digit
// picks one), 0^e = 0 for e > 0 (some digit picks zero).
template <int WB>
BN_FN Fr fr_pow_raw(const Fr &a, const Fr &e) {
    constexpr int T = 1 << WB, NW = (FR_BITS + WB - 1) / WB;
    Fr tbl[T];
    tbl[0] = fr_one();
    tbl[1] = a;
#pragma unroll
    for (int i = 2; i < T; ++i) tbl[i] = fr_mul(tbl[i - 1], a);
    Fr acc = fr_zero();
#pragma unroll 1
    for (int w = NW - 1; w >= 0; --w) {
        const uint32_t d = fr_digit<WB>(e, w);
        Fr f = tbl[0];
#pragma unroll
        for (int i = 1; i < T; ++i) f = fr_select(d == (uint32_t)i, f, tbl[i]);
        if (w == NW - 1) { acc = f; continue; }                            // uniform: the top window starts the chain
#pragma unroll
        for (int s = 0; s < WB; ++s) acc = fr_mul(acc, acc);
        acc = fr_mul(acc, f);
    }
    return acc;
}

// ---- the bodies: element i of a launch
BN_FN void fr_add_body(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t i, int negate_b) {
    const Fr x = fr_load(a, i), y = fr_load(b, i);
    fr_store(negate_b ? fr_sub(x, y) : fr_add(x, y), out, i);
}
BN_FN void fr_mul_body(const uint32_t *a, const uint32_t *b, uint32_t *out, size_t i) {
    const Fr x = fr_load(a, i), y = fr_load(b, i);
    fr_store(fr_mul(x, y), out, i);
}
// a^(canonical integer of e), lib.rs:23
template <int WB>
BN_FN void fr_pow_body(const uint32_t *a, const uint32_t *e, uint32_t *out, size_t i) {
    const Fr x = fr_load(a, i), y = fr_raw(fr_load(e, i));
    fr_store(fr_pow_raw<WB>(x, y), out, i);
}
// lib.rs:27-29 over arith.rs:90-97: record i of 64 bytes as a big-endian 512-bit integer hi * 2^256 + lo, mod r.  lo * R^2 / R = lo * R and
// hi * R^3 / R = (hi * 2^256) * R are both canonical (R^2, R^3 are), so their sum needs one subtraction.
BN_FN void fr_interpret_body(const uint8_t *in, uint32_t *out, size_t i) {
    Fr hi, lo;
#if defined(BN_HOSTSIM)
    const uint8_t *p = in + 64 * i;
    for (int j = 0; j < 8; ++j) {
        hi.w[7 - j] = (uint32_t)p[4 * j] << 24 | (uint32_t)p[4 * j + 1] << 16 | (uint32_t)p[4 * j + 2] << 8 | p[4 * j + 3];
        lo.w[7 - j] = (uint32_t)p[32 + 4 * j] << 24 | (uint32_t)p[32 + 4 * j + 1] << 16 | (uint32_t)p[32 + 4 * j + 2] << 8 | p[32 + 4 * j + 3];
    }
#else
    const uint4 *p = (const uint4 *)in + 4 * i;
    const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    const uint32_t b[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) { hi.w[7 - j] = __builtin_bswap32(b[j]); lo.w[7 - j] = __builtin_bswap32(b[8 + j]); }
#endif
    fr_store(fr_add(fr_mul(lo, fr_const(k::FR_R2_32)), fr_mul(hi, fr_const(FR_R3_32))), out, i);
}
// Option<Fr> inverse of the run of K consecutive elements [lane * K, min(n, (lane + 1) * K)) with ONE exponentiation (Montgomery's trick):
// forward, the product of the elements in front of each one (one in place of a zero element) goes to `prefix`; the run's product is raised
// to r - 2; backward, element j gets (inverse so far) * (its prefix) and the inverse so far takes the element in.  A zero element yields
// out = Fr::zero() and ok = 0 (ok may be NULL) and leaves its neighbours alone.  out may be a: a lane reads element j before it writes it and
// touches no other lane's run.  prefix: K * lanes records, record j of a run at (j * lanes + lane) so that a wave writes adjacent records.
template <int WB>
BN_FN void fr_inverse_body(const uint32_t *a, uint32_t *out, int32_t *ok, uint32_t *prefix, uint32_t n, uint32_t lane, uint32_t lanes, uint32_t K) {
    const size_t lo = (size_t)lane * K;
    if (lane >= lanes || lo >= n) return;
    const uint32_t len = (uint32_t)(n - lo < K ? n - lo : K);
    const Fr one = fr_one();
    Fr acc = one;
#pragma unroll 1
    for (uint32_t j = 0; j < len; ++j) {
        const Fr x = fr_load(a, lo + j);
        fr_store(acc, prefix, (size_t)j * lanes + lane);
        acc = fr_mul(acc, fr_select(fr_is_zero(x), x, one));
    }
    Fr inv = fr_pow_raw<WB>(acc, fr_const(FR_MINUS_2_32));
#pragma unroll 1
    for (uint32_t j = len; j-- > 0;) {
        const Fr x = fr_load(a, lo + j);
        const bool z = fr_is_zero(x);
        const Fr r = fr_mul(inv, fr_load(prefix, (size_t)j * lanes + lane));
        inv = fr_mul(inv, fr_select(z, x, one));
        fr_store(fr_select(z, r, fr_zero()), out, lo + j);
        if (ok) ok[lo + j] = z ? 0 : 1;
    }
}

}  // namespace bn254
