// The constants of the wide Poseidon calls (bn254_fr_poseidon_ex_batch, bn254_fr_poseidon_chain_batch: widths t = 2 .. 17), derived on the HOST at
// the first use of a width: the tables of all sixteen widths hold 12 638 field elements (404 KB), which as a generated header would be more
// than a megabyte of text, so the derivation of bn_amd/poseidon.py is restated here instead - the Grain LFSR of the Poseidon paper (appendix F),
// round constants by rejection sampling, the 2 t matrix draws reduced mod r, M[i][j] = 1 / (xs[i] + ys[j]).  The first Cauchy draw is good at
// every width (distinct values, no zero sum; tests/test_poseidon_wide_model.py), so there is no retry.  The tests compare every element with the Python derivation.
//
// Plain host code, no HIP and none of the device headers: four 64-bit limbs, a Montgomery product, Fermat for the t^2 inversions of a width
// (1 784 in all).  The host simulation compiles this very file.  Entries come out as Montgomery images, eight u32 words, least significant first -
// what fr_const (fr.hpp) expects.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bn254 { namespace psdw {

constexpr int T_MIN = 2, T_MAX = 17, R_F = 8;
// R_P of t = 2 .. 17 (circomlib's list)
constexpr int R_P[T_MAX + 1] = {0, 0, 56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68};
constexpr int rounds(int t) { return R_F + R_P[t]; }
constexpr size_t table_elems(int t) { return (size_t)rounds(t) * t + (size_t)t * t; }      // C, then M row-major

struct U256 { uint64_t w[4]; };
constexpr U256 MOD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};     // r

inline bool lt(const U256 &a, const U256 &b) {
    for (int i = 3; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
    return false;
}
inline bool is_zero(const U256 &a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) == 0; }
inline bool eq(const U256 &a, const U256 &b) { return !lt(a, b) && !lt(b, a); }
// a - b for a >= b
inline U256 sub(const U256 &a, const U256 &b) {
    U256 r; unsigned __int128 br = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - br;
        r.w[i] = (uint64_t)d; br = (uint64_t)(d >> 64) ? 1 : 0;
    }
    return r;
}
// a + b mod r for a, b < r (r < 2^254: the sum has no carry out)
inline U256 add_mod(const U256 &a, const U256 &b) {
    U256 r; unsigned __int128 c = 0;
    for (int i = 0; i < 4; ++i) { c += (unsigned __int128)a.w[i] + b.w[i]; r.w[i] = (uint64_t)c; c >>= 64; }
    return lt(r, MOD) ? r : sub(r, MOD);
}
// -r^-1 mod 2^64 by Newton's iteration
inline uint64_t mont_inv64() {
    uint64_t x = 1;
    for (int i = 0; i < 6; ++i) x *= 2 - MOD.w[0] * x;
    return 0 - x;
}
// a b / 2^256 mod r for a, b < r (CIOS over 64-bit limbs)
inline U256 mont_mul(const U256 &a, const U256 &b) {
    static const uint64_t inv = mont_inv64();
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; ++j) { c += (unsigned __int128)a.w[i] * b.w[j] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * inv;
        c = ((unsigned __int128)m * MOD.w[0] + t[0]) >> 64;
        for (int j = 1; j < 4; ++j) { c += (unsigned __int128)m * MOD.w[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
    }
    U256 r = {{t[0], t[1], t[2], t[3]}};
    return (t[4] || !lt(r, MOD)) ? sub(r, MOD) : r;
}
// 2^256 mod r and 2^512 mod r by doubling
inline U256 pow2_mod(int e) {
    U256 x = {{1, 0, 0, 0}};
    for (int i = 0; i < e; ++i) x = add_mod(x, x);
    return x;
}
inline const U256 &mont_one() { static const U256 v = pow2_mod(256); return v; }
inline const U256 &mont_r2() { static const U256 v = pow2_mod(512); return v; }
inline U256 to_mont(const U256 &a) { return mont_mul(a, mont_r2()); }
// 1 / a as a Montgomery image, for a Montgomery image a != 0: a^(r - 2)
inline U256 mont_inverse(const U256 &a) {
    const U256 two = {{2, 0, 0, 0}};
    const U256 e = sub(MOD, two);
    U256 acc = mont_one();
    for (int i = 253; i >= 0; --i) {
        acc = mont_mul(acc, acc);
        if ((e.w[i >> 6] >> (i & 63)) & 1) acc = mont_mul(acc, a);
    }
    return acc;
}

// The 80-bit LFSR: start bits, most significant first, 1 in 2 bits (a prime field), 0 in 4 bits (the S-box x^alpha), the field size in 12
// bits, t in 12, R_F in 10, R_P in 10, thirty ones; the first 160 outputs are discarded.  b[(head + i) % 80] is bit i of the paper.
struct Grain {
    unsigned char b[80];
    int head = 0;
    Grain(int t, int r_f, int r_p) {
        const unsigned long value[7] = {1, 0, 254, (unsigned long)t, (unsigned long)r_f, (unsigned long)r_p, (1ul << 30) - 1};
        const int width[7] = {2, 4, 12, 12, 10, 10, 30};
        int at = 0;
        for (int f = 0; f < 7; ++f)
            for (int i = 0; i < width[f]; ++i) b[at++] = (unsigned char)((value[f] >> (width[f] - 1 - i)) & 1);
        for (int i = 0; i < 160; ++i) step();
    }
    int tap(int i) const { return b[(head + i) % 80]; }
    int step() {
        const int n = tap(62) ^ tap(51) ^ tap(38) ^ tap(23) ^ tap(13) ^ tap(0);
        b[head] = (unsigned char)n;            // the oldest bit leaves, the new one is bit 79
        head = (head + 1) % 80;
        return n;
    }
    // one stream bit: outputs are taken in pairs, and a pair whose first bit is 0 is thrown away
    int bit() {
        while (step() == 0) step();
        return step();
    }
    // 254 bits, most significant first
    U256 draw() {
        U256 v = {{0, 0, 0, 0}};
        for (int i = 0; i < 254; ++i) {
            for (int j = 3; j > 0; --j) v.w[j] = v.w[j] << 1 | v.w[j - 1] >> 63;
            v.w[0] = v.w[0] << 1 | (uint64_t)bit();
        }
        return v;
    }
};

inline void put_words(const U256 &a, uint32_t *out) {
    for (int i = 0; i < 4; ++i) { out[2 * i] = (uint32_t)a.w[i]; out[2 * i + 1] = (uint32_t)(a.w[i] >> 32); }
}

// The table of width t: rounds(t) * t round constants in round order, then the t x t matrix row-major, table_elems(t) records of eight words.
// Returns false for a width outside 2 .. 17 or - at no width, see above - a Cauchy draw that would need the retry.
inline bool derive(int t, std::vector<uint32_t> &out) {
    if (t < T_MIN || t > T_MAX) return false;
    Grain g(t, R_F, R_P[t]);
    const size_t nc = (size_t)rounds(t) * t;
    out.assign(table_elems(t) * 8, 0u);
    for (size_t i = 0; i < nc;) {
        const U256 v = g.draw();
        if (lt(v, MOD)) put_words(to_mont(v), out.data() + 8 * i++);      // rejection sampling: a draw at or above r is skipped
    }
    U256 xy[2 * T_MAX];
    for (int i = 0; i < 2 * t; ++i) {                                    // the matrix draws are reduced, not rejected: a draw is below 2^254 < 6 r
        U256 v = g.draw();
        while (!lt(v, MOD)) v = sub(v, MOD);
        xy[i] = v;
    }
    for (int i = 0; i < 2 * t; ++i)
        for (int j = 0; j < i; ++j)
            if (eq(xy[i], xy[j])) return false;
    for (int i = 0; i < t; ++i)
        for (int j = 0; j < t; ++j) {
            const U256 s = add_mod(xy[i], xy[t + j]);
            if (is_zero(s)) return false;
            put_words(mont_inverse(to_mont(s)), out.data() + 8 * (nc + (size_t)i * t + j));
        }
    return true;
}

}}  // namespace bn254::psdw
