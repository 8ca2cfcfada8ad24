// The per-lane bodies of the scalar-field kernels (bn254_fr.hip): bn254_fr_{add,mul,inverse,pow,interpret}_batch, and of the generator of
// the synthetic benchmark scalars (bn254_measure.hip).  One Fr per lane as eight u32 words in Montgomery radix 2^256 - the bytes of the C
// ABI, so nothing is converted on the way in or out - and every result canonical (< r), hence unique: the bytes are the reference's whichever
// algorithm computes them (fields/fp.rs, arith.rs:183-279).  The arithmetic itself is fr.hpp; here are the moves between memory and
// registers, pow, and the bodies.  Everything is pure and takes plain pointers and an element (inverse: run) index, so the host simulation
// (tests/hostsim/hostsim_fr.cpp) runs the very same bodies over host arrays.
#pragma once
#include <stddef.h>
#include "fr.hpp"

namespace bn254 {

BN254_CONSTANT uint32_t FR_MINUS_2_32[8] = {0xefffffffu, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}; // r - 2 (raw): the Fermat exponent
constexpr int FR_BITS = 254;                 // bits of r: a canonical exponent has no bit above
// The shipped choices (plain constants - the library has no compile switch for them; bn254_fr.hip carries a run-time override for the
// sweep of tools/time_fr.py only).  Window width of pow, one of 1 / 2 / 4; elements per lane that share one inversion, one of 1 / 4 / 8 / 16.
constexpr int FR_POW_WINDOW = 2;
constexpr uint32_t FR_INV_RUN = 8;

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
// the canonical integer of a Montgomery image: a / 2^256 mod r
BN_FN Fr fr_raw(const Fr &a) {
    Fr r;
    fr_from_mont(a.w, r.w);
    return r;
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
// lib.rs:27-29 over arith.rs:90-97: record i of 64 bytes as a big-endian 512-bit integer hi * 2^256 + lo, mod r
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
    fr_store(fr_from_wide(lo, hi), out, i);
}
// element j of bn254_synthetic_scalars_dev: the 512-bit SplitMix64 draw of stream 2 * (lo + j) + which (eight outputs, least significant
// first, each as two words), mod r - bn_amd.distributed.synthetic_scalars word for word
BN_FN void fr_synthetic_body(uint64_t seed, uint64_t lo, uint32_t j, uint32_t which, uint32_t *out) {
    uint64_t state = seed + (((lo + j) * 2 + which) << 32);
    Fr half[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        half[i >> 2].w[2 * (i & 3)] = (uint32_t)z; half[i >> 2].w[2 * (i & 3) + 1] = (uint32_t)(z >> 32);
    }
    fr_store(fr_from_wide(half[0], half[1]), out, j);
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
