// Compressed point encodings on the GPU (include/bn254_hip.h bn254_g{1,2}_compress_batch / _decompress_batch): x and one sign bit, 32 bytes
// for G1 and 64 for G2, in two byte layouts over one record body per group.  The layouts are written as ark-serialize and gnark-crypto
// describe theirs; they are not checked against those libraries here.
//     BN254_COMPRESSED_ARK    little-endian; G2 is x.c0 then x.c1; the top two bits of the LAST byte: bit 7 = sign(y), bit 6 = infinity
//     BN254_COMPRESSED_GNARK  big-endian; G2 is x.c1 then x.c0; the top two bits of the FIRST byte: 10 sign 0, 11 sign 1, 01 infinity, 00 invalid
// In both the flags sit in the top bits of the most significant component (q < 2^254 leaves them free), so a record is parsed into canonical
// words plus two flag bits and the rest is format-agnostic.  sign(y) = 1 iff y > -y as canonical integers; in Fq2 c1 decides and c0 only
// when c1 == 0.  Decompression checks in the order flags, range, curve, subgroup (WIRE_* of io_wire.hpp: 3, 1, 4, 5); a rejected record
// decodes to G::zero(); an accepted one to the bytes g*_decode_record gives for the uncompressed record of the same point.
#pragma once
#include "io.hpp"
#include "io_wire.hpp"
#include "sqrt_ops.hpp"

namespace bn254 {

enum { COMPRESSED_ARK = 0, COMPRESSED_GNARK = 1 };

// canonical integer above (q - 1) / 2 = q >> 1
BN_FN bool words_gt_half_q(const uint32_t *w) {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t h = (k::Q32[i] >> 1) | (i < 7 ? k::Q32[i + 1] << 31 : 0u);
        int64_t s = (int64_t)h - (int64_t)w[i] + br; br = s >> 32;
    }
    return br != 0;
}
BN_FN bool fe_sign(const Fe &y) {
    uint32_t w[8];
    fe_to_raw_words(y, w);
    return words_gt_half_q(w);
}
BN_FN bool f2_sign(const Fq2A &y) {
    uint32_t w0[8], w1[8];
    fe_to_raw_words(y.c0, w0); fe_to_raw_words(y.c1, w1);
    return words_all_zero(w1, 8) ? words_gt_half_q(w0) : words_gt_half_q(w1);
}

struct CompressedFlags { bool ok, inf, sign; };
// NC components of 8 words each (c0 first) out of 32 NC bytes; the flag bits are taken off the top word
template <int NC>
BN_FN CompressedFlags compressed_parse(const uint8_t *in, int format, uint32_t (*c)[8]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (format == COMPRESSED_ARK) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint8_t *b = in + 32 * j + 4 * i;
                c[j][i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
            }
        } else {
            be_to_words<8>(in + 32 * (NC - 1 - j), c[j]);
        }
    }
    const uint32_t f = c[NC - 1][7] >> 30;
    c[NC - 1][7] &= 0x3fffffffu;
    if (format == COMPRESSED_ARK) return {f != 3u, (f & 1u) != 0, (f >> 1) != 0};
    return {f != 0u, f == 1u, f == 3u};
}
template <int NC>
BN_FN void compressed_write(uint32_t (*c)[8], bool inf, bool sign, int format, uint8_t *out) {
    const uint32_t f = format == COMPRESSED_ARK ? (inf ? 1u : sign ? 2u : 0u) : (inf ? 1u : sign ? 3u : 2u);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
#pragma unroll
        for (int i = 0; i < 8; ++i) if (inf) c[j][i] = 0u;
    }
    c[NC - 1][7] |= f << 30;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (format == COMPRESSED_ARK) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                uint8_t *b = out + 32 * j + 4 * i;
                const uint32_t v = c[j][i];
                b[0] = (uint8_t)v; b[1] = (uint8_t)(v >> 8); b[2] = (uint8_t)(v >> 16); b[3] = (uint8_t)(v >> 24);
            }
        } else {
            words_to_be<8>(c[j], out + 32 * (NC - 1 - j));
        }
    }
}
// flags, then range (curve and subgroup are the caller's): `on_curve` and `in_subgroup` only count where the earlier checks passed
BN_FN int compressed_status(const CompressedFlags &fl, bool zero, bool in_range, bool on_curve, bool in_subgroup) {
    if (!fl.ok || (fl.inf && !zero)) return WIRE_E_INVALID_LEADING_BYTE;
    if (fl.inf) return WIRE_OK;
    if (!in_range) return WIRE_E_NOT_LESS_THAN_MODULUS;
    if (!on_curve) return WIRE_E_NOT_ON_CURVE;
    return in_subgroup ? WIRE_OK : WIRE_E_NOT_IN_SUBGROUP;
}

// ---- G1: 32 bytes -------------------------------------------------------------------------------------------------------
BN_FN void g1_compress_record(const uint32_t *p, int format, uint8_t *out) {
    const bool inf = words_all_zero(p + 16, 8);
    const G1Aff<Fe> a = g1_to_affine(fe_from_u32x8(p), fe_from_u32x8(p + 8), fe_from_u32x8(p + 16));
    uint32_t c[1][8];
    fe_to_raw_words(a.x, c[0]);
    compressed_write<1>(c, inf, fe_sign(a.y), format, out);
}
template <int FORM = BN254_SQRT_WINDOW>
BN_FN int g1_decompress_record(const uint8_t *in, int format, uint32_t *out) {
    uint32_t c[1][8];
    const CompressedFlags fl = compressed_parse<1>(in, format, c);
    const Fe x = fe_from_raw_words(c[0]);
    const Fe rhs = fe_lc3<1, 1, 0>(fe_mul(fe_sqr(x), x), fe_const(k::G1_B), x);
    const FeSqrtCand r = fe_sqrt_cand<FORM>(rhs);
    const bool on_curve = fe_equal(fe_sqr(r.y), rhs);
    const Fe y = fe_select(fe_sign(r.y) != fl.sign, r.y, fe_lc3<-1, 0, 0>(r.y, r.y, r.y));
    const int status = compressed_status(fl, words_all_zero(c[0], 8), words_lt_q(c[0]), on_curve, true);
    const bool inf = fl.inf || status != WIRE_OK;                          // failed records come back as G::zero()
    uint32_t o[24];
    fe_to_u32x8(fe_select(inf, x, fe_zero()), o);
    fe_to_u32x8(fe_select(inf, y, fe_one()), o + 8);
    fe_to_u32x8(fe_select(inf, fe_one(), fe_zero()), o + 16);
    for (int i = 0; i < 24; ++i) out[i] = o[i];
    return status;
}

// ---- G2: 64 bytes -------------------------------------------------------------------------------------------------------
BN_FN void g2_compress_record(const uint32_t *p, int format, uint8_t *out) {
    const bool inf = words_all_zero(p + 32, 16);
    const G2Aff<Fq2A> a = g2_to_affine(f2_load((const Fq2A *)nullptr, p), f2_load((const Fq2A *)nullptr, p + 16), f2_load((const Fq2A *)nullptr, p + 32));
    uint32_t c[2][8];
    fe_to_raw_words(a.x.c0, c[0]); fe_to_raw_words(a.x.c1, c[1]);
    compressed_write<2>(c, inf, f2_sign(a.y), format, out);
}
// x -> (x, y): everything but the subgroup check.  `status` is final unless it is WIRE_OK for a finite point, which the subgroup check may still reject.
template <int FORM = BN254_SQRT_WINDOW>
BN_FN int g2_decompress_xy(const uint8_t *in, int format, Fq2A &x, Fq2A &y, bool &inf) {
    uint32_t c[2][8];
    const CompressedFlags fl = compressed_parse<2>(in, format, c);
    x = {fe_from_raw_words(c[0]), fe_from_raw_words(c[1])};
    const Fq2A rhs = f2_lc3<1, 1, 0>(f2_mul(f2_sqr(x), x), f2_const((const Fq2A *)nullptr, k::G2_B), x);
    const F2Sqrt r = f2_sqrt<FORM>(rhs);
    y = f2_select(f2_sign(r.root) != fl.sign, r.root, f2_neg(r.root));
    inf = fl.inf;
    return compressed_status(fl, words_all_zero(c[0], 8) && words_all_zero(c[1], 8), words_lt_q(c[0]) && words_lt_q(c[1]), r.is_square, true);
}
template <int FORM = BN254_SQRT_WINDOW>
BN_FN int g2_decompress_record(const uint8_t *in, int format, uint32_t *out) {
    using F = Fq2Field<Fq2A>;
    Fq2A x, y;
    bool inf;
    int status = g2_decompress_xy<FORM>(in, format, x, y, inf);
    const bool in_subgroup = g2_in_subgroup(x, y);                         // every lane runs the chain: its scalar is uniform, its result counts only here
    if (status == WIRE_OK && !inf && !in_subgroup) status = WIRE_E_NOT_IN_SUBGROUP;
    inf = inf || status != WIRE_OK;
    uint32_t o[48];
    f2_store(f2_select(inf, x, F::zero()), o);
    f2_store(f2_select(inf, y, F::one()), o + 16);
    f2_store(f2_select(inf, F::one(), F::zero()), o + 32);
    for (int i = 0; i < 48; ++i) out[i] = o[i];
    return status;
}

}  // namespace bn254
