// Boundary I/O of the HIP pairing engine: the reference's #[repr(C)] images <-> engine values.
//   G1 = 24 u32 (x,y,z Fq)   G2 = 48 u32 (x,y,z Fq2)   Gt/Fq12 = 96 u32 in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1
#pragma once
#include "pairing.hpp"

namespace bn254 {

#define F2P ((const F2 *)nullptr)
template <class F2>
BN_FN Fq12<F2> f12_load(const uint32_t *w) {
    Fq12<F2> f;
    f.c0.c0 = f2_load(F2P, w + 0);  f.c0.c1 = f2_load(F2P, w + 16); f.c0.c2 = f2_load(F2P, w + 32);
    f.c1.c0 = f2_load(F2P, w + 48); f.c1.c1 = f2_load(F2P, w + 64); f.c1.c2 = f2_load(F2P, w + 80);
    return f;
}
template <class F2>
BN_FN void f12_store(const Fq12<F2> &f, uint32_t *w) {
    f2_store(f.c0.c0, w + 0);  f2_store(f.c0.c1, w + 16); f2_store(f.c0.c2, w + 32);
    f2_store(f.c1.c0, w + 48); f2_store(f.c1.c1, w + 64); f2_store(f.c1.c2, w + 80);
}
// one piece of a segmented Fq12 fold (bn254_pairing_product_batch): dst = src[0] * ... * src[cnt-1], or one for cnt == 0.
// Built on the host, read by bn254_gt_mul_B<true> and bn254_gt_tail_W<true>.
// The same record drives the segmented point fold of bn254_g{1,2}_msm_batch (bn254_g{1,2}_add_M<true>): dst = src[0] + ... + src[cnt-1]
// in Jacobian form, or the point at infinity for cnt == 0; `last` != 0 marks the piece that completes a segment, which is normalised.
struct BnSegPiece {
    const uint32_t *src;
    uint32_t *dst;
    uint32_t cnt, last;
};
// one piece of the segmented multi-pairing over prepared points (bn254_pairing_product_batch_prepared_native): `cnt` <= 4 consecutive pairs from
// pair `first` (relative to the sub-launch) share one Miller accumulator on a lane pair; cnt == 0 (an empty segment) gives one.
// Built on the host, read by bn254_miller_native_shared4_B<true>.
struct BnMillerPiece {
    uint32_t first, cnt;
};
// one piece of a sparse linear map over Fr (bn254_fr_dot_batch): `len` consecutive terms from term `first` on - or, in a fold level, `len`
// consecutive partial sums from scratch slot `first` on - are summed into record `dst` of the output (`to_out`) or of the scratch; len == 0
// (an empty segment) gives zero.  Two words: src = first (48 bits) | len << 48 (15 bits) | to_out << 63.  Built on the host
// (host_plan.hpp bn_dot_plan), read by the bodies of dot_ops.hpp.
struct BnDotPiece {
    uint64_t src, dst;
};
constexpr uint32_t BN_DOT_LEN_MAX = 0x7fffu;
BN_FN uint64_t dot_piece_first(const BnDotPiece &p) { return p.src & (((uint64_t)1 << 48) - 1); }
BN_FN uint32_t dot_piece_len(const BnDotPiece &p) { return (uint32_t)(p.src >> 48) & BN_DOT_LEN_MAX; }
BN_FN bool dot_piece_to_out(const BnDotPiece &p) { return (p.src >> 63) != 0; }
// one piece of a segmented scan over Fr (bn254_fr_scan_batch).  Three words: src = first (48 bits) | len << 48 (15 bits) | flag << 63, the
// segment, a scratch slot.  In the apply level (which the reduce level shares): `len` consecutive terms of segment `seg` from term `first` on
// (REVERSE: downwards), whose map goes to, and whose carry comes from, slot `slot`; flag: the piece is its whole segment and starts from
// init[seg].  In an up level: the maps of slots [first, first + len) composed into `slot`.  In a down level: the carries of slots
// [first, first + len) from the carry of `slot`, or - flag - from init[seg].  Built on the host (host_plan.hpp bn_scan_plan), read by the
// bodies of scan_ops.hpp.
struct BnScanPiece {
    uint64_t src, seg, slot;
};
BN_FN uint64_t scan_piece_first(const BnScanPiece &p) { return p.src & (((uint64_t)1 << 48) - 1); }
BN_FN uint32_t scan_piece_len(const BnScanPiece &p) { return (uint32_t)(p.src >> 48) & BN_DOT_LEN_MAX; }
BN_FN bool scan_piece_flag(const BnScanPiece &p) { return (p.src >> 63) != 0; }
// the products of one sumcheck round (bn254_fr_sumcheck_round): `groups` groups, group c = coeff[c] (eight words, a Montgomery image) times
// the len[c] tables table[c][0 .. len[c]).  The same for every lane: it travels as a kernel argument.  Built on the host
// (host_plan.hpp bn_sumcheck_desc, which checks the bounds), read by the round body of mle_ops.hpp.
constexpr uint32_t BN_SUMCHECK_GROUPS = 16, BN_SUMCHECK_FACTORS = 4;
struct BnSumcheckDesc {
    uint32_t coeff[BN_SUMCHECK_GROUPS][8];
    uint8_t table[BN_SUMCHECK_GROUPS][BN_SUMCHECK_FACTORS];
    uint8_t len[BN_SUMCHECK_GROUPS];
    uint32_t groups;
};
BN_FN bool words_all_zero(const uint32_t *w, int n) {
    uint32_t o = 0;
    for (int i = 0; i < n; ++i) o |= w[i];
    return o == 0;
}
// a raw 256-bit integer (8 words, little-endian word order) below q
BN_FN bool words_lt_q(const uint32_t *w) {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { int64_t s = (int64_t)w[i] - (int64_t)k::Q32[i] + br; br = s >> 32; }
    return br != 0;
}
#undef F2P
}  // namespace bn254
