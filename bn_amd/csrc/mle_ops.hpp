// The per-lane bodies of the multilinear kernels over Fr (bn254_mle.hip): bn254_fr_mle_eq, bn254_fr_mle_fold, bn254_fr_sumcheck_round,
// bn254_fr_sumcheck_fold_round, bn254_fr_mle_quotients and their _dev twins.  A multilinear table of nv variables is 2^nv records; the record
// at index i is the value at the point whose variable j is bit j of i.  Several tables of one sumcheck are stored index-major: tables[i * k + j] is table j at index i.
//   eq      out[i] = prod_{j < nv} (bit j of i ? z[j] : 1 - z[j]): one lane per element, nv products, whatever the data
//   fold    out[i] = in[i] + r * (in[i + half] - in[i]): binds the MOST significant variable; lane i alone touches records i and i + half
//   round   for t = 0 .. D:  sum over i < h, over the groups c, of coeff[c] * prod_{j in group c} (T_j[i] + t (T_j[i + h] - T_j[i])).
//           There are `lanes` = ceil(h / P) lanes and lane l sums the at most P indices l, l + lanes, l + 2 lanes, .. below h, so that the lanes of
//           a wave read neighbouring rows; its D + 1 sums go to part[t * lanes + l] - or, with one lane, straight to out[t]
//   fold_round  the fold of n = 4 h2 rows by r and the round over the 2 h2 folded rows in one pass: the round's lanes over h2 indices; for
//           index i a lane folds rows (i, i + 2 h2) and (i + h2, i + 3 h2) of all k tables into rows i and i + h2 of the folded array, then
//           sums the groups over these two rows.  The folded array may be the tables: rows i and i + h2 belong to that lane alone
//   sum     levels of fan F over the partial sums (additions only), laid out [t][piece] before and after; the last level writes out[t]
//   quotients  the nv tables q_j of an opening at z, f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1}): from t = a, for j = nv - 1 down to 0 with
//           half = 2^j, q_j[i] = t[i + half] - t[i] and t[i] += z[j] q_j[i] - the fold by z[j], whose difference is kept.  One launch does RHO of
//           these levels in registers: a pass over a table of L records has L / 2^RHO lanes and lane i holds the records i + c L / 2^RHO
// so the length of a lane's serial chain is a constant of the plan, never a property of the data, and no lane waits for another: the order
// between the levels is the order of the launches on their stream.  Every product and every sum is canonical (fr.hpp), hence the bytes are
// those of the Python-integer sums however the indices are dealt out.  Everything is pure and takes plain pointers and a lane index, so the
// host simulation (tests/hostsim/hostsim_mle.cpp, hostsim_mle_open.cpp, hostsim_fold_round.cpp) runs the very same bodies over host arrays.
#pragma once
#include "fr_ops.hpp"
#include "io.hpp"

namespace bn254 {

// The shipped choices (plain constants; bn254_mle.hip carries a run-time override of the piece length for the sweep of tools/time_mle.py
// only).  Indices per lane of the round kernel: the rule fixed before measuring is "the fastest of 4 / 8 / 16 / 32 on four tables of 2^22
// entries at degree 3 ships"; that is 16 (0.668 / 0.629 / 0.612 / 0.770 ms, profiles/r17_mle.txt), which is also the fastest on one table of
// 2^24 entries and three times behind 4 on four tables of 2^16, where 2048 lanes leave most of the machine idle.  Partial sums per lane of a
// sum level: not swept.
constexpr uint32_t FR_SUMCHECK_PIECE = 16;
constexpr uint32_t FR_SUMCHECK_FAN = 16;
// Levels per launch of the quotient kernel, one of 1 / 2 / 3 / 4 (bn254_mle.hip carries a run-time override for the sweep of
// tools/time_mle_open.py only).  The rule fixed before measuring: the fastest on one table of 2^22 records ships, an instance that spills
// being out of the sweep.  None spills (52 / 86 / 150 / 265 registers) and 2 is the fastest (0.224 / 0.158 / 0.177 / 0.233 ms,
// profiles/r19_mle_open.txt), at 2^16 and 2^20 records as well.  Why the larger instances lose was not investigated.
constexpr uint32_t FR_MLE_QUOT_LEVELS = 2;
constexpr uint32_t FR_MLE_QUOT_LEVELS_MAX = 4;
// the profile scope of the quotient passes (a constant here: bn254_mle.hip names its scopes through it)
constexpr char FR_MLE_QUOT_SCOPE[] = "fr_mle_quotients";
// Indices per lane of the fused fold-then-round kernel (bn254_fr_sumcheck_fold_round; bn254_mle.hip carries a run-time override for the sweep
// of tools/time_fold_round.py and the tests).  The rule fixed before measuring is the round's: the fastest of 4 / 8 / 16 on four tables of
// 2^22 entries at degree 3 ships; that is 8 (0.605 / 0.595 / 0.671 ms, profiles/r20_fold_round.txt).  Below that size host_plan.hpp's
// bn_sumcheck_fold_piece halves it while the lanes do not fill the machine: 0.175 against 0.312 ms on four tables of 2^16, and at no swept size
// slower than the fixed 8, so the adaptive choice ships.
constexpr uint32_t FR_SUMCHECK_FOLD_PIECE = 8;
constexpr char FR_SUMCHECK_FOLD_ROUND_SCOPE[] = "fr_sumcheck_fold_round";

BN_FN void fr_mle_eq_body(const uint32_t *z, uint32_t nv, uint32_t *out, size_t i) {
    const Fr one = fr_one();
    Fr acc = one;
#pragma unroll 1
    for (uint32_t j = 0; j < nv; ++j) {
        const Fr zj = fr_load(z, j);
        acc = fr_mul(acc, fr_select(((i >> j) & 1) != 0, fr_sub(one, zj), zj));
    }
    fr_store(acc, out, i);
}
// out may be in: both records are read before record i is written, and no other lane touches either
BN_FN void fr_mle_fold_body(const uint32_t *in, const Fr &r, uint32_t *out, size_t half, size_t i) {
    const Fr lo = fr_load(in, i), hi = fr_load(in, i + half);
    fr_store(fr_add(lo, fr_mul(fr_sub(hi, lo), r)), out, i);
}
// one level over the 2 HC records a lane has left, record pair C and the pairs after it.  A recursion over template arguments, not a loop:
// every index into v is a constant whatever the unroller's budget makes of eight products in a row, so v stays in registers
template <int HC, int C = 0>
BN_FN void fr_mle_quotients_level(Fr *v, const Fr &zk, uint32_t *out, size_t at, size_t S) {
    if constexpr (C < HC) {
        const Fr q = fr_sub(v[C + HC], v[C]);
        fr_store(q, out, at + C * S);
        v[C] = fr_add(v[C], fr_mul(q, zk));
        fr_mle_quotients_level<HC, C + 1>(v, zk, out, at, S);
    }
}
// Lane i of a quotient pass of RHO levels over a table of 2^m records at src (m >= RHO), S = 2^(m - RHO) lanes.  The lane loads the 2^RHO
// records i + c S - all of them before it stores anything - and level k binds variable j = m - 1 - k by zz[k] = z[j]: among the 2^(RHO - k)
// records left, c and c + 2^(RHO - 1 - k) are index i + c S and its partner half = 2^j above.  The difference is q_j[i + c S], record
// 2^j + i + c S of the heap `out`; the sum is the folded record.  After RHO levels record i of the folded table goes to fold_dst[i] - the
// working table, which may be src (no other lane touches the records of this one), or, in the last pass (S == 1), out itself: record 0.
// At every load and store the lanes of a wave touch neighbouring records.
template <int RHO>
BN_FN void fr_mle_quotients_body(const uint32_t *src, const Fr *zz, uint32_t m, uint32_t *fold_dst, uint32_t *out, size_t i) {
    static_assert(RHO >= 1 && RHO <= (int)FR_MLE_QUOT_LEVELS_MAX, "one instance per number of levels");
    const size_t S = (size_t)1 << (m - RHO), top = (size_t)1 << (m - 1);
    Fr v[1 << RHO];
#pragma unroll
    for (int c = 0; c < (1 << RHO); ++c) v[c] = fr_load(src, i + c * S);
    fr_mle_quotients_level<(1 << (RHO - 1))>(v, zz[0], out, top + i, S);
    if constexpr (RHO > 1) fr_mle_quotients_level<(1 << (RHO - 2))>(v, zz[1], out, (top >> 1) + i, S);
    if constexpr (RHO > 2) fr_mle_quotients_level<(1 << (RHO - 3))>(v, zz[2], out, (top >> 2) + i, S);
    if constexpr (RHO > 3) fr_mle_quotients_level<(1 << (RHO - 4))>(v, zz[3], out, (top >> 3) + i, S);
    fr_store(v[0], fold_dst, i);
}

// Lane `lane` of a round over h indices of `tables` - the round kernel's and, with a fold in front of every index, the fused kernel's.
// pre(row_lo, row_hi) runs once per index before its rows are read: nothing for the round, the fold of the two rows for the fused call - the
// one function both bodies call, so the group walk exists once.  The factors of a group are walked one at a time: v = lo, d = hi - lo, and
// per t (unrolled: acc and prod have compile-time indices and stay in registers) prod[t] *= v, v += d - the values at t = 0, 1, 2, .. cost
// additions only.  The coefficient goes into the first factor's v and d: two products per group and index, not D + 1.  dst: part, or out
// when lanes == 1.
template <int D, class Pre>
BN_FN void fr_sumcheck_lane(const uint32_t *tables, uint64_t h, uint32_t k, const BnSumcheckDesc &desc, uint64_t lanes, uint32_t *dst, uint64_t lane,
                            const Pre &pre) {
    Fr acc[D + 1];
#pragma unroll
    for (int t = 0; t <= D; ++t) acc[t] = fr_zero();
#pragma unroll 1
    for (uint64_t i = lane; i < h; i += lanes) {
        const uint64_t row_lo = i * k, row_hi = (i + h) * k;
        pre(row_lo, row_hi);
#pragma unroll 1
        for (uint32_t c = 0; c < desc.groups; ++c) {
            Fr prod[D + 1];
            {
                const uint32_t j = desc.table[c][0];
                const Fr co = fr_const(desc.coeff[c]), lo = fr_load(tables, row_lo + j), hi = fr_load(tables, row_hi + j);
                Fr v = fr_mul(lo, co);
                const Fr d = fr_mul(fr_sub(hi, lo), co);
#pragma unroll
                for (int t = 0; t <= D; ++t) {
                    prod[t] = v;
                    if (t < D) v = fr_add(v, d);
                }
            }
#pragma unroll 1
            for (uint32_t f = 1; f < desc.len[c]; ++f) {
                const uint32_t j = desc.table[c][f];
                const Fr lo = fr_load(tables, row_lo + j), hi = fr_load(tables, row_hi + j);
                Fr v = lo;
                const Fr d = fr_sub(hi, lo);
#pragma unroll
                for (int t = 0; t <= D; ++t) {
                    prod[t] = fr_mul(prod[t], v);
                    if (t < D) v = fr_add(v, d);
                }
            }
#pragma unroll
            for (int t = 0; t <= D; ++t) acc[t] = fr_add(acc[t], prod[t]);
        }
    }
#pragma unroll
    for (int t = 0; t <= D; ++t) fr_store(acc[t], dst, t * lanes + lane);     // one lane: record t of out
}
template <int D>
BN_FN void fr_sumcheck_round_body(const uint32_t *tables, uint64_t h, uint32_t k, const BnSumcheckDesc &desc, uint64_t lanes, uint32_t *dst, uint64_t lane) {
    fr_sumcheck_lane<D>(tables, h, k, desc, lanes, dst, lane, [](uint64_t, uint64_t) {});
}
// Lane `lane` of the fused fold-then-round kernel over n = 4 h2 rows of k tables: the round's mapping over the h2 indices of the round that
// follows the fold.  For index i the lane first folds rows (i, i + 2 h2) and (i + h2, i + 3 h2) of every one of the k tables by r - two
// products per table, the fold's own - into rows i and i + h2 of `folded`, then walks the groups over those two rows: it reads back what it
// has just written itself, which program order makes visible.  No other lane reads or writes rows i and i + h2 of either array and rows
// >= 2 h2 are only read, so `folded` may be `tables` and no lane waits for another.  dst: part, or out when lanes == 1.
template <int D>
BN_FN void fr_sumcheck_fold_round_body(const uint32_t *tables, const Fr &r, uint32_t *folded, uint64_t h2, uint32_t k, const BnSumcheckDesc &desc, uint64_t lanes, uint32_t *dst,
                                       uint64_t lane) {
    const uint64_t up = 2 * h2 * k;
    fr_sumcheck_lane<D>(folded, h2, k, desc, lanes, dst, lane, [&](uint64_t row_lo, uint64_t row_hi) {
#pragma unroll 1
        for (uint32_t j = 0; j < k; ++j) {
            const Fr a0 = fr_load(tables, row_lo + j), a1 = fr_load(tables, row_hi + j), a2 = fr_load(tables, row_lo + up + j), a3 = fr_load(tables, row_hi + up + j);
            fr_store(fr_add(a0, fr_mul(fr_sub(a2, a0), r)), folded, row_lo + j);
            fr_store(fr_add(a1, fr_mul(fr_sub(a3, a1), r)), folded, row_hi + j);
        }
    });
}
// Lane `lane` of a sum level over `cnt` partial sums per t: with cnt2 = ceil(cnt / F), lane = t * cnt2 + i adds src[t * cnt + i F ..] (at most
// F of them) into dst[t * cnt2 + i]; the last level has cnt2 == 1 and its dst is out.  src and dst are different ranges of the scratch.
BN_FN void fr_sumcheck_sum_body(const uint32_t *src, uint64_t cnt, uint32_t F, uint32_t *dst, uint64_t lane) {
    const uint64_t cnt2 = (cnt + F - 1) / F, t = lane / cnt2, i = lane % cnt2, first = i * F;
    const uint32_t len = (uint32_t)(cnt - first < F ? cnt - first : F);
    Fr acc = fr_zero();
#pragma unroll 1
    for (uint32_t j = 0; j < len; ++j) acc = fr_add(acc, fr_load(src, t * cnt + first + j));
    fr_store(acc, dst, lane);
}

}  // namespace bn254
