// The per-lane bodies of the Poseidon kernels over Fr (bn254_poseidon.hip): bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch,
// bn254_fr_merkle_tree and their _dev twins.  The circomlib / iden3 instance: S-box x^5, width T = arity + 1 = 2 .. 5 (and the width 6 of babyjub_ops.hpp), R_F = 8 full rounds (four in
// front, four behind) around R_P = 56 / 57 / 56 / 60 (/ 60) partial ones; the constants are poseidon_constants.hpp (generated from bn_amd/poseidon.py).
//   round    s[i] += C[round * T + i];  s[i] = s[i]^5 for every i (full) or for i = 0 (partial);  s = M s
//   permute  the R_F + R_P rounds over a state of T records
//   hash     element 0 of permute([0, x_1 .. x_arity]); a Merkle node is hash(left, right), so a tree level is the hash of arity 2 over the
//            level below read as pairs
// One lane per permutation; the state stays in registers.  The loop over the rounds is NOT unrolled - a full round of T = 5 is 40 inlined
// products, about 60 KB of code, and the three loops (full, partial, full: the S-box choice is never a branch inside a round) already
// add up to more than the instruction cache holds - while everything inside a round is, so the state has compile-time indices.  The
// constants are addressed by the round counter alone: the address is the same in every lane of a wave.  fr_mul wants one canonical operand: the
// constants are, and so are every sum and every product, hence the bytes are those of the integer model.  Everything is pure and takes plain
// pointers and a lane index, so the host simulation (tests/hostsim/hostsim_poseidon.cpp) runs the very same bodies over host arrays.
#pragma once
#include "fr_ops.hpp"
#include "poseidon_constants.hpp"

namespace bn254 {

// Ends a scheduling region on the device (nothing on the host).  A full round of T = 5 is one basic block of 40 inlined products, and the
// instruction scheduler's time grows with the square of a region: one region per S-box and per matrix row compiles the T = 5 instance in
// 50 s instead of 214 s, and the T = 4 one with 139 VGPRs instead of 199.
// The matrix row: 1 = one fr_dot (fr.hpp: T product rows per word, one reduction), 0 = T products and T - 1 sums.  The rule was fixed before
// measuring - the fused row ships if its [min, max] of five runs lies wholly below the plain one's on 2^20 hashes of arity 2 - and it does:
// 7.10 ms [7.08 7.39] against 9.47 ms [9.46 10.72] (profiles/r18_poseidon.txt).  The switch stays for tools/time_poseidon.py --variants and for
// the host simulation, which runs both; the bytes are the same.
#ifndef BN254_POSEIDON_FUSED_ROW
#define BN254_POSEIDON_FUSED_ROW 1
#endif

#if defined(BN_HOSTSIM)
#define BN_PSD_REGION_END() ((void)0)
#else
#define BN_PSD_REGION_END() __builtin_amdgcn_sched_barrier(0)
#endif

template <int T>
BN_FN void fr_poseidon_add_constants(Fr (&s)[T], int round) {
#pragma unroll
    for (int i = 0; i < T; ++i) s[i] = fr_add(s[i], fr_const(psd::K<T>::C[round * T + i]));
}
BN_FN Fr fr_pow5(const Fr &x) {
    const Fr x2 = fr_mul(x, x);
    return fr_mul(fr_mul(x2, x2), x);
}
// The loops over the elements that hold products are written as compile-time recursions: with T = 3 already, a `#pragma unroll` loop of
// inlined products is larger than the compiler's limit for a pragma, stays a loop, and the state it indexes goes to private memory.
template <int T, int I = 0>
BN_FN void fr_poseidon_sbox_all(Fr (&s)[T]) {
    if constexpr (I < T) {
        s[I] = fr_pow5(s[I]);
        BN_PSD_REGION_END();
        fr_poseidon_sbox_all<T, I + 1>(s);
    }
}
// row I of M s: one fr_dot, or - BN254_POSEIDON_FUSED_ROW=0 - T products and T - 1 sums.  Both give the canonical value of the row, so the
// bytes do not depend on the choice.
template <int T, int I, int J = 1>
BN_FN Fr fr_poseidon_row_tail(const Fr (&s)[T], const Fr &acc) {
    if constexpr (J < T) return fr_poseidon_row_tail<T, I, J + 1>(s, fr_add(acc, fr_mul(s[J], fr_const(psd::K<T>::M[I * T + J]))));
    else return acc;
}
// Width 6 (the challenge of EdDSA-Poseidon, babyjub_ops.hpp; no public Poseidon call reaches it): fr_dot stops at five pairs because
// 5 r < 2^256 < 6 r, so a fused row is fr_dot<5> plus one product and one sum (BN254_POSEIDON_ROW6_SPLIT=0, shipped) or two fr_dot<3> and a
// sum (=1): 64 multiply-add rows per word either way, both canonical, the same bytes.  The host simulation runs both.
#ifndef BN254_POSEIDON_ROW6_SPLIT
#define BN254_POSEIDON_ROW6_SPLIT 0
#endif
template <int I>
BN_FN Fr fr_poseidon_row6(const Fr (&s)[6]) {
    const uint32_t (*m)[8] = psd::K<6>::M + I * 6;
#if BN254_POSEIDON_ROW6_SPLIT
    const Fr lo[3] = {s[0], s[1], s[2]}, hi[3] = {s[3], s[4], s[5]};
    return fr_add(fr_dot<3>(lo, m), fr_dot<3>(hi, m + 3));
#else
    const Fr lo[5] = {s[0], s[1], s[2], s[3], s[4]};
    return fr_add(fr_dot<5>(lo, m), fr_mul(s[5], fr_const(m[5])));
#endif
}
template <int T, int I = 0>
BN_FN void fr_poseidon_rows(const Fr (&s)[T], Fr (&n)[T]) {
    if constexpr (I < T) {
#if BN254_POSEIDON_FUSED_ROW
        if constexpr (T == 6) n[I] = fr_poseidon_row6<I>(s);
        else n[I] = fr_dot<T>(s, psd::K<T>::M + I * T);
#else
        n[I] = fr_poseidon_row_tail<T, I>(s, fr_mul(s[0], fr_const(psd::K<T>::M[I * T])));
#endif
        BN_PSD_REGION_END();
        fr_poseidon_rows<T, I + 1>(s, n);
    }
}
// s = M s
template <int T>
BN_FN void fr_poseidon_mix(Fr (&s)[T]) {
    Fr n[T];
    fr_poseidon_rows<T>(s, n);
#pragma unroll
    for (int i = 0; i < T; ++i) s[i] = n[i];
}
template <int T>
BN_FN void fr_poseidon_full_round(Fr (&s)[T], int round) {
    fr_poseidon_add_constants<T>(s, round);
    fr_poseidon_sbox_all<T>(s);
    fr_poseidon_mix<T>(s);
}
template <int T>
BN_FN void fr_poseidon_permute(Fr (&s)[T]) {
    constexpr int HALF = psd::R_F / 2, RP = psd::K<T>::R_P;
#pragma unroll 1
    for (int round = 0; round < HALF; ++round) fr_poseidon_full_round<T>(s, round);
#pragma unroll 1
    for (int round = HALF; round < HALF + RP; ++round) {
        fr_poseidon_add_constants<T>(s, round);
        s[0] = fr_pow5(s[0]);
        BN_PSD_REGION_END();
        fr_poseidon_mix<T>(s);
    }
#pragma unroll 1
    for (int round = HALF + RP; round < 2 * HALF + RP; ++round) fr_poseidon_full_round<T>(s, round);
}

// ---- the bodies: lane i of a launch
// hash:    out[i] = permute([0, in[i * (T - 1)] .. in[i * (T - 1) + T - 2]])[0].  A tree level: T = 3, in the level below, out the parents.
// permute: state i of T records; out may be in: the lane reads its T records before it writes them and touches no other lane's.
// ONE body for both, the choice a flag that is the same in every lane: the kernel holds one copy of the rounds per width.
template <int T>
BN_FN void fr_poseidon_body(const uint32_t *in, uint32_t *out, size_t i, bool hash) {
    Fr s[T];
    const size_t first = hash ? i * (T - 1) : i * T + 1;                       // of the records behind element 0
    s[0] = fr_zero();
    if (!hash) s[0] = fr_load(in, i * T);
#pragma unroll
    for (int j = 1; j < T; ++j) s[j] = fr_load(in, first + (j - 1));
    fr_poseidon_permute<T>(s);
    if (hash) { fr_store(s[0], out, i); return; }
#pragma unroll
    for (int j = 0; j < T; ++j) fr_store(s[j], out, i * T + j);
}
template <int T>
BN_FN void fr_poseidon_permute_body(const uint32_t *in, uint32_t *out, size_t i) { fr_poseidon_body<T>(in, out, i, false); }
template <int T>
BN_FN void fr_poseidon_hash_body(const uint32_t *in, uint32_t *out, size_t i) { fr_poseidon_body<T>(in, out, i, true); }

}  // namespace bn254
