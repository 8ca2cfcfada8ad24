// The per-lane bodies of the transforms over G1 and G2 (bn254_g{1,2}_ntt_batch; kernels: bn254_kernels_mul.hip, host: bn254_group_ntt.hip).
// A transform of n = 2^log_n points is log_n radix-2 Stockham stages (decimation in time) in global memory, so the data are in natural order
// before the first and after the last stage and nothing reverses bits.  Before stage i the array holds, for every residue rho < r = n / 2^i,
// the transform of length l = 2^i of the subsequence x[rho + r j] at A[rho + r k], k < l.  Stage i halves r (r' = r / 2) and doubles l:
//     A'[rho + r' k]       = A[rho + r k] + [w_2l^k] A[rho + r' + r k]
//     A'[rho + r' (k + l)] = A[rho + r k] - [w_2l^k] A[rho + r' + r k]                 rho < r', k < l
// One lane (G2: lane pair) per butterfly b = rho + r' k < n / 2: it writes records b and b + n / 2 - adjacent lanes adjacent records - and reads
// two records r' apart.  A stage reads one array and writes another (host_plan.hpp bn_group_ntt_group plans the buffers).
// The twiddle w_2l^k = w_n^(k r') comes from the factored root tables of bn254_fr_ntt_batch (ntt_ops.hpp ntt_root_power: two loads, one product;
// an inverse transform takes the powers of w^-1 from the same tables); the product [w] B is ONE GLV / GLS chain left in Jacobian form, as in the
// term kernels of the multi-scalar multiplications, and the sum and the difference are the COMPLETE addition (group_ops.hpp add_body): equal
// operands and opposite operands are ordinary here - a constant input doubles at every stage and cancels everywhere but at index 0.
// Stage 0 has l = 1: all its twiddles are one, and it runs no chain.  Points stay Jacobian between the stages; the call ends with the
// shared-inversion normalisation (normalize_body).
// A coset shift and the n^-1 of an inverse transform are one further pass of chains (group_ntt_scale_body): point j times s^j before the first
// stage, or times n^-1 s^-j after the last one, the scalars from the shift tables of bn254_fr_ntt_batch (ntt_shift_power); an inverse without
// a shift multiplies every point by the one scalar n^-1.
// Everything is pure and takes plain pointers and a lane (lane pair) index: the host simulation (tests/hostsim/hostsim_group_ntt.cpp) runs the
// same bodies over host arrays.
#pragma once
#include "group_ops.hpp"
#include "ntt_ops.hpp"

// template arguments of the kernels bn254_g{1,2}_add_M<Args>: in the unnamed namespace like the records of group_ops.hpp
namespace {
struct GroupNttStageArgs {   // butterflies [lo, lo + launch) of one stage over whole transforms laid back to back
    const uint32_t *src; uint32_t *dst; const uint32_t *wtbl; uint32_t log_n, stage, inverse, lo;
};
struct GroupNttScaleArgs {   // points [lo, lo + launch): dst[j] = [c] src[j], c = stbl's power for j mod n (per_point) or `scale`; dst may be src
    const uint32_t *src; uint32_t *dst; const uint32_t *stbl; uint32_t log_n, per_point, lo; bn254::Fr scale;
};
// what runs chains carries the window tables of its launch (640 B per lane); stage 0 is launched with the plain stage record
struct GroupNttChainArgs { GroupNttStageArgs st; uint4 *table; };
struct GroupNttPassArgs { GroupNttScaleArgs sc; uint4 *table; };
}  // namespace

namespace bn254 {
constexpr uint32_t GROUP_NTT_LOG_MAX = 22;     // BN254_GROUP_NTT_LOG_MAX
static_assert(GROUP_NTT_LOG_MAX <= NTT_LOG_MAX, "the twiddles are powers of the root tables' w_24");

// butterfly g of a stage, counted over all transforms of the launch's arrays: the records it reads (a, b) and writes (o0, o1) and the exponent
// of w_24 of its twiddle.  log_n >= 1.
struct GroupNttIdx { uint32_t a, b, o0, o1, e; };
BN_FN GroupNttIdx group_ntt_index(uint32_t log_n, uint32_t stage, uint32_t g) {
    const uint32_t hb = log_n - 1u, lr = hb - stage;                        // n / 2 = 2^hb butterflies per transform; r' = 2^lr
    const uint32_t base = (g >> hb) << log_n, bf = g & ((1u << hb) - 1u);
    const uint32_t rho = bf & ((1u << lr) - 1u), k = bf >> lr;
    GroupNttIdx x;
    x.a = base + rho + (k << (lr + 1u)); x.b = x.a + (1u << lr);
    x.o0 = base + bf; x.o1 = x.o0 + (1u << hb);
    x.e = (k << lr) << (NTT_LOG_MAX - log_n);                               // w_n^(k r') as a power of w_24: below 2^23
    return x;
}
// the chain of a group: GLV (G1) or GLS (G2) over the window table `tab`, the result left Jacobian
template <class Tab>
BN_FN Jac<FqField> group_ntt_chain(const Jac<FqField> &p, const uint32_t *raw, Tab &tab) { return scalar_mul_glv(p, raw, tab); }
template <class F2, class Tab>
BN_FN Jac<Fq2Field<F2>> group_ntt_chain(const Jac<Fq2Field<F2>> &p, const uint32_t *raw, Tab &tab) { return scalar_mul_gls<F2>(p, raw, tab); }
// (a + t, a - t) to the two outputs
template <class F>
BN_FN void group_ntt_butterfly(const GroupNttStageArgs &g, const GroupNttIdx &x, const Jac<F> &t, PointIo<F> io) {
    const Jac<F> a = io(g.src + (size_t)x.a * io.WORDS);
    const Jac<F> r0 = add_body<F>(a, t, 0);
    io(r0, g.dst + (size_t)x.o0 * io.WORDS);
    const Jac<F> r1 = add_body<F>(a, t, 1);
    io(r1, g.dst + (size_t)x.o1 * io.WORDS);
}
// stage 0: every twiddle is one
template <class F>
BN_FN void group_ntt_stage0_body(const GroupNttStageArgs &g, uint32_t i, PointIo<F> io) {
    const GroupNttIdx x = group_ntt_index(g.log_n, 0u, g.lo + i);
    const Jac<F> t = io(g.src + (size_t)x.b * io.WORDS);
    group_ntt_butterfly<F>(g, x, t, io);
}
// stages 1 .. log_n - 1: `a` is loaded behind the chain, so that it is not alive across it
template <class F, class Tab>
BN_FN void group_ntt_stage_body(const GroupNttStageArgs &g, uint32_t i, Tab &tab, PointIo<F> io) {
    const GroupNttIdx x = group_ntt_index(g.log_n, g.stage, g.lo + i);
    NttPass P = {};
    P.wtbl = g.wtbl; P.inverse = g.inverse;
    const Fr w = ntt_root_power(P, x.e);
    uint32_t raw[8];
    fr_from_mont(w.w, raw);
    const Jac<F> b = io(g.src + (size_t)x.b * io.WORDS);
    const Jac<F> t = group_ntt_chain(b, raw, tab);
    group_ntt_butterfly<F>(g, x, t, io);
}
// the pass of a shift or of an inverse
template <class F, class Tab>
BN_FN void group_ntt_scale_body(const GroupNttScaleArgs &g, uint32_t i, Tab &tab, PointIo<F> io) {
    const uint32_t j = g.lo + i;
    Fr c = g.scale;
    if (g.per_point) {
        NttPass P = {};
        P.stbl = g.stbl; P.log_n = g.log_n;
        c = ntt_shift_power(P, j & ((1u << g.log_n) - 1u));
    }
    uint32_t raw[8];
    fr_from_mont(c.w, raw);
    const Jac<F> p = io(g.src + (size_t)j * io.WORDS);
    const Jac<F> r = group_ntt_chain(p, raw, tab);
    io(r, g.dst + (size_t)j * io.WORDS);
}
}  // namespace bn254
