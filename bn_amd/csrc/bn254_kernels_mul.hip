// G * Fr kernels of the BN254 engine for MI355X (gfx950): `Mul<Fr> for G<P>` (src/groups/mod.rs:250-270) batched.
//   bn254_g1_mul_M   one lane per point (G1 is over Fq: a Jacobian point is 27 VGPRs)
//   bn254_g2_mul_M   one point per lane PAIR (Fq2B: even lane = c0, odd lane = c1 of every coordinate, DPP exchange)
// normalize = 0 runs the reference's own double-and-add chain (raw Jacobian limbs identical to the crate's, used to make
// benchmark inputs with z != 1); normalize = 1 returns the normalized point by the short chains of curve.hpp: GLV (G1) / GLS (G2)
// decomposition, signed 4-bit windows, a window table brought to a common z so that every addition is a mixed one.
//
// This translation unit inlines the point operations and the multiplier leaves: the running point stays in registers for the
// whole chain (in the call-based build of bn254_hip.hip every doubling went through private memory: 6 / 27 GB of HBM traffic
// per 2^16 G1 / G2 multiplications).  Only the 16-entry window table is a per-lane array in private memory.
#define BN_INLINE_ALL 1       // fe.hpp: leaves and Fq6/Fq12-sized steps force-inlined
#define BN_MUL_WAVES 3        // resident waves per SIMD the G1 kernels are compiled for (168 VGPRs, 7 spilled; 2: equal since round 6's single launch, 4: 72 spilled, -2.5 %: profiles/r06_ab_mul_launch_size.txt)
#include <hip/hip_runtime.h>
#include <type_traits>
// The G2 kernel runs two resident waves per SIMD like the lane-pair pairing kernels, and the same ONE hand-over of the issue priority keeps both
// alive to the end (bn254_kernels_b.hip bn_fair_handover; the hardware's oldest-first arbitration lets the older wave leave early and the younger
// one finish alone): 2^16 / 2^17 / 2^18 G2 multiplications per call 33.5 / 35.1 / 36.1 -> 35.7 / 36.6 / 36.9 M/s (profiles/r06_ab_mul_launch_size.txt).
// Called from the window loop of scalar_mul_gls only (curve.hpp BN_MUL_HOOK); the G1 kernels run three waves per SIMD and keep the default.
__device__ __forceinline__ void bn_mul_fair_handover(int step, int total) {
    const uint32_t slot = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 4) & 1;      // HW_ID.wave_id
    if (slot == 0) { if (step * 1000 < 769 * total) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(0); }
    else { if (step * 1000 < 231 * total) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(2); }
}
#define BN_MUL_HOOK(step, total) bn_mul_fair_handover(step, total)
// The G1 kernel (three resident waves per SIMD, oldest first) ends a launch with every SIMD draining its last waves one after the other.  In the
// LAST resident round of a multi-round launch (the last 3 x 4 x 256 workgroups: MI355X; elsewhere the policy is merely mis-sized) a wave lowers
// its own priority as it advances, so the three share the SIMD by progress and finish together: +0.9 ... +1.6 % at 2^20 per launch
// (profiles/r06_ab_mul_launch_size.txt).  Single-round launches keep the default (waves of one age in lockstep are slower).
constexpr unsigned BN_G1_RESIDENT_WAVES = BN_MUL_WAVES * 4 * 256;
__device__ __forceinline__ void bn_g1_tail_policy(int step, int total) {
    if (gridDim.x >= 2 * BN_G1_RESIDENT_WAVES && blockIdx.x + BN_G1_RESIDENT_WAVES >= gridDim.x) {
        const int q = step * 4 / total;
        if (q == 0) __builtin_amdgcn_s_setprio(3); else if (q == 1) __builtin_amdgcn_s_setprio(2); else if (q == 2) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
    }
}
#define BN_G1_HOOK(step, total) bn_g1_tail_policy(step, total)
#include "group_ops.hpp"       // the per-lane bodies of everything below but the chains of curve.hpp: shared with the host simulation
#include "group_ntt_ops.hpp"   // ... and those of the transforms over G1 / G2
#include "lane_launch.hpp"     // the shell and the launchers of the integer kernels

using namespace bn254;

namespace {
constexpr int BLOCK = 64;
typedef Fq2B<Fe> F2;
typedef FqField G1F;
typedef Fq2Field<F2> G2F;

// The G2 kernels with a fixed argument list keep both lanes of every pair active for the DPP exchanges: a pair past the end works on the
// last element again (both lanes of a pair share it: the exchanges never meet a retired partner) and stores nothing.
struct LanePair { uint32_t pair; bool live; };
__device__ __forceinline__ LanePair lane_pair_clamped(uint32_t t, uint32_t n) {
    const bool live = (t >> 1) < n;
    return {live ? t >> 1 : n - 1, live};
}

// NORMALIZE is a template parameter, i.e. each flavour is its OWN kernel: with a run-time flag the reference chain and the GLV /
// windowed chain were register-allocated together (round 2: 74 spilled VGPRs in the G1 kernel).
// KEEP_JAC (the term kernels of bn254_g{1,2}_msm_batch): the fast chain WITHOUT jac_normalize - the sum of a segment is normalised once.
template <class F, bool NORMALIZE, bool KEEP_JAC = false>
__device__ __forceinline__ Jac<F> run_chain(const Jac<F> &p, const uint32_t *km, uint4 *table, uint32_t lane) {
    uint32_t raw[8];
    fr_load_raw(km, raw);
    if constexpr (NORMALIZE) {
#ifdef BN_AB_ALIAS_SCRATCH
        // TIMING EXPERIMENT ONLY (wrong results): all waves use the tables of the first 64 lanes (40 KB: cache resident) - the same
        // instruction stream without the HBM traffic of 640 B of table per lane
        AffTableMem<F> tab = {table + (size_t)(lane & 63u) * AFF_LANE_U4};
#else
        AffTableMem<F> tab = {table + (size_t)lane * AFF_LANE_U4};
#endif
        if constexpr (KEEP_JAC) {
            if constexpr (std::is_same<F, FqField>::value) return scalar_mul_glv(p, raw, tab);
            else return scalar_mul_gls<F2>(p, raw, tab);
        } else if constexpr (std::is_same<F, FqField>::value) return jac_normalize<F>(scalar_mul_glv(p, raw, tab));      // G1: GLV + signed windows
        else return jac_normalize<F>(scalar_mul_gls<F2>(p, raw, tab));                                             // G2: GLS, four signed-window streams
    } else {
        return scalar_mul_reference_chain<F>(p, raw);
    }
}

template <bool NORMALIZE, bool KEEP_JAC = false>
__device__ __forceinline__ void g1_mul_body(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n, uint4 *table) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    const PointIo<G1F> io;
    Jac<G1F> pt = io(p + io.WORDS * idx);
    Jac<G1F> r = run_chain<G1F, NORMALIZE, KEEP_JAC>(pt, k + 8u * idx, table, idx);
    io(r, out + io.WORDS * idx);
}
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BN_MUL_WAVES, BN_MUL_WAVES))) bn254_g1_mul_M(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n, uint4 *table) {
    g1_mul_body<true>(p, k, out, n, table);
}
// The term kernel of bn254_g1_msm_batch: out[i] = p[i] * k[i] by the same GLV chain, left in JACOBIAN form (any representation of the
// group element; infinity as z = 0) for the segmented fold below, which normalises once per segment.  A template beside the plain kernel,
// whose name and body stay as they are.
template <bool JACOBIAN>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BN_MUL_WAVES, BN_MUL_WAVES))) bn254_g1_mul_M(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n, uint4 *table) {
    g1_mul_body<true, JACOBIAN>(p, k, out, n, table);
}
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BN_MUL_WAVES, BN_MUL_WAVES))) bn254_g1_mul_chain_M(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n) {
    g1_mul_body<false>(p, k, out, n, nullptr);
}

template <bool NORMALIZE, bool KEEP_JAC = false>
__device__ __forceinline__ void g2_mul_body(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n, uint4 *table) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const LanePair lp = lane_pair_clamped(t, n);
    const PointIo<G2F> io;
    Jac<G2F> pt = io(p + io.WORDS * lp.pair);
    Jac<G2F> r = run_chain<G2F, NORMALIZE, KEEP_JAC>(pt, k + 8u * lp.pair, table, t);
    if (lp.live) io(r, out + io.WORDS * lp.pair);
}
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) bn254_g2_mul_M(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n, uint4 *table) {
    g2_mul_body<true>(p, k, out, n, table);
}
// the term kernel of bn254_g2_msm_batch (see bn254_g1_mul_M<JACOBIAN>)
template <bool JACOBIAN>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) bn254_g2_mul_M(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n, uint4 *table) {
    g2_mul_body<true, JACOBIAN>(p, k, out, n, table);
}
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) bn254_g2_mul_chain_M(const uint32_t *p, const uint32_t *k, uint32_t *out, uint32_t n) {
    g2_mul_body<false>(p, k, out, n, nullptr);
}
// a[i] + b[i] or a[i] - b[i] (group_ops.hpp add_body)
__global__ void __launch_bounds__(BLOCK) bn254_g1_add_M(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t n, int negate_b) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    const PointIo<G1F> io;
    const uint32_t *wa = a + io.WORDS * idx, *wb = b + io.WORDS * idx;
    Jac<G1F> pa = io(wa), pb = io(wb);
    Jac<G1F> r = add_body<G1F>(pa, pb, negate_b);
    io(r, out + io.WORDS * idx);
}
__global__ void __launch_bounds__(BLOCK) bn254_g2_add_M(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t n, int negate_b) {
    const LanePair lp = lane_pair_clamped(blockIdx.x * BLOCK + threadIdx.x, n);
    const PointIo<G2F> io;
    const uint32_t *wa = a + io.WORDS * lp.pair, *wb = b + io.WORDS * lp.pair;
    Jac<G2F> pa = io(wa), pb = io(wb);
    Jac<G2F> r = add_body<G2F>(pa, pb, negate_b);
    if (lp.live) io(r, out + io.WORDS * lp.pair);
}
// One level of the segmented fold of bn254_g{1,2}_msm_batch (group_ops.hpp msm_fold_body): lane (G2: lane pair) i folds pieces[i].
// Instances of the names bn254_g{1,2}_add_M beside the plain kernels; `SEG` is always true.
template <bool SEG>
__global__ void __launch_bounds__(BLOCK) bn254_g1_add_M(const BnSegPiece *pieces, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    const BnSegPiece pc = pieces[idx];
    Jac<G1F> r = msm_fold_body<G1F>(pc);
    PointIo<G1F>()(r, pc.dst);
}
template <bool SEG>
__global__ void __launch_bounds__(BLOCK) bn254_g2_add_M(const BnSegPiece *pieces, uint32_t n) {
    const LanePair lp = lane_pair_clamped(blockIdx.x * BLOCK + threadIdx.x, n);
    const BnSegPiece pc = pieces[lp.pair];
    Jac<G2F> r = msm_fold_body<G2F>(pc);
    if (lp.live) PointIo<G2F>()(r, pc.dst);
}

// ---- the integer kernels of the bucket method (group_ops.hpp describes the method and holds its point bodies), Ops of lane_launch.hpp's
// bn254_fr_decode_k with workgroups of 256 lanes (they take the canonical integer of a scalar apart); they need a wave or a workgroup, so they
// have no twin in the host simulation.
// COUNT: counts[key] += 1 for every non-zero digit of k[0..n); SCATTER: the same walk, (index, key) written at cursor[key]++ (the scanned counts).
// When every active lane of a wave holds the same digit (equal scalars: the skew case) one lane adds for all of them; large groups of
// equal digits inside a wave are served the same way.
struct MsmDigitsOp {
    const uint32_t *k; uint32_t n, c, W; uint32_t *counts; uint32_t *idx, *keys; int scatter;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * 256 + threadIdx.x;
        if (i >= n) return;
        uint32_t raw[8];
        fr_load_raw(k + 8u * i, raw);
        const uint64_t active = __ballot(1);
        const uint32_t lane = __lane_id(), leader = (uint32_t)__ffsll((unsigned long long)active) - 1u;
        const uint32_t rank = (uint32_t)__popcll(active & ((1ull << lane) - 1ull)), total = (uint32_t)__popcll(active);
#pragma unroll 1
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t d = msm_digit(raw, w, c), first = (uint32_t)__shfl((int)d, (int)leader);
            const uint32_t key = (w << c) + d;
            uint32_t pos = 0;
            if (__all(d == first)) {                                   // wave-uniform
                if (d && lane == leader) pos = atomicAdd(&counts[key], total);
                pos = (uint32_t)__shfl((int)pos, (int)leader) + rank;
            } else {
                // lanes that share a digit with the first lane not yet served add through ONE atomic (a short top window has a handful of
                // buckets that every term hits: 2^20 atomics on three addresses otherwise); after two groups of fewer than three lanes -
                // the usual case, random digits in a wide window - the rest add for themselves
                bool done = d == 0;
                uint64_t rem = __ballot(!done);
                for (int small = 0; rem && small < 2;) {
                    const uint32_t lead = (uint32_t)__ffsll((unsigned long long)rem) - 1u, dl = (uint32_t)__shfl((int)d, (int)lead);
                    const bool mine = !done && d == dl;
                    const uint64_t m = __ballot(mine);
                    rem &= ~m;
                    const uint32_t cnt = (uint32_t)__popcll(m);
                    if (cnt < 3) { ++small; continue; }
                    uint32_t base = 0;
                    if (lane == lead) base = atomicAdd(&counts[(w << c) + dl], cnt);
                    base = (uint32_t)__shfl((int)base, (int)lead);
                    if (mine) { pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); done = true; }
                }
                if (!done) pos = atomicAdd(&counts[key], 1u);
            }
            if (scatter && d) { idx[pos] = i; keys[pos] = key; }
        }
    }
};
// The same walk over the signed digits of a call against prepared bases (group_ops.hpp msm_signed_digit): ONE set of 2^(c-1) buckets for all
// windows, key = |d| - 1; the entry written for term i and window w is the table index w * count + first + i, MSM_NEG set for d < 0.
struct MsmSignedDigitsOp {
    const uint32_t *k; uint32_t n, c, W, count, first; uint32_t *counts; uint32_t *idx, *keys; int scatter;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * 256 + threadIdx.x;
        if (i >= n) return;
        uint32_t raw[8];
        fr_load_raw(k + 8u * i, raw);
        const uint64_t active = __ballot(1);
        const uint32_t lane = __lane_id(), leader = (uint32_t)__ffsll((unsigned long long)active) - 1u;
        const uint32_t rank = (uint32_t)__popcll(active & ((1ull << lane) - 1ull)), total = (uint32_t)__popcll(active);
        uint32_t carry = 0;
#pragma unroll 1
        for (uint32_t w = 0; w < W; ++w) {
            bool neg;
            const uint32_t d = msm_signed_digit(raw, w, c, carry, neg), first_d = (uint32_t)__shfl((int)d, (int)leader);
            const uint32_t key = d - 1u;                               // used for d != 0 only
            uint32_t pos = 0;
            if (__all(d == first_d)) {                                 // wave-uniform
                if (d && lane == leader) pos = atomicAdd(&counts[key], total);
                pos = (uint32_t)__shfl((int)pos, (int)leader) + rank;
            } else {
                // groups of equal digits inside a wave add through ONE atomic, as in MsmDigitsOp
                bool done = d == 0;
                uint64_t rem = __ballot(!done);
                for (int small = 0; rem && small < 2;) {
                    const uint32_t lead = (uint32_t)__ffsll((unsigned long long)rem) - 1u, dl = (uint32_t)__shfl((int)d, (int)lead);
                    const bool mine = !done && d == dl;
                    const uint64_t m = __ballot(mine);
                    rem &= ~m;
                    const uint32_t cnt = (uint32_t)__popcll(m);
                    if (cnt < 3) { ++small; continue; }
                    uint32_t base = 0;
                    if (lane == lead) base = atomicAdd(&counts[dl - 1u], cnt);
                    base = (uint32_t)__shfl((int)base, (int)lead);
                    if (mine) { pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); done = true; }
                }
                if (!done) pos = atomicAdd(&counts[key], 1u);
            }
            if (scatter && d) { idx[pos] = (w * count + first + i) | (neg ? MSM_NEG : 0u); keys[pos] = key; }
        }
    }
};
// exclusive scan of `total` counts in place, three launches: mode 0 - the sum of every tile; 1 - ONE workgroup scans the (at most 1024) tile
// sums and writes the grand total to *n0; 2 - every tile scans its counts from its base
struct MsmScanOp {
    uint32_t *counts; uint32_t total; uint32_t *tiles; uint32_t *n0; int mode;
    __device__ __forceinline__ void operator()() const {
        __shared__ uint32_t sh[256];
        const uint32_t t = threadIdx.x;
        uint32_t *v = mode == 1 ? tiles : counts + (size_t)blockIdx.x * MSM_TILE;
        const uint32_t len = mode == 1 ? (total + MSM_TILE - 1) / MSM_TILE : min(MSM_TILE, total - blockIdx.x * MSM_TILE);
        uint32_t x[4], s = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) { x[j] = 4 * t + j < len ? v[4 * t + j] : 0u; s += x[j]; }
        sh[t] = s;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            const uint32_t a = t >= off ? sh[t - off] : 0u;
            __syncthreads();
            sh[t] += a;
            __syncthreads();
        }
        if (mode == 0) { if (t == 255) tiles[blockIdx.x] = sh[255]; return; }
        uint32_t run = sh[t] - s + (mode == 2 ? tiles[blockIdx.x] : 0u);
        if (mode == 1 && t == 255) *n0 = sh[255];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) { if (4 * t + j < len) v[4 * t + j] = run; run += x[j]; }
    }
};

// The table build of the fixed-base multiplication after the shipped normalising kernel (bn254_g{1,2}_mul_M over the tiled base and the
// host-known scalars d * 2^(c w)): tile - record j of `out` = the one point at `src`; repack - thread t turns component t % comps of the
// normalised point t / comps into its 80-byte record.  Ops of bn254_fr_decode_k like the other integer kernels of this unit.
struct BaseTileOp {
    const uint32_t *src; uint32_t *out; uint32_t words, n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t t = blockIdx.x * 256 + threadIdx.x;
        if (t >= n * words) return;
        out[t] = src[t % words];
    }
};
struct BaseRepackOp {
    const uint32_t *pts; uint4 *table; uint32_t comps, n;                     // comps: 1 (G1) or 2 (G2)
    __device__ __forceinline__ void operator()() const {
        const uint32_t t = blockIdx.x * 256 + threadIdx.x;
        if (t >= n * comps) return;
        const uint32_t e = t / comps, comp = t % comps;
        const uint32_t *p = pts + (size_t)e * PointIo<G1F>::WORDS * comps;
        const Fe x = fe_from_u32x8(p + 8u * comp), y = fe_from_u32x8(p + 8u * comps + 8u * comp);
        uint32_t z = 0;                                                      // normalised: z is one, or zero at infinity (canonical words)
        for (uint32_t j = 0; j < 8u * comps; ++j) z |= p[16u * comps + j];
        aff_record_pack(x, y, z == 0 ? 1u : 0u, table, (size_t)t);
    }
};
// The generic point kernels: lane (G2: lane pair) i < n runs the body that belongs to `Args` (group_ops.hpp).  A lane pair past n retires as a
// whole - the bodies return early themselves (a lane past a level's entries), both lanes of a pair alike, so nothing here is clamped.
template <class F> __device__ __forceinline__ void msm_point_op(const MsmAccArgs &g, uint32_t i) { msm_acc_body<F>(g, i); }
template <class F> __device__ __forceinline__ void msm_point_op(const MsmReduceArgs &g, uint32_t i) { msm_reduce_body<F>(g, i); }
template <class F> __device__ __forceinline__ void msm_point_op(const MsmAccPrepArgs &g, uint32_t i) {
    msm_acc_prep_body<F>(g, i, BaseTableMem<F>{g.table, std::is_same<F, G1F>::value ? 0u : threadIdx.x & 1u});
}
template <class F> __device__ __forceinline__ void msm_point_op(const MsmPrepDoubleArgs &g, uint32_t i) { msm_prep_double_body<F>(g, i, PointIo<F>()); }
template <class F> __device__ __forceinline__ void msm_point_op(const BaseMulArgs &g, uint32_t i) {
    base_mul_body<F>(g, i, BaseTableMem<F>{g.table, std::is_same<F, G1F>::value ? 0u : threadIdx.x & 1u}, PointIo<F>());
}
// the normalisation: lane (lane pair) i owns the run of NORM_RUN points from i * NORM_RUN on; both lanes of a pair walk the same run
template <class F> __device__ __forceinline__ void msm_point_op(const NormalizeArgs &g, uint32_t i) {
    normalize_body<F>(g, i, NORM_RUN, PrefixMem<F>{g.prefix, std::is_same<F, G1F>::value ? 0u : threadIdx.x & 1u}, PointIo<F>());
}
// the comparison: one int32 per pair of points, stored by the lane (G2: the even lane of the pair)
template <class F> __device__ __forceinline__ void msm_point_op(const EqArgs &g, uint32_t i) {
    const PointIo<F> io;
    const int32_t r = eq_body<F>(io(g.a + (size_t)i * io.WORDS), io(g.b + (size_t)i * io.WORDS));
    if (std::is_same<F, G1F>::value || !(threadIdx.x & 1u)) g.out[i] = r;
}
template <class Args>
__global__ void __launch_bounds__(BLOCK) bn254_g1_add_M(Args g, uint32_t n) {
    const uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx < n) msm_point_op<G1F>(g, idx);
}
template <class Args>
__global__ void __launch_bounds__(BLOCK) bn254_g2_add_M(Args g, uint32_t n) {
    const uint32_t pair = (blockIdx.x * BLOCK + threadIdx.x) >> 1;
    if (pair < n) msm_point_op<G2F>(g, pair);
}

// ---- the transforms over G1 / G2 (bn254_g{1,2}_ntt_batch, group_ntt_ops.hpp): lane (G2: lane pair) i < n of a launch is butterfly lo + i of a
// stage, or point lo + i of a shift / inverse pass - further instances of the generic point kernels bn254_g{1,2}_add_M<Args> below (a lane
// pair past n retires as a whole).  What runs a chain keeps its window table in the launch's scratch like the term kernels
// (`table`: bn254_mul_table_bytes_M(g, n) bytes, one table per lane); the hand-over hooks of the chains are those of this unit.
template <class F> __device__ __forceinline__ AffTableMem<F> group_ntt_table(uint4 *table, uint32_t i) {
    const uint32_t lane = std::is_same<F, G1F>::value ? i : 2u * i + (threadIdx.x & 1u);
    return {table + (size_t)lane * AFF_LANE_U4};
}
template <class F> __device__ __forceinline__ void msm_point_op(const GroupNttStageArgs &g, uint32_t i) { group_ntt_stage0_body<F>(g, i, PointIo<F>()); }
template <class F> __device__ __forceinline__ void msm_point_op(const GroupNttChainArgs &g, uint32_t i) {
    AffTableMem<F> tab = group_ntt_table<F>(g.table, i);
    group_ntt_stage_body<F>(g.st, i, tab, PointIo<F>());
}
template <class F> __device__ __forceinline__ void msm_point_op(const GroupNttPassArgs &g, uint32_t i) {
    AffTableMem<F> tab = group_ntt_table<F>(g.table, i);
    group_ntt_scale_body<F>(g.sc, i, tab, PointIo<F>());
}
// Every launch of a group kernel: one lane per G1 element, one lane pair per G2 element, BLOCK lanes per workgroup
unsigned group_grid(int g, size_t n) { return (unsigned)(((g == 1 ? n : 2 * n) + BLOCK - 1) / BLOCK); }
template <class... A>
int launch_group(int g, size_t n, hipStream_t s, void (*k1)(A...), void (*k2)(A...), A... a) {
    hipLaunchKernelGGL(g == 1 ? k1 : k2, dim3(group_grid(g, n)), dim3(BLOCK), 0, s, a...);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" {
int bn254_launch_g1_add_M(const void *a, const void *b, void *out, size_t n, int negate_b, hipStream_t s) { return launch_group(1, n, s, bn254_g1_add_M, bn254_g2_add_M, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, (uint32_t)n, negate_b); }
int bn254_launch_g2_add_M(const void *a, const void *b, void *out, size_t n, int negate_b, hipStream_t s) { return launch_group(2, n, s, bn254_g1_add_M, bn254_g2_add_M, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, (uint32_t)n, negate_b); }
// `table` (normalize != 0 only): bn254_mul_table_bytes_M(g, n) bytes of scratch for the window tables of this launch
size_t bn254_mul_table_bytes_M(int g, size_t n) { return (size_t)group_grid(g, n) * BLOCK * AFF_LANE_U4 * sizeof(uint4); }
static int launch_mul(int g, const void *p, const void *k, void *out, size_t n, int normalize, void *table, hipStream_t s) {
    if (normalize) return launch_group(g, n, s, bn254_g1_mul_M, bn254_g2_mul_M, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n, (uint4 *)table);
    return launch_group(g, n, s, bn254_g1_mul_chain_M, bn254_g2_mul_chain_M, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n);
}
int bn254_launch_g1_mul_M(const void *p, const void *k, void *out, size_t n, int normalize, void *table, hipStream_t s) { return launch_mul(1, p, k, out, n, normalize, table, s); }
int bn254_launch_g2_mul_M(const void *p, const void *k, void *out, size_t n, int normalize, void *table, hipStream_t s) { return launch_mul(2, p, k, out, n, normalize, table, s); }
// bn254_g{1,2}_msm_batch: the term kernel (Jacobian results, `table` as above) and one level of the segmented fold (`count` pieces in device memory)
int bn254_launch_msm_mul_M(int g, const void *p, const void *k, void *out, size_t n, void *table, hipStream_t s) { return launch_group(g, n, s, bn254_g1_mul_M<true>, bn254_g2_mul_M<true>, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n, (uint4 *)table); }
int bn254_launch_msm_fold_M(int g, const void *pieces, size_t count, hipStream_t s) { return launch_group(g, count, s, bn254_g1_add_M<true>, bn254_g2_add_M<true>, (const BnSegPiece *)pieces, (uint32_t)count); }
// bn254_g{1,2}_msm, bucket route.  n terms (< 2^32 / W entries in all), window width c, W windows.
// digits: scatter == 0 counts the terms per key into `counts` (zeroed by the caller); scatter != 0 writes (index, key) at the scanned counts
int bn254_launch_msm_digits_M(const void *k, size_t n, unsigned c, unsigned W, void *counts, void *idx, void *keys, int scatter, hipStream_t s) {
    const MsmDigitsOp op = {(const uint32_t *)k, (uint32_t)n, c, W, (uint32_t *)counts, (uint32_t *)idx, (uint32_t *)keys, scatter};
    return bn_lane_launch<256>(op, n, s);
}
// counts[0..total) -> their exclusive scan in place, the grand total to *n0; total <= 2^20, `tiles`: 1024 words of scratch
int bn254_launch_msm_scan_M(void *counts, size_t total, void *tiles, void *n0, hipStream_t s) {
    const unsigned blocks = (unsigned)((total + MSM_TILE - 1) / MSM_TILE);
    if (blocks == 0 || blocks > MSM_TILE) return (int)hipErrorInvalidValue;
    for (int mode = 0; mode < 3; ++mode) {
        const MsmScanOp op = {(uint32_t *)counts, (uint32_t)total, (uint32_t *)tiles, (uint32_t *)n0, mode};
        if (int rc = bn_block_launch<256>(op, mode == 1 ? 1u : blocks, 0, s)) return rc;
    }
    return (int)hipSuccess;
}
unsigned bn254_msm_piece_M(void) { return MSM_PIECE; }
// one accumulation level over `lanes` lanes (G2: lane pairs); idx != NULL only at level 0
int bn254_launch_msm_bucket_M(int g, const void *pts, const void *idx, const void *keys, const void *n0, unsigned level, void *out_pts, void *out_keys, void *buckets,
                              size_t lanes, hipStream_t s) {
    const MsmAccArgs a = {(const uint32_t *)pts, (const uint32_t *)idx, (const uint32_t *)keys, (const uint32_t *)n0, level, (uint32_t *)out_pts, (uint32_t *)out_keys, (uint32_t *)buckets};
    return launch_group(g, lanes, s, bn254_g1_add_M<MsmAccArgs>, bn254_g2_add_M<MsmAccArgs>, a, (uint32_t)lanes);
}
// the bucket reduction: count = W * groups lanes (lane pairs), terms = 2 * count points
int bn254_launch_msm_reduce_M(int g, const void *buckets, unsigned G, unsigned groups, unsigned c, size_t count, void *terms, hipStream_t s) {
    const MsmReduceArgs a = {(const uint32_t *)buckets, G, groups, c, (uint32_t)count, (uint32_t *)terms};
    return launch_group(g, count, s, bn254_g1_add_M<MsmReduceArgs>, bn254_g2_add_M<MsmReduceArgs>, a, (uint32_t)count);
}
// bn254_g{1,2}_msm_prepared.  digits: as above over the signed digits - `count` points in the handle, term i of this launch is point first + i;
// counts: 2^(c-1) words
int bn254_launch_msmp_digits_M(const void *k, size_t n, unsigned c, unsigned W, size_t count, size_t first, void *counts, void *idx, void *keys, int scatter, hipStream_t s) {
    const MsmSignedDigitsOp op = {(const uint32_t *)k, (uint32_t)n, c, W, (uint32_t)count, (uint32_t)first, (uint32_t *)counts, (uint32_t *)idx, (uint32_t *)keys, scatter};
    return bn_lane_launch<256>(op, n, s);
}
// level 0 of the accumulation over the handle's table, `lanes` lanes (G2: lane pairs)
int bn254_launch_msmp_bucket_M(int g, const void *table, const void *idx, const void *keys, const void *n0, void *out_pts, void *out_keys, void *buckets, size_t lanes, hipStream_t s) {
    const MsmAccPrepArgs a = {(const uint4 *)table, (const uint32_t *)idx, (const uint32_t *)keys, (const uint32_t *)n0, (uint32_t *)out_pts, (uint32_t *)out_keys, (uint32_t *)buckets};
    return launch_group(g, lanes, s, bn254_g1_add_M<MsmAccPrepArgs>, bn254_g2_add_M<MsmAccPrepArgs>, a, (uint32_t)lanes);
}
// a table build's window step: the n Jacobian points at d_pts doubled c times in place
int bn254_launch_msmp_double_M(int g, void *d_pts, unsigned c, size_t n, hipStream_t s) {
    const MsmPrepDoubleArgs a = {(uint32_t *)d_pts, c};
    return launch_group(g, n, s, bn254_g1_add_M<MsmPrepDoubleArgs>, bn254_g2_add_M<MsmPrepDoubleArgs>, a, (uint32_t)n);
}
size_t bn254_msmp_entry_bytes_M(int g) { return (size_t)(g == 1 ? 1 : 2) * AFF_ENTRY_U4 * sizeof(uint4); }
// bn254_g{1,2}_mul_base_batch.  A table: W * 2^(c-1) entries of 80 (G1) / 160 (G2) bytes for c-bit windows, 3 <= c <= 16 (c W > 254).
size_t bn254_mul_base_table_bytes_M(int g, unsigned c) {
    return (size_t)((254 + c - 1) / c) * ((size_t)1 << (c - 1)) * (g == 1 ? 1 : 2) * AFF_ENTRY_U4 * sizeof(uint4);
}
// out[i] = normalize(base * k[i]) for i < n <= 2^22 over the table of the base
int bn254_launch_mul_base_M(int g, const void *table, unsigned c, const void *k, void *out, size_t n, hipStream_t s) {
    const BaseMulArgs a = {(const uint32_t *)k, (uint32_t *)out, (const uint4 *)table, c, (254 + c - 1) / c};
    return launch_group(g, n, s, bn254_g1_add_M<BaseMulArgs>, bn254_g2_add_M<BaseMulArgs>, a, (uint32_t)n);
}
// the two ends of a table build: `n` copies of the point at d_base to d_out; the n normalised points at d_pts into the n records of `table`
int bn254_launch_mul_base_tile_M(int g, const void *d_base, void *d_out, size_t n, hipStream_t s) {
    const uint32_t words = g == 1 ? PointIo<G1F>::WORDS : PointIo<G2F>::WORDS;
    const BaseTileOp op = {(const uint32_t *)d_base, (uint32_t *)d_out, words, (uint32_t)n};
    return bn_lane_launch<256>(op, n * words, s);
}
// bn254_g{1,2}_normalize_batch: n points in runs of bn254_normalize_run_M() per lane (lane pair); `prefix`: bn254_normalize_prefix_bytes_M(g, n)
// bytes of scratch; d_out may be d_p
unsigned bn254_normalize_run_M(void) { return NORM_RUN; }
size_t bn254_normalize_prefix_bytes_M(int g, size_t n) { return n * PrefixMem<G1F>::REC * (g == 1 ? 1 : 2) * sizeof(uint4); }
int bn254_launch_normalize_M(int g, const void *d_p, void *d_out, size_t n, void *prefix, hipStream_t s) {
    const NormalizeArgs a = {(const uint32_t *)d_p, (uint32_t *)d_out, (uint4 *)prefix, (uint32_t)n};
    const size_t lanes = (n + NORM_RUN - 1) / NORM_RUN;
    return launch_group(g, lanes, s, bn254_g1_add_M<NormalizeArgs>, bn254_g2_add_M<NormalizeArgs>, a, (uint32_t)lanes);
}
// bn254_g{1,2}_eq_batch: out[i] = 1 when a[i] and b[i] are the same group element, else 0 (n int32)
int bn254_launch_eq_M(int g, const void *d_a, const void *d_b, void *d_out, size_t n, hipStream_t s) {
    const EqArgs a = {(const uint32_t *)d_a, (const uint32_t *)d_b, (int32_t *)d_out};
    return launch_group(g, n, s, bn254_g1_add_M<EqArgs>, bn254_g2_add_M<EqArgs>, a, (uint32_t)n);
}
// bn254_g{1,2}_ntt_batch.  A stage: butterflies [lo, lo + n) of stage `stage` of transforms of 2^log_n points laid back to back from d_src, written
// to d_dst (another array); wtbl: the root table pair of bn254_fr_ntt_batch; `table` (stage > 0): bn254_mul_table_bytes_M(g, n) bytes
int bn254_launch_group_ntt_stage_M(int g, const void *d_src, void *d_dst, const void *wtbl, unsigned log_n, unsigned stage, int inverse, size_t lo, size_t n, void *table, hipStream_t s) {
    const GroupNttStageArgs a = {(const uint32_t *)d_src, (uint32_t *)d_dst, (const uint32_t *)wtbl, log_n, stage, inverse ? 1u : 0u, (uint32_t)lo};
    if (stage == 0) return launch_group(g, n, s, bn254_g1_add_M<GroupNttStageArgs>, bn254_g2_add_M<GroupNttStageArgs>, a, (uint32_t)n);
    const GroupNttChainArgs c = {a, (uint4 *)table};
    return launch_group(g, n, s, bn254_g1_add_M<GroupNttChainArgs>, bn254_g2_add_M<GroupNttChainArgs>, c, (uint32_t)n);
}
// a pass: d_dst[j] = [c_j] d_src[j] (Jacobian; d_dst may be d_src) for the points j in [lo, lo + n): c_j = the shift table pair's power for
// j mod 2^log_n (scale == NULL), or the one Montgomery image at `scale`
int bn254_launch_group_ntt_scale_M(int g, const void *d_src, void *d_dst, const void *stbl, unsigned log_n, const uint64_t *scale, size_t lo, size_t n, void *table, hipStream_t s) {
    GroupNttScaleArgs a = {(const uint32_t *)d_src, (uint32_t *)d_dst, (const uint32_t *)stbl, log_n, scale ? 0u : 1u, (uint32_t)lo, {}};
    for (int i = 0; scale && i < 4; ++i) { a.scale.w[2 * i] = (uint32_t)scale[i]; a.scale.w[2 * i + 1] = (uint32_t)(scale[i] >> 32); }
    const GroupNttPassArgs c = {a, (uint4 *)table};
    return launch_group(g, n, s, bn254_g1_add_M<GroupNttPassArgs>, bn254_g2_add_M<GroupNttPassArgs>, c, (uint32_t)n);
}
int bn254_launch_mul_base_repack_M(int g, const void *d_pts, void *table, size_t n, hipStream_t s) {
    const uint32_t comps = g == 1 ? 1u : 2u;
    const BaseRepackOp op = {(const uint32_t *)d_pts, (uint4 *)table, comps, (uint32_t)n};
    return bn_lane_launch<256>(op, n * comps, s);
}
}
