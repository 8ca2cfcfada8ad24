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
#include "curve.hpp"
#include "io.hpp"

using namespace bn254;

namespace {
constexpr int BLOCK = 64;
typedef Fq2B<Fe> F2;

// The affine window table of a lane in global memory: [lane][entry 1..8][18 dwords padded to 80 bytes] - a lane reads the entry of
// ITS digit as five 16-byte loads from one or two cache lines (curve.hpp AffTableVars explains why not a private array).
// 16-byte groups per entry: 5 = packed (80 B: an entry may straddle two 128-byte lines; one whole line per entry measured no faster, a
// prefetch one window ahead 2 % slower: profiles/r04c_ab_g1mul.txt)
constexpr uint32_t AFF_ENTRY_U4 = 5, AFF_LANE_U4 = 8 * AFF_ENTRY_U4;                 // 80 B per entry, 640 B per lane
template <class F>
struct AffTableMem {
    uint4 *base;             // this lane's 8 entries
    __device__ __forceinline__ static void split(const Fe &a, const Fe &b, uint32_t *w) {
#pragma unroll
        for (int i = 0; i < 9; ++i) { w[i] = a.l[i]; w[9 + i] = b.l[i]; }
        w[18] = 0; w[19] = 0;
    }
    __device__ __forceinline__ void put_fe(int i, const Fe &x, const Fe &y) const {
        uint32_t w[20];
        split(x, y, w);
        uint4 *e = base + (uint32_t)(i - 1) * AFF_ENTRY_U4;
#pragma unroll
        for (int g = 0; g < 5; ++g) e[g] = make_uint4(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]);
    }
    __device__ __forceinline__ void get_fe(int i, Fe &x, Fe &y) const {
        const uint4 *e = base + (uint32_t)(i - 1) * AFF_ENTRY_U4;
        uint32_t w[20];
#pragma unroll
        for (int g = 0; g < 5; ++g) { const uint4 v = e[g]; w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w; }
#pragma unroll
        for (int i2 = 0; i2 < 9; ++i2) { x.l[i2] = w[i2]; y.l[i2] = w[9 + i2]; }
    }
    // G1: (x, y) are Fe; G2 in the lane-pair mapping: this lane's components of (x, y)
    __device__ __forceinline__ void put(int i, const Aff<FqField> &v) const { put_fe(i, v.x, v.y); }
    __device__ __forceinline__ void put(int i, const Aff<Fq2Field<Fq2B<Fe>>> &v) const { put_fe(i, v.x.v, v.y.v); }
    __device__ __forceinline__ Aff<F> get(int i) const {
        Aff<F> r;
        if constexpr (std::is_same<F, FqField>::value) get_fe(i, r.x, r.y);
        else get_fe(i, r.x.v, r.y.v);
        return r;
    }
};

// NORMALIZE is a template parameter, i.e. each flavour is its OWN kernel: with a run-time flag the reference chain and the GLV /
// windowed chain were register-allocated together (round 2: 74 spilled VGPRs in the G1 kernel).
// KEEP_JAC (the term kernels of bn254_g{1,2}_msm_batch): the fast chain WITHOUT jac_normalize - the sum of a segment is normalised once.
template <class F, bool NORMALIZE, bool KEEP_JAC = false>
__device__ __forceinline__ Jac<F> run_chain(const Jac<F> &p, const uint32_t *km, uint4 *table, uint32_t lane) {
    uint32_t kw[8], raw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kw[i] = km[i];
    fr_from_mont(kw, raw);
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
    const uint32_t *w = p + 24u * idx;
    Jac<FqField> pt = {fe_from_u32x8(w), fe_from_u32x8(w + 8), fe_from_u32x8(w + 16)};
    Jac<FqField> r = run_chain<FqField, NORMALIZE, KEEP_JAC>(pt, k + 8u * idx, table, idx);
    uint32_t *o = out + 24u * idx;
    fe_to_u32x8(r.x, o); fe_to_u32x8(r.y, o + 8); fe_to_u32x8(r.z, o + 16);
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
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pair = t >> 1;
    bool live = pair < n;
    if (!live) pair = n - 1;                       // keep both lanes of every pair active for the DPP exchanges
    const uint32_t *w = p + 48u * pair;
    typedef Fq2Field<F2> F;
    Jac<F> pt = {f2_load((const F2 *)nullptr, w), f2_load((const F2 *)nullptr, w + 16), f2_load((const F2 *)nullptr, w + 32)};
    Jac<F> r = run_chain<F, NORMALIZE, KEEP_JAC>(pt, k + 8u * pair, table, t);
    if (live) {
        uint32_t *o = out + 48u * pair;
        f2_store(r.x, o); f2_store(r.y, o + 16); f2_store(r.z, o + 32);
    }
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
// a[i] + b[i]  (or a[i] - b[i] = a[i] + (-b[i]): lib.rs:103-114,146-157, groups/mod.rs:275-347): the reference's add-2007-bl
// with its zero / equal-point branches, so the Jacobian limbs returned are the reference's own
template <class F>
__device__ __forceinline__ Jac<F> add_body(const Jac<F> &a, Jac<F> b, int negate_b) {
    const bool bz = F::is_zero(b.z);
    if (negate_b) b.y = F::select(bz, F::template lc3<-1, 0, 0>(b.y, b.y, b.y), b.y);     // neg(0) = 0 (groups/mod.rs:334-346)
    return jac_add_flags<F>(a, b, F::is_zero(a.z), bz);
}
__global__ void __launch_bounds__(BLOCK) bn254_g1_add_M(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t n, int negate_b) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    const uint32_t *wa = a + 24u * idx, *wb = b + 24u * idx;
    Jac<FqField> pa = {fe_from_u32x8(wa), fe_from_u32x8(wa + 8), fe_from_u32x8(wa + 16)};
    Jac<FqField> pb = {fe_from_u32x8(wb), fe_from_u32x8(wb + 8), fe_from_u32x8(wb + 16)};
    Jac<FqField> r = add_body<FqField>(pa, pb, negate_b);
    uint32_t *o = out + 24u * idx;
    fe_to_u32x8(r.x, o); fe_to_u32x8(r.y, o + 8); fe_to_u32x8(r.z, o + 16);
}
__global__ void __launch_bounds__(BLOCK) bn254_g2_add_M(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t n, int negate_b) {
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pair = t >> 1;
    bool live = pair < n;
    if (!live) pair = n - 1;
    typedef Fq2Field<F2> F;
    const uint32_t *wa = a + 48u * pair, *wb = b + 48u * pair;
    Jac<F> pa = {f2_load((const F2 *)nullptr, wa), f2_load((const F2 *)nullptr, wa + 16), f2_load((const F2 *)nullptr, wa + 32)};
    Jac<F> pb = {f2_load((const F2 *)nullptr, wb), f2_load((const F2 *)nullptr, wb + 16), f2_load((const F2 *)nullptr, wb + 32)};
    Jac<F> r = add_body<F>(pa, pb, negate_b);
    if (live) {
        uint32_t *o = out + 48u * pair;
        f2_store(r.x, o); f2_store(r.y, o + 16); f2_store(r.z, o + 32);
    }
}
// One level of the segmented fold of bn254_g{1,2}_msm_batch: lane (G2: lane pair) i adds the pieces[i].cnt consecutive Jacobian points at
// pieces[i].src in index order - a serial chain chosen by the host (at most BN_MSM_FOLD = 4 values) - into pieces[i].dst; an empty piece is
// the point at infinity.  The COMPLETE addition: two equal terms of a segment double, P*k + P*(r-k) cancels, and a partial sum at infinity is
// the left operand of the next addition.  pieces[i].last: the sum of a whole segment, normalised (infinity: G::zero() = (0, 1, 0)).
// Instances of the names bn254_g{1,2}_add_M beside the plain kernels; `SEG` is always true.
template <class F, class Load>
__device__ __forceinline__ Jac<F> msm_fold_body(const BnSegPiece &pc, uint32_t words, Load load) {
    Jac<F> acc = {F::zero(), F::one(), F::zero()};
    if (pc.cnt) acc = load(pc.src);
#pragma unroll 1
    for (uint32_t j = 1; j < pc.cnt; ++j) {
        const Jac<F> q = load(pc.src + words * j);
        acc = jac_add_flags<F>(acc, q, F::is_zero(acc.z), F::is_zero(q.z));
    }
    if (pc.last) acc = jac_normalize<F>(acc);
    return acc;
}
template <bool SEG>
__global__ void __launch_bounds__(BLOCK) bn254_g1_add_M(const BnSegPiece *pieces, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    const BnSegPiece pc = pieces[idx];
    Jac<FqField> r = msm_fold_body<FqField>(pc, 24u, [](const uint32_t *w) { return Jac<FqField>{fe_from_u32x8(w), fe_from_u32x8(w + 8), fe_from_u32x8(w + 16)}; });
    fe_to_u32x8(r.x, pc.dst); fe_to_u32x8(r.y, pc.dst + 8); fe_to_u32x8(r.z, pc.dst + 16);
}
template <bool SEG>
__global__ void __launch_bounds__(BLOCK) bn254_g2_add_M(const BnSegPiece *pieces, uint32_t n) {
    uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pair = t >> 1;
    bool live = pair < n;
    if (!live) pair = n - 1;                       // both lanes of a pair share the piece: the DPP exchanges never meet a retired partner
    typedef Fq2Field<F2> F;
    const BnSegPiece pc = pieces[pair];
    Jac<F> r = msm_fold_body<F>(pc, 48u, [](const uint32_t *w) { return Jac<F>{f2_load((const F2 *)nullptr, w), f2_load((const F2 *)nullptr, w + 16), f2_load((const F2 *)nullptr, w + 32)}; });
    if (live) { f2_store(r.x, pc.dst); f2_store(r.y, pc.dst + 16); f2_store(r.z, pc.dst + 32); }
}

// ---- bucket (Pippenger) method of bn254_g{1,2}_msm: one large sum (bn254_hip.hip bn_launch_msm_bucket plans the launches)
// A scalar is cut into W = ceil(254 / c) unsigned c-bit digits; term i belongs to bucket KEY = w * 2^c + digit for every window w whose digit
// is not zero.  The integer kernels count the terms per key, scan the counts and scatter (term index, key) into key order - a counting sort,
// arbitrary order inside a key.  Instances of the name bn254_fr_decode_k beside the wire decoder of bn254_hip.hip (they take the canonical
// integer of a scalar apart); the point kernels below are instances of bn254_g{1,2}_add_M.
constexpr uint32_t MSM_NONE = 0x7fffffffu;        // key of an unused entry
constexpr uint32_t MSM_SKIP = 0x80000000u;        // key flag: the entry belongs to the run of its key but carries no point
constexpr uint32_t MSM_PIECE = 16;                // entries per lane of one accumulation level: the longest serial chain, whatever the data
constexpr uint32_t MSM_TILE = 1024;               // counts per workgroup of the scan (256 threads x 4)

__device__ __forceinline__ uint32_t msm_digit(const uint32_t *raw, uint32_t w, uint32_t c) {
    const uint32_t bit = w * c, word = bit >> 5;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) { if (i == word) lo = raw[i]; if (i == word + 1) hi = raw[i]; }      // selects: `raw` stays in registers
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (bit & 31u)) & ((1u << c) - 1u);
}
// COUNT: counts[key] += 1 for every non-zero digit of k[0..n); SCATTER: the same walk, (index, key) written at cursor[key]++ (the scanned counts).
// When every active lane of a wave holds the same digit (equal scalars: the skew case) one lane adds for all of them; large groups of
// equal digits inside a wave are served the same way.
struct MsmDigitsOp {
    const uint32_t *k; uint32_t n, c, W; uint32_t *counts; uint32_t *idx, *keys; int scatter;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * 256 + threadIdx.x;
        if (i >= n) return;
        uint32_t kw[8], raw[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) kw[j] = k[8u * i + j];
        fr_from_mont(kw, raw);
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
template <class Op>
__global__ void __launch_bounds__(256) bn254_fr_decode_k(Op op) { op(); }

// One level of the bucket accumulation.  The input is a sequence of N entries in key order (level 0: the sorted terms, their points gathered
// by index; level l > 0: the partial sums level l - 1 wrote); lane (G2: lane pair) i adds the entries [i * MSM_PIECE, (i + 1) * MSM_PIECE) with
// the complete addition, run by run.  A run of one key that lies inside the lane's entries is complete: buckets[key] += sum (the buckets
// collect over the chunks of a call).  A run that began before the lane's first entry or goes on behind its last one is a piece of a longer
// run: its sum becomes an entry of the next level - slot 2i for a run that began earlier, slot 2i + 1 for one that goes on (a run over ALL of
// the lane's entries takes slot 2i and marks 2i + 1 MSM_SKIP, so that the key's run stays contiguous) - and the next level, eight times
// shorter, does the same.  So no lane's chain exceeds 2 * MSM_PIECE additions (every entry a run of its own) whatever the scalars are: 2^20 equal scalars are 2^16 lanes of
// 16 terms, then 2^13, ... - never one chain of 2^20.  N = the level-0 count on the device (*n0) taken through the levels.
struct MsmAccArgs {
    const uint32_t *pts, *idx, *keys, *n0;
    uint32_t level;
    uint32_t *out_pts, *out_keys, *buckets;
};
__device__ __forceinline__ uint32_t msm_level_len(uint32_t n, uint32_t level) {
    for (uint32_t l = 0; l < level; ++l) n = 2u * ((n + MSM_PIECE - 1) / MSM_PIECE);
    return n;
}
template <class F, uint32_t WORDS, class Load, class Store>
__device__ __forceinline__ void msm_acc_body(const MsmAccArgs &g, uint32_t i, Load load, Store store) {
    const uint32_t N = msm_level_len(*g.n0, g.level), a = i * MSM_PIECE;
    if (a >= N) return;
    const uint32_t b = min(a + MSM_PIECE, N);
    const uint32_t prev = a ? g.keys[a - 1] & ~MSM_SKIP : 0xffffffffu, next = b < N ? g.keys[b] & ~MSM_SKIP : 0xffffffffu;
    g.out_keys[2 * i] = MSM_NONE; g.out_keys[2 * i + 1] = MSM_NONE;
    Jac<F> acc = {F::zero(), F::one(), F::zero()};
    uint32_t cur = g.keys[a] & ~MSM_SKIP, j = a;
    bool first_run = true;
#pragma unroll 1
    for (;;) {
        // one step = at most one addition: an entry joins the run, or a complete run joins its bucket
        const bool at_end = j >= b;
        const uint32_t kj = at_end ? 0u : g.keys[j], key = kj & ~MSM_SKIP;
        const bool flush = at_end || key != cur;
        const uint32_t *src = nullptr;
        uint32_t *dst = nullptr;
        if (flush) {
            const bool began_earlier = first_run && prev == cur, goes_on = at_end && next == cur;
            if (cur != MSM_NONE) {
                if (!began_earlier && !goes_on) { dst = g.buckets + (size_t)cur * WORDS; src = dst; }
                else {
                    const uint32_t slot = began_earlier ? 2 * i : 2 * i + 1;
                    dst = g.out_pts + (size_t)slot * WORDS;
                    g.out_keys[slot] = cur;
                    if (began_earlier && goes_on) g.out_keys[2 * i + 1] = cur | MSM_SKIP;
                }
            }
        } else if (!(kj & MSM_SKIP) && key != MSM_NONE) {
            src = g.pts + (size_t)(g.idx ? g.idx[j] : j) * WORDS;
        }
        if (src) {
            const Jac<F> q = load(src);
            acc = jac_add_flags<F>(acc, q, F::is_zero(acc.z), F::is_zero(q.z));
        }
        if (dst) store(acc, dst);
        if (at_end) break;
        if (flush) { first_run = false; acc = {F::zero(), F::one(), F::zero()}; cur = key; }
        else ++j;
    }
}
// The bucket reduction: lane (lane pair) t = w * groups + g walks the G buckets [base, base + G) of window w from the top with a running sum,
// two additions per bucket, and leaves S = sum B_b and T = sum (b - base) B_b as two terms of the tail - the one-segment bn254_g{1,2}_msm_batch
// over 2 * W * groups terms whose scalars the host knows: base * 2^(c w) for S, 2^(c w) for T.
struct MsmReduceArgs {
    const uint32_t *buckets; uint32_t G, groups, log2B, count; uint32_t *terms;       // terms: S of every lane, then T of every lane
};
template <class F, uint32_t WORDS, class Load, class Store>
__device__ __forceinline__ void msm_reduce_body(const MsmReduceArgs &g, uint32_t t, Load load, Store store) {
    const uint32_t w = t / g.groups, base = (w << g.log2B) + (t % g.groups) * g.G;
    Jac<F> run = {F::zero(), F::one(), F::zero()}, T = run;
#pragma unroll 1
    for (uint32_t b = g.G; b-- > 0;) {
        const Jac<F> q = load(g.buckets + (size_t)(base + b) * WORDS);
        run = jac_add_flags<F>(run, q, F::is_zero(run.z), F::is_zero(q.z));
        if (b) T = jac_add_flags<F>(T, run, F::is_zero(T.z), F::is_zero(run.z));
    }
    store(run, g.terms + (size_t)t * WORDS);
    store(T, g.terms + (size_t)(g.count + t) * WORDS);
}
struct G1PointIo {
    __device__ __forceinline__ Jac<FqField> operator()(const uint32_t *w) const { return Jac<FqField>{fe_from_u32x8(w), fe_from_u32x8(w + 8), fe_from_u32x8(w + 16)}; }
    __device__ __forceinline__ void operator()(const Jac<FqField> &r, uint32_t *o) const { fe_to_u32x8(r.x, o); fe_to_u32x8(r.y, o + 8); fe_to_u32x8(r.z, o + 16); }
};
struct G2PointIo {
    typedef Fq2Field<F2> F;
    __device__ __forceinline__ Jac<F> operator()(const uint32_t *w) const { return Jac<F>{f2_load((const F2 *)nullptr, w), f2_load((const F2 *)nullptr, w + 16), f2_load((const F2 *)nullptr, w + 32)}; }
    __device__ __forceinline__ void operator()(const Jac<F> &r, uint32_t *o) const { f2_store(r.x, o); f2_store(r.y, o + 16); f2_store(r.z, o + 32); }
};
// ---- fixed-base scalar multiplication of bn254_g{1,2}_mul_base_batch: out[i] = normalize(B * k[i]) for ONE base B per call
// (bn254_seg.hip bn_launch_mul_base keeps the tables and plans the launches).  The table of a base holds the AFFINE points d * 2^(c w) * B for
// w < W = ceil(254 / c) and d = 1 .. 2^(c-1), entry (w, d) at index w * 2^(c-1) + d - 1, in the form of AffTableMem: 9 + 9 limbs padded to
// 80 bytes per lane, read as five 16-byte loads - G1 one such record per entry, G2 two (component c0 for the even lane of a pair, c1 for the
// odd one).  Word 18 of a record is not zero when the entry is the point at infinity (the base was).
// The chain: the canonical integer of the scalar is recoded, low window first, into W signed c-bit digits in [-2^(c-1), 2^(c-1)] with a
// carry (the top window of a scalar below r < 2^254 <= 2^(c W - 1) never carries), and every non-zero digit is ONE mixed addition of the
// entry |d| of its window, y negated for d < 0 - no doubling, and the accumulator starts at infinity.  The partial sum below window w is
// smaller than 2^(c w) in absolute value, so it never equals +- the entry of window w as an INTEGER; mod r that argument holds up to the
// top window only: k = r - 2 (r mod 2^(c (W-1))) recodes (when the low part carries, as it does for c = 8, 10 and 12) to a partial sum -t B and a top entry
// (r - t) B, the same point.  The additions are therefore the complete ones (jac_madd_signed / jac_madd_flags: equal points double,
// opposite points and an accumulator at infinity are followed by flags).
struct BaseMulArgs {
    const uint32_t *k; uint32_t *out; const uint4 *table; uint32_t c, W;
};
template <class F>
__device__ __forceinline__ Aff<F> base_entry(const uint4 *rec, bool &inf) {
    uint32_t w[20];
#pragma unroll
    for (int g = 0; g < 5; ++g) { const uint4 v = rec[g]; w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w; }
    Aff<F> r;
    Fe x, y;
#pragma unroll
    for (int i = 0; i < 9; ++i) { x.l[i] = w[i]; y.l[i] = w[9 + i]; }
    if constexpr (std::is_same<F, FqField>::value) { r.x = x; r.y = y; } else { r.x.v = x; r.y.v = y; }
    inf = w[18] != 0;
    return r;
}
// comp: 0 for G1; the lane's component (lane & 1) of a G2 lane pair - both lanes of a pair walk the same digits
template <class F, uint32_t WORDS, class Store>
__device__ __forceinline__ void base_mul_body(const BaseMulArgs &g, uint32_t i, uint32_t comp, Store store) {
    constexpr bool G1 = std::is_same<F, FqField>::value;
    constexpr uint32_t REC = G1 ? AFF_ENTRY_U4 : 2 * AFF_ENTRY_U4;            // 16-byte groups per table entry
    uint32_t kw[8], raw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kw[j] = g.k[8u * i + j];
    fr_from_mont(kw, raw);
    const uint32_t half = 1u << (g.c - 1);
    Jac<F> acc = {F::zero(), F::one(), F::zero()};
    bool acc_inf = true;
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < g.W; ++w) {
        const uint32_t v = msm_digit(raw, w, g.c) + carry;
        carry = v > half ? 1u : 0u;
        const uint32_t ad = carry ? (2u * half - v) : v;                      // |digit| <= 2^(c-1)
        bool e_inf;
        const Aff<F> q = base_entry<F>(g.table + (size_t)(w * half + (ad ? ad - 1u : 0u)) * REC + comp * AFF_ENTRY_U4, e_inf);
        const bool q_inf = e_inf || ad == 0;                                  // digit 0: the operand is ignored
        if constexpr (G1) {
            acc = jac_madd_signed(acc, q, carry != 0, acc_inf, q_inf);
        } else {
            Aff<F> qs = q;
            qs.y = F::select(carry != 0, q.y, F::template lc3<-1, 0, 0>(q.y, q.y, q.y));
            acc = jac_madd_flags<F>(acc, qs, acc_inf, q_inf);
            acc_inf = F::is_zero_std(acc.z);
        }
    }
    store(jac_normalize<F>(acc), g.out + (size_t)i * WORDS);
}
// The table build after the shipped normalising kernel (bn254_g{1,2}_mul_M over the tiled base and the host-known scalars d * 2^(c w)):
// tile - record j of `out` = the one point at `src`; repack - thread t turns component t % comps of the normalised point t / comps into its
// 80-byte record.  Instances of bn254_fr_decode_k like the other integer kernels of this unit.
struct BaseTileOp {
    const uint32_t *src; uint32_t *out; uint32_t words, n;
    __device__ __forceinline__ void operator()() const {
        const uint32_t t = blockIdx.x * 256 + threadIdx.x;
        if (t >= n * words) return;
        out[t] = src[t % words];
    }
};
struct BaseRepackOp {
    const uint32_t *pts; uint4 *table; uint32_t comps, n;                     // comps: 1 (G1: 24 words per point) or 2 (G2: 48)
    __device__ __forceinline__ void operator()() const {
        const uint32_t t = blockIdx.x * 256 + threadIdx.x;
        if (t >= n * comps) return;
        const uint32_t e = t / comps, comp = t % comps;
        const uint32_t *p = pts + (size_t)e * 24u * comps;
        const Fe x = fe_from_u32x8(p + 8u * comp), y = fe_from_u32x8(p + 8u * comps + 8u * comp);
        uint32_t z = 0;
        for (uint32_t j = 0; j < 8u * comps; ++j) z |= p[16u * comps + j];   // normalised: z is one, or zero at infinity (canonical words)
        uint32_t w[20];
        AffTableMem<FqField>::split(x, y, w);
        w[18] = z == 0 ? 1u : 0u;
        uint4 *rec = table + (size_t)t * AFF_ENTRY_U4;
#pragma unroll
        for (int g = 0; g < 5; ++g) rec[g] = make_uint4(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]);
    }
};
// `n`: lanes (G2: lane pairs) launched; a lane past the level's entries, or past the reduction's groups, has nothing to do (both lanes of a pair alike)
__device__ __forceinline__ void msm_point_op(const BaseMulArgs &g, uint32_t i, G1PointIo io) { base_mul_body<FqField, 24u>(g, i, 0u, io); }
__device__ __forceinline__ void msm_point_op(const BaseMulArgs &g, uint32_t i, G2PointIo io) { base_mul_body<Fq2Field<F2>, 48u>(g, i, threadIdx.x & 1u, io); }
__device__ __forceinline__ void msm_point_op(const MsmAccArgs &g, uint32_t i, G1PointIo io) { msm_acc_body<FqField, 24u>(g, i, io, io); }
__device__ __forceinline__ void msm_point_op(const MsmAccArgs &g, uint32_t i, G2PointIo io) { msm_acc_body<Fq2Field<F2>, 48u>(g, i, io, io); }
__device__ __forceinline__ void msm_point_op(const MsmReduceArgs &g, uint32_t i, G1PointIo io) { msm_reduce_body<FqField, 24u>(g, i, io, io); }
__device__ __forceinline__ void msm_point_op(const MsmReduceArgs &g, uint32_t i, G2PointIo io) { msm_reduce_body<Fq2Field<F2>, 48u>(g, i, io, io); }
template <class Args>
__global__ void __launch_bounds__(BLOCK) bn254_g1_add_M(Args g, uint32_t n) {
    const uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx < n) msm_point_op(g, idx, G1PointIo());
}
template <class Args>
__global__ void __launch_bounds__(BLOCK) bn254_g2_add_M(Args g, uint32_t n) {
    const uint32_t pair = (blockIdx.x * BLOCK + threadIdx.x) >> 1;
    if (pair < n) msm_point_op(g, pair, G2PointIo());
}
}  // namespace

extern "C" {
int bn254_launch_g1_add_M(const void *a, const void *b, void *out, size_t n, int negate_b, hipStream_t s) {
    unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(bn254_g1_add_M, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, (uint32_t)n, negate_b);
    return (int)hipGetLastError();
}
int bn254_launch_g2_add_M(const void *a, const void *b, void *out, size_t n, int negate_b, hipStream_t s) {
    unsigned grid = (unsigned)((2 * n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(bn254_g2_add_M, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)a, (const uint32_t *)b, (uint32_t *)out, (uint32_t)n, negate_b);
    return (int)hipGetLastError();
}
// `table` (normalize != 0 only): bn254_mul_table_bytes_M(g, n) bytes of scratch for the window tables of this launch
size_t bn254_mul_table_bytes_M(int g, size_t n) {
    const size_t lanes = g == 1 ? (n + BLOCK - 1) / BLOCK * BLOCK : (2 * n + BLOCK - 1) / BLOCK * BLOCK;
    return lanes * AFF_LANE_U4 * sizeof(uint4);
}
int bn254_launch_g1_mul_M(const void *p, const void *k, void *out, size_t n, int normalize, void *table, hipStream_t s) {
    unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    if (normalize) hipLaunchKernelGGL(bn254_g1_mul_M, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n, (uint4 *)table);
    else hipLaunchKernelGGL(bn254_g1_mul_chain_M, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n);
    return (int)hipGetLastError();
}
int bn254_launch_g2_mul_M(const void *p, const void *k, void *out, size_t n, int normalize, void *table, hipStream_t s) {
    unsigned grid = (unsigned)((2 * n + BLOCK - 1) / BLOCK);
    if (normalize) hipLaunchKernelGGL(bn254_g2_mul_M, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n, (uint4 *)table);
    else hipLaunchKernelGGL(bn254_g2_mul_chain_M, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n);
    return (int)hipGetLastError();
}
// bn254_g{1,2}_msm_batch: the term kernel (Jacobian results, `table` as above) and one level of the segmented fold (`count` pieces in device memory)
int bn254_launch_msm_mul_M(int g, const void *p, const void *k, void *out, size_t n, void *table, hipStream_t s) {
    unsigned grid = (unsigned)(((g == 1 ? n : 2 * n) + BLOCK - 1) / BLOCK);
    if (g == 1) hipLaunchKernelGGL(bn254_g1_mul_M<true>, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n, (uint4 *)table);
    else hipLaunchKernelGGL(bn254_g2_mul_M<true>, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t *)p, (const uint32_t *)k, (uint32_t *)out, (uint32_t)n, (uint4 *)table);
    return (int)hipGetLastError();
}
int bn254_launch_msm_fold_M(int g, const void *pieces, size_t count, hipStream_t s) {
    unsigned grid = (unsigned)(((g == 1 ? count : 2 * count) + BLOCK - 1) / BLOCK);
    if (g == 1) hipLaunchKernelGGL(bn254_g1_add_M<true>, dim3(grid), dim3(BLOCK), 0, s, (const BnSegPiece *)pieces, (uint32_t)count);
    else hipLaunchKernelGGL(bn254_g2_add_M<true>, dim3(grid), dim3(BLOCK), 0, s, (const BnSegPiece *)pieces, (uint32_t)count);
    return (int)hipGetLastError();
}
// bn254_g{1,2}_msm, bucket route.  n terms (< 2^32 / W entries in all), window width c, W windows.
// digits: scatter == 0 counts the terms per key into `counts` (zeroed by the caller); scatter != 0 writes (index, key) at the scanned counts
int bn254_launch_msm_digits_M(const void *k, size_t n, unsigned c, unsigned W, void *counts, void *idx, void *keys, int scatter, hipStream_t s) {
    const MsmDigitsOp op = {(const uint32_t *)k, (uint32_t)n, c, W, (uint32_t *)counts, (uint32_t *)idx, (uint32_t *)keys, scatter};
    hipLaunchKernelGGL(bn254_fr_decode_k<MsmDigitsOp>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, op);
    return (int)hipGetLastError();
}
// counts[0..total) -> their exclusive scan in place, the grand total to *n0; total <= 2^20, `tiles`: 1024 words of scratch
int bn254_launch_msm_scan_M(void *counts, size_t total, void *tiles, void *n0, hipStream_t s) {
    const unsigned blocks = (unsigned)((total + MSM_TILE - 1) / MSM_TILE);
    if (blocks == 0 || blocks > MSM_TILE) return (int)hipErrorInvalidValue;
    for (int mode = 0; mode < 3; ++mode) {
        const MsmScanOp op = {(uint32_t *)counts, (uint32_t)total, (uint32_t *)tiles, (uint32_t *)n0, mode};
        hipLaunchKernelGGL(bn254_fr_decode_k<MsmScanOp>, dim3(mode == 1 ? 1u : blocks), dim3(256), 0, s, op);
    }
    return (int)hipGetLastError();
}
unsigned bn254_msm_piece_M(void) { return MSM_PIECE; }
// one accumulation level over `lanes` lanes (G2: lane pairs); idx != NULL only at level 0
int bn254_launch_msm_bucket_M(int g, const void *pts, const void *idx, const void *keys, const void *n0, unsigned level, void *out_pts, void *out_keys, void *buckets,
                              size_t lanes, hipStream_t s) {
    const MsmAccArgs a = {(const uint32_t *)pts, (const uint32_t *)idx, (const uint32_t *)keys, (const uint32_t *)n0, level, (uint32_t *)out_pts, (uint32_t *)out_keys, (uint32_t *)buckets};
    const unsigned grid = (unsigned)(((g == 1 ? lanes : 2 * lanes) + BLOCK - 1) / BLOCK);
    if (g == 1) hipLaunchKernelGGL(bn254_g1_add_M<MsmAccArgs>, dim3(grid), dim3(BLOCK), 0, s, a, (uint32_t)lanes);
    else hipLaunchKernelGGL(bn254_g2_add_M<MsmAccArgs>, dim3(grid), dim3(BLOCK), 0, s, a, (uint32_t)lanes);
    return (int)hipGetLastError();
}
// the bucket reduction: count = W * groups lanes (lane pairs), terms = 2 * count points
int bn254_launch_msm_reduce_M(int g, const void *buckets, unsigned G, unsigned groups, unsigned c, size_t count, void *terms, hipStream_t s) {
    const MsmReduceArgs a = {(const uint32_t *)buckets, G, groups, c, (uint32_t)count, (uint32_t *)terms};
    const unsigned grid = (unsigned)(((g == 1 ? count : 2 * count) + BLOCK - 1) / BLOCK);
    if (g == 1) hipLaunchKernelGGL(bn254_g1_add_M<MsmReduceArgs>, dim3(grid), dim3(BLOCK), 0, s, a, (uint32_t)count);
    else hipLaunchKernelGGL(bn254_g2_add_M<MsmReduceArgs>, dim3(grid), dim3(BLOCK), 0, s, a, (uint32_t)count);
    return (int)hipGetLastError();
}
// bn254_g{1,2}_mul_base_batch.  A table: W * 2^(c-1) entries of 80 (G1) / 160 (G2) bytes for c-bit windows, 3 <= c <= 16 (c W > 254).
size_t bn254_mul_base_table_bytes_M(int g, unsigned c) {
    return (size_t)((254 + c - 1) / c) * ((size_t)1 << (c - 1)) * (g == 1 ? 1 : 2) * AFF_ENTRY_U4 * sizeof(uint4);
}
// out[i] = normalize(base * k[i]) for i < n <= 2^22 over the table of the base
int bn254_launch_mul_base_M(int g, const void *table, unsigned c, const void *k, void *out, size_t n, hipStream_t s) {
    const BaseMulArgs a = {(const uint32_t *)k, (uint32_t *)out, (const uint4 *)table, c, (254 + c - 1) / c};
    const unsigned grid = (unsigned)(((g == 1 ? n : 2 * n) + BLOCK - 1) / BLOCK);
    if (g == 1) hipLaunchKernelGGL(bn254_g1_add_M<BaseMulArgs>, dim3(grid), dim3(BLOCK), 0, s, a, (uint32_t)n);
    else hipLaunchKernelGGL(bn254_g2_add_M<BaseMulArgs>, dim3(grid), dim3(BLOCK), 0, s, a, (uint32_t)n);
    return (int)hipGetLastError();
}
// the two ends of a table build: `n` copies of the point at d_base to d_out; the n normalised points at d_pts into the n records of `table`
int bn254_launch_mul_base_tile_M(int g, const void *d_base, void *d_out, size_t n, hipStream_t s) {
    const uint32_t words = g == 1 ? 24u : 48u;
    const BaseTileOp op = {(const uint32_t *)d_base, (uint32_t *)d_out, words, (uint32_t)n};
    hipLaunchKernelGGL(bn254_fr_decode_k<BaseTileOp>, dim3((unsigned)((n * words + 255) / 256)), dim3(256), 0, s, op);
    return (int)hipGetLastError();
}
int bn254_launch_mul_base_repack_M(int g, const void *d_pts, void *table, size_t n, hipStream_t s) {
    const uint32_t comps = g == 1 ? 1u : 2u;
    const BaseRepackOp op = {(const uint32_t *)d_pts, (uint4 *)table, comps, (uint32_t)n};
    hipLaunchKernelGGL(bn254_fr_decode_k<BaseRepackOp>, dim3((unsigned)((n * comps + 255) / 256)), dim3(256), 0, s, op);
    return (int)hipGetLastError();
}
}
