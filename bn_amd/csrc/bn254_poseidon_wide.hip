// Wide Poseidon over Fr on the device (include/bn254_hip.h bn254_fr_poseidon_ex_batch, bn254_fr_poseidon_chain_batch and their _dev twins): the two
// kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, BN254_POSEIDON_WIDE_LANES lanes per permutation over the
// bodies of poseidon_wide_ops.hpp -, the tables of the widths (poseidon_wide_table.hpp: derived on the host and uploaded at the first use of a
// width), the sub-launches and the four entry points.
#include <mutex>
#include <vector>

#include "poseidon_wide_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned PSDW_BLOCK = 128;                    // lanes of a workgroup: two waves
constexpr int PSDW_G = BN254_POSEIDON_WIDE_LANES;
static_assert(PSDW_G == 4 || PSDW_G == 8 || PSDW_G == 16, "lanes per permutation: 4, 8 or 16 (a group never straddles a wave)");
constexpr unsigned PSDW_GROUPS = PSDW_BLOCK / PSDW_G;   // permutations of a workgroup

// The boundary between two phases, for ONE wave: its lanes run in lockstep and its LDS operations are served in order, so what is left is
// to wait for the operations in flight and to keep the compiler from moving an access across.  No workgroup barrier anywhere: the groups of
// a workgroup run different numbers of blocks (the chain) and leave at different times.
__device__ __forceinline__ void psdw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int G_>
struct PsdwWaveLanes {
    static constexpr int G = G_;
    int g;
    template <class F>
    __device__ __forceinline__ void phase(F f) const { f(g); psdw_wave_sync(); }
};
// The exchange buffers of the workgroup's groups: word-interleaved (PsdwExchange), 272 words per group - 8.5 / 17 / 34 KB for G = 16 / 8 / 4.
// A group whose index is past the sub-launch leaves at once: it stores nothing, and no other group reads its part of the buffer.
template <int G>
struct FrPoseidonWideExOp {
    const uint32_t *in, *init; uint32_t *out; const uint32_t *tbl; uint64_t lo; uint32_t n; int n_inputs, n_outs, rp;
    __device__ __forceinline__ void operator()() const {
        __shared__ uint32_t lds[PSDW_GROUP_WORDS * (PSDW_BLOCK / G)];
        const uint32_t q = threadIdx.x / G, grp = blockIdx.x * (PSDW_BLOCK / G) + q;
        if (grp >= n) return;
        psdw_ex_body(PsdwExchange{lds + q, PSDW_BLOCK / G}, in, n_inputs, init, n_outs, out, (size_t)(lo + grp), rp, tbl, PsdwWaveLanes<G>{(int)(threadIdx.x % G)});
    }
};
template <int G>
struct FrPoseidonWideChainOp {
    const uint32_t *in; const uint64_t *off; uint32_t *out; const uint32_t *tbl; uint64_t lo; uint32_t n; int rate, rp;
    __device__ __forceinline__ void operator()() const {
        __shared__ uint32_t lds[PSDW_GROUP_WORDS * (PSDW_BLOCK / G)];
        const uint32_t q = threadIdx.x / G, grp = blockIdx.x * (PSDW_BLOCK / G) + q;
        if (grp >= n) return;
        const uint64_t j = lo + grp, first = off[j];
        psdw_chain_body(PsdwExchange{lds + q, PSDW_BLOCK / G}, in, first, off[j + 1] - first, rate, out, (size_t)j, rp, tbl, PsdwWaveLanes<G>{(int)(threadIdx.x % G)});
    }
};

BnLaunchMax g_psdw_launch_max;      // tests only: the sub-launch size, in lanes
size_t psdw_step() { const size_t groups = g_psdw_launch_max.step() / PSDW_G; return groups ? groups : 1; }

// The table of width t in the context's device memory.  First use: derived on the host and uploaded with a BLOCKING copy under the
// context's table mutex, so every launch enqueued after this returns - on any stream, from any thread - finds it in place; never rewritten.
int psdw_table(bn254_ctx *c, int t, const uint32_t **d_tbl) {
    std::lock_guard<std::mutex> lk(c->psd_wide_mu);
    BnBuf &buf = c->psd_wide_tbl[t - psdw::T_MIN];
    if (!c->psd_wide_ready[t - psdw::T_MIN]) {
        std::vector<uint32_t> host;
        if (!psdw::derive(t, host)) return BN254_E_INTERNAL;
        const int rc = buf.reserve(host.size() * sizeof(uint32_t)); if (rc) return rc;
        HIP_TRY(hipMemcpy(buf.p, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->psd_wide_ready[t - psdw::T_MIN] = true;
    }
    *d_tbl = (const uint32_t *)buf.p;
    return BN254_OK;
}
int ex_run(bn254_ctx *c, const void *d_in, int n_inputs, const void *d_init, int n_outs, void *d_out, size_t n, hipStream_t s) {
    const int t = n_inputs + 1;
    const uint32_t *tbl;
    const int rc = psdw_table(c, t, &tbl); if (rc) return rc;
    return bn_for_parts(n, psdw_step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, "fr_poseidon_ex");
        return bn_lane_launch<PSDW_BLOCK>(FrPoseidonWideExOp<PSDW_G>{(const uint32_t *)d_in, (const uint32_t *)d_init, (uint32_t *)d_out, tbl, (uint64_t)lo, (uint32_t)cnt, n_inputs, n_outs,
                                                                     psdw::R_P[t]}, cnt * PSDW_G, s);
    });
}
// scratch guard held by the caller: the offsets go up in one copy through the context's work-list staging (bn_plan_upload: `off` may be freed
// as soon as the call returns)
int chain_run(bn254_ctx *c, const void *d_in, const size_t *off, size_t m, int rate, void *d_out, hipStream_t s) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "the offsets are uploaded as they are");
    const int t = rate + 1;
    const uint32_t *tbl;
    int rc = psdw_table(c, t, &tbl); if (rc) return rc;
    if ((rc = bn_plan_upload(c, off, (m + 1) * sizeof(size_t), nullptr, 0, s))) return rc;
    const uint64_t *d_off = (const uint64_t *)c->seg_plan.p;
    return bn_for_parts(m, psdw_step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, "fr_poseidon_chain");
        return bn_lane_launch<PSDW_BLOCK>(FrPoseidonWideChainOp<PSDW_G>{(const uint32_t *)d_in, d_off, (uint32_t *)d_out, tbl, (uint64_t)lo, (uint32_t)cnt, rate, psdw::R_P[t]}, cnt * PSDW_G, s);
    });
}
}  // namespace

extern "C" {

// order of the checks everywhere: arguments (nothing of them touches a device), then context and device; nothing waits, nothing is read back
int bn254_fr_poseidon_ex_batch_dev(bn254_ctx *ctx, const void *d_in, int n_inputs, const void *d_init, int n_outs, void *d_out, size_t n, void *stream) {
    int rc = bn_poseidon_ex_range(n_inputs, n_outs); if (rc) return rc;
    if (n == 0) return BN254_OK;
    if ((rc = bn_poseidon_ex_check(d_in, n_inputs, d_init, n_outs, d_out, n, false))) return rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return ex_run(ctx, d_in, n_inputs, d_init, n_outs, d_out, n, s); });
}
int bn254_fr_poseidon_ex_batch(bn254_ctx *ctx, const bn_fr *in, int n_inputs, const bn_fr *init, int n_outs, bn_fr *out, size_t n) {
    int rc = bn_poseidon_ex_range(n_inputs, n_outs); if (rc) return rc;
    if (n == 0) return BN254_OK;
    if ((rc = bn_poseidon_ex_check(in, n_inputs, init, n_outs, out, n, true))) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {in, n * (size_t)n_inputs * sizeof(bn_fr)}, {init, n * sizeof(bn_fr)}, out, n * (size_t)n_outs * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_poseidon_ex_batch_dev(ctx, d.in[0], n_inputs, d.in[1], n_outs, d.out, n, ctx->stream); });
}
int bn254_fr_poseidon_chain_batch_dev(bn254_ctx *ctx, const void *d_in, const size_t *offsets, size_t m, int rate, void *d_out, void *stream) {
    if (rate < 1 || rate > BN254_POSEIDON_EX_INPUTS_MAX) return BN254_E_BAD_ARG;
    if (m == 0) return BN254_OK;
    const int rc = bn_poseidon_chain_check(d_in, offsets, m, rate, d_out, false); if (rc) return rc;
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return chain_run(ctx, d_in, offsets, m, rate, d_out, s); });
}
int bn254_fr_poseidon_chain_batch(bn254_ctx *ctx, const bn_fr *in, const size_t *offsets, size_t m, int rate, bn_fr *out) {
    if (rate < 1 || rate > BN254_POSEIDON_EX_INPUTS_MAX) return BN254_E_BAD_ARG;
    if (m == 0) return BN254_OK;
    const int rc = bn_poseidon_chain_check(in, offsets, m, rate, out, true); if (rc) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    const size_t n = offsets[m];
    return bn_staged(ctx, {n ? in : nullptr, n * sizeof(bn_fr)}, {nullptr, 0}, out, m * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_poseidon_chain_batch_dev(ctx, d.in[0], offsets, m, rate, d.out, ctx->stream); });
}

// internal (not in the header; tests and tools/time_poseidon_wide.py): the lanes per permutation and the workgroup size the library was built
// with, an override of the sub-launch size in lanes (0 restores BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with
// a handful of rows, and the table of a width as the kernels read it - table_elems(t) records of eight words, C then M - without a device
int bn254_fr_poseidon_wide_lanes(void) { return PSDW_G; }
int bn254_fr_poseidon_wide_block(void) { return (int)PSDW_BLOCK; }
int bn254_fr_poseidon_wide_set_launch_max(size_t lanes) { return g_psdw_launch_max.set(lanes); }
int bn254_fr_poseidon_wide_table(int t, uint32_t *out) {
    return bn_no_throw([&]() -> int {
        std::vector<uint32_t> host;
        if (!out || !psdw::derive(t, host)) return BN254_E_BAD_ARG;
        for (size_t i = 0; i < host.size(); ++i) out[i] = host[i];
        return BN254_OK;
    });
}

}  // extern "C"
