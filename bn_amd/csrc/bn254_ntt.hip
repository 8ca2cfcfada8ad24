// Number-theoretic transforms over Fr on the device (include/bn254_hip.h bn254_fr_ntt_batch, its _dev twin and bn254_fr_root_of_unity): the
// two kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, launched by workgroup, over the bodies of
// ntt_ops.hpp -, the context-owned twiddle tables, the cut of a call into groups of transforms, passes and sub-launches, and the entry points.
#include <algorithm>

#include "host_ctx.hpp"
#include "lane_launch.hpp"
#include "ntt_ops.hpp"

using namespace bn254;

namespace {
// one workgroup per tile of 2^T elements: load, t stages, store
struct NttPassOp {
    NttPass P;
    __device__ __forceinline__ void operator()() const {
        extern __shared__ uint4 ntt_lds[];                                          // ntt_lds_bytes(): the tile, then the stage twiddles
        uint32_t *const tl = (uint32_t *)ntt_lds, *const tw = tl + (8u << P.T);
        ntt_twiddle_lane(P, tw, threadIdx.x);
        ntt_load_lane(P, tl, blockIdx.x, threadIdx.x);
        __syncthreads();
#pragma unroll 1
        for (uint32_t st = 0; st < P.t; ++st) {
            ntt_stage_lane(P, tl, tw, blockIdx.x, threadIdx.x, st);
            __syncthreads();
        }
        ntt_store_lane(P, tl, blockIdx.x, threadIdx.x);
    }
};
struct NttTableOp {
    uint32_t *out; Fr c0, g0, c1, g1;
    __device__ __forceinline__ void operator()() const { ntt_table_body(out, c0, g0, c1, g1, blockIdx.x * NTT_BLOCK + threadIdx.x); }
};

// LDS of a pass, sized at the launch for the tile log in force, so that a smaller tile also gets the occupancy of a smaller tile: 2^T
// elements and the 2^(t-1) stage twiddles, 48 KiB at T = t = 10
size_t ntt_lds_bytes(unsigned T, unsigned t) { return ((size_t)sizeof(bn_fr) << T) + (t ? (size_t)sizeof(bn_fr) << (t - 1) : 0); }

// tests and tools/time_ntt.py only: the tile log in force and the sub-launch size
BnOverride<unsigned> g_ntt_tile_log;
BnLaunchMax g_ntt_launch_max;

Fr fr_of(const uint64_t *l) {
    Fr r;
    for (int i = 0; i < 4; ++i) { r.w[2 * i] = (uint32_t)l[i]; r.w[2 * i + 1] = (uint32_t)(l[i] >> 32); }
    return r;
}
constexpr size_t NTT_PAIR_BYTES = 2 * (size_t)NTT_TBL * sizeof(bn_fr);      // one table pair: 256 KiB
int ntt_build_pair(bn254_ctx *c, uint32_t *out, const uint64_t *c0, const uint64_t *g0, hipStream_t s) {
    const uint64_t e[4] = {NTT_TBL, 0, 0, 0};
    bn_fr one, g1;
    bn_fr_one(&one);
    bn_fr_pow(g0, e, g1.l);
    BnScope sc(c, s, "ntt_table");
    return bn_block_launch<NTT_BLOCK>(NttTableOp{out, fr_of(c0), fr_of(g0), fr_of(one.l), fr_of(g1.l)}, 2 * NTT_TBL / NTT_BLOCK, 0, s);
}
// scratch guard held by the caller.  The root pair is built once per context; the shift pair is rebuilt when its key changes: the shift
// alone for a forward transform (the pair holds s^i, whatever the size), shift and size for an inverse one (n^-1 s^-i).
int ntt_tables(bn254_ctx *c, int log_n, int inverse, const bn_fr *shift, hipStream_t s) {
    int rc = c->ntt_tbl.reserve(2 * NTT_PAIR_BYTES); if (rc) return rc;
    if (!c->ntt_root_ready) {
        bn_fr one, w;
        bn_fr_one(&one);
        bn_fr_root((int)NTT_LOG_MAX, &w);
        if ((rc = ntt_build_pair(c, (uint32_t *)c->ntt_tbl.p, one.l, w.l, s))) return rc;
        c->ntt_root_ready = true;
    }
    if (!shift) return BN254_OK;
    const uint64_t key[5] = {shift->l[0], shift->l[1], shift->l[2], shift->l[3], inverse ? (uint64_t)log_n << 1 | 1u : 0u};
    if (c->ntt_shift_valid && !memcmp(key, c->ntt_shift_key, sizeof key)) return BN254_OK;
    bn_fr c0, g0 = *shift;
    bn_fr_inv_pow2(inverse ? (unsigned)log_n : 0u, &c0);
    if (inverse) bn_fr_inverse(shift->l, g0.l);
    c->ntt_shift_valid = false;
    if ((rc = ntt_build_pair(c, (uint32_t *)c->ntt_tbl.p + 8 * 2 * NTT_TBL, c0.l, g0.l, s))) return rc;
    memcpy(c->ntt_shift_key, key, sizeof key);
    c->ntt_shift_valid = true;
    return BN254_OK;
}

// scratch guard held by the caller.  Groups, passes, buffers and sub-launches are host_plan.hpp's (bn_ntt_run, bn_ntt_group); here the
// buffers get their addresses and every step becomes one launch.
int ntt_run(bn254_ctx *c, const void *d_in, void *d_out, int log_n, size_t count, int inverse, const bn_fr *shift, hipStream_t s) {
    const unsigned T = g_ntt_tile_log.get(NTT_TILE_LOG);
    const size_t N = (size_t)1 << log_n, step = g_ntt_launch_max.step();
    const bool in_place = d_in == (const void *)d_out;
    const BnNttRun run = bn_ntt_run((unsigned)log_n, T, count, step, in_place);
    int rc = ntt_tables(c, log_n, inverse, shift, s); if (rc) return rc;
    if (run.ws_bufs && (rc = c->ntt_ws.reserve(run.ws_bufs * run.most * sizeof(bn_fr)))) return rc;
    NttPass K = {};
    K.wtbl = (const uint32_t *)c->ntt_tbl.p; K.stbl = K.wtbl + 8 * 2 * NTT_TBL;
    K.log_n = (uint32_t)log_n; K.T = T; K.inverse = inverse != 0;
    if (inverse && !shift) {
        bn_fr sc;
        bn_fr_inv_pow2((unsigned)log_n, &sc);
        K.scale = fr_of(sc.l);
    }
    return bn_for_parts(count, run.per_group, [&](size_t tr0, size_t cnt) -> int {
        uint32_t *const buf[4] = {(uint32_t *)d_in + 8 * tr0 * N, (uint32_t *)d_out + 8 * tr0 * N, (uint32_t *)c->ntt_ws.p, (uint32_t *)c->ntt_ws.p + 8 * run.most};
        return bn_ntt_group(run, (unsigned)log_n, T, cnt, step, in_place, shift != nullptr, inverse != 0, [&](const BnNttStep &st) -> int {
            K.in = buf[st.src]; K.out = buf[st.dst];
            K.t = st.g.t; K.log_m = st.g.log_m; K.log_s = st.g.log_s;
            K.pre = st.pre; K.post = st.post;
            K.tile_lo = (uint32_t)st.lo; K.tile_end = (uint32_t)(st.lo + st.n);
            BnScope sc(c, s, "ntt");
            return bn_block_launch<NTT_BLOCK>(NttPassOp{K}, st.blocks, ntt_lds_bytes(T, K.t), s);
        });
    });
}

// order of the checks: empty call, arguments (nothing of them touches a device), then context and device
int ntt_check(const void *in, const void *out, int log_n, size_t count, const bn_fr *shift) {
    if (log_n < 0 || log_n > BN254_NTT_LOG_MAX || !in || !out) return BN254_E_BAD_ARG;
    if (count > (BN_N_MAX >> log_n)) return BN254_E_BAD_ARG;
    if (shift && bn_fr_is_zero(shift->l)) return BN254_E_BAD_ARG;
    return BN254_OK;
}
}  // namespace

// the tables for bn254_group_ntt.hip (host_ctx.hpp): the same pairs under the same keys, so the two families share them
int bn_ntt_tables(bn254_ctx *c, int log_n, int inverse, const bn_fr *shift, hipStream_t s) { return ntt_tables(c, log_n, inverse, shift, s); }

extern "C" {

int bn254_fr_root_of_unity(int log_n, bn_fr *out) { return bn_fr_root(log_n, out); }

int bn254_fr_ntt_batch_dev(bn254_ctx *ctx, const void *d_in, void *d_out, int log_n, size_t count, int inverse, const bn_fr *shift, void *stream) {
    if (count == 0) return BN254_OK;
    int rc = ntt_check(d_in, d_out, log_n, count, shift); if (rc) return rc;      // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return ntt_run(ctx, d_in, d_out, log_n, count, inverse, shift, s); });
}
int bn254_fr_ntt_batch(bn254_ctx *ctx, const bn_fr *in, bn_fr *out, int log_n, size_t count, int inverse, const bn_fr *shift) {
    if (count == 0) return BN254_OK;
    int rc = ntt_check(in, out, log_n, count, shift); if (rc) return rc;          // before any device lookup
    BnHost h(ctx); if (h.rc) return h.rc;
    const size_t bytes = (count << log_n) * sizeof(bn_fr);
    return bn_staged(ctx, {in, bytes}, {nullptr, 0}, out, bytes, nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_ntt_batch_dev(ctx, d.in[0], d.out, log_n, count, inverse, shift, ctx->stream); });
}

// internal (not in the header; tests and tools/time_ntt.py): the shipped tile log, a process-wide override of it (0 restores the shipped
// one, otherwise 1 .. shipped; same bytes whatever is set), and an override of the sub-launch
// size (0 restores BN_LAUNCH_MAX) so that a test reaches the seams between groups and sub-launches with a handful of elements
unsigned bn254_ntt_tile_log(void) { return NTT_TILE_LOG; }
int bn254_ntt_set_tile_log(unsigned T) { return T > NTT_TILE_LOG ? BN254_E_BAD_ARG : g_ntt_tile_log.set(T); }
int bn254_ntt_set_launch_max(size_t elements) { return g_ntt_launch_max.set(elements); }

}  // extern "C"
