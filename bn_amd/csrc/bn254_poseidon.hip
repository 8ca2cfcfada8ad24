// Poseidon hashes and Merkle trees over Fr on the device (include/bn254_hip.h bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch,
// bn254_fr_merkle_tree and their _dev twins): the kernels - Ops of lane_launch.hpp's bn254_fr_decode_k like the other integer kernels, one lane of the
// body of poseidon_ops.hpp each, one instance per width, hash or permutation by a flag -, the levels host_plan.hpp's bn_merkle_plan computes as sub-launches, and the six
// entry points.
#include "poseidon_ops.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"

using namespace bn254;

namespace {
constexpr unsigned PSD_BLOCK = 256;

// lanes [lo, lo + n) of a call: a sub-launch.  hash: the digest of arity T - 1, or the whole permutation of width T
template <int T>
struct FrPoseidonOp {
    const uint32_t *in; uint32_t *out; uint64_t lo; uint32_t n; uint32_t hash;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * PSD_BLOCK + threadIdx.x;
        if (i < n) fr_poseidon_body<T>(in, out, lo + i, hash != 0);
    }
};

BnLaunchMax g_psd_launch_max;       // tests only: the sub-launch size

int psd_launch_t(int t, bool hash, const uint32_t *in, uint32_t *out, size_t lo, size_t cnt, hipStream_t s) {
    switch (t) {
    case 2: return bn_lane_launch<PSD_BLOCK>(FrPoseidonOp<2>{in, out, (uint64_t)lo, (uint32_t)cnt, hash}, cnt, s);
    case 3: return bn_lane_launch<PSD_BLOCK>(FrPoseidonOp<3>{in, out, (uint64_t)lo, (uint32_t)cnt, hash}, cnt, s);
    case 4: return bn_lane_launch<PSD_BLOCK>(FrPoseidonOp<4>{in, out, (uint64_t)lo, (uint32_t)cnt, hash}, cnt, s);
    default: return bn_lane_launch<PSD_BLOCK>(FrPoseidonOp<5>{in, out, (uint64_t)lo, (uint32_t)cnt, hash}, cnt, s);
    }
}
int hash_run(bn254_ctx *c, const void *d_in, int t, void *d_out, size_t n, hipStream_t s, const char *scope) {
    return bn_for_parts(n, g_psd_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, scope);
        return psd_launch_t(t, true, (const uint32_t *)d_in, (uint32_t *)d_out, lo, cnt, s);
    });
}
int permute_run(bn254_ctx *c, const void *d_in, int t, void *d_out, size_t n, hipStream_t s) {
    return bn_for_parts(n, g_psd_launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, "fr_poseidon_permute");
        return psd_launch_t(t, false, (const uint32_t *)d_in, (uint32_t *)d_out, lo, cnt, s);
    });
}
// one launch (or its sub-launches) per level, in the plan's order; the stream orders them
int merkle_run(bn254_ctx *c, const void *d_leaves, int log_n, void *d_nodes, hipStream_t s) {
    uint32_t *const nodes = (uint32_t *)d_nodes;
    for (const BnMerkleLevel &lv : bn_merkle_plan(log_n, g_psd_launch_max.step())) {
        const int rc = hash_run(c, lv.from_leaves ? d_leaves : (const void *)(nodes + 8 * lv.src), 3, nodes + 8 * lv.dst, lv.cnt, s, "fr_merkle_level");
        if (rc) return rc;
    }
    return BN254_OK;
}
}  // namespace

extern "C" {

// order of the checks everywhere: arguments (nothing of them touches a device), then context and device; nothing waits, nothing is read back
int bn254_fr_poseidon_batch_dev(bn254_ctx *ctx, const void *d_in, int arity, void *d_out, size_t n, void *stream) {
    if (arity < 1 || arity > BN254_POSEIDON_ARITY_MAX) return BN254_E_BAD_ARG;
    if (n == 0) return BN254_OK;
    int rc = bn_poseidon_check(d_in, arity + 1, d_out, n); if (rc) return rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return hash_run(ctx, d_in, arity + 1, d_out, n, s, "fr_poseidon"); });
}
int bn254_fr_poseidon_batch(bn254_ctx *ctx, const bn_fr *in, int arity, bn_fr *out, size_t n) {
    if (arity < 1 || arity > BN254_POSEIDON_ARITY_MAX) return BN254_E_BAD_ARG;
    if (n == 0) return BN254_OK;
    int rc = bn_poseidon_check(in, arity + 1, out, n); if (rc) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {in, n * (size_t)arity * sizeof(bn_fr)}, {nullptr, 0}, out, n * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_poseidon_batch_dev(ctx, d.in[0], arity, d.out, n, ctx->stream); });
}
int bn254_fr_poseidon_permute_batch_dev(bn254_ctx *ctx, const void *d_in, int t, void *d_out, size_t n, void *stream) {
    if (t < 2 || t > BN254_POSEIDON_ARITY_MAX + 1) return BN254_E_BAD_ARG;
    if (n == 0) return BN254_OK;
    int rc = bn_poseidon_check(d_in, t, d_out, n); if (rc) return rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return permute_run(ctx, d_in, t, d_out, n, s); });
}
int bn254_fr_poseidon_permute_batch(bn254_ctx *ctx, const bn_fr *in, int t, bn_fr *out, size_t n) {
    if (t < 2 || t > BN254_POSEIDON_ARITY_MAX + 1) return BN254_E_BAD_ARG;
    if (n == 0) return BN254_OK;
    int rc = bn_poseidon_check(in, t, out, n); if (rc) return rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {in, n * (size_t)t * sizeof(bn_fr)}, {nullptr, 0}, out, n * (size_t)t * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_poseidon_permute_batch_dev(ctx, d.in[0], t, d.out, n, ctx->stream); });
}
int bn254_fr_merkle_tree_dev(bn254_ctx *ctx, const void *d_leaves, int log_n, void *d_nodes, void *stream) {
    int rc = bn_merkle_check(d_leaves, log_n, d_nodes); if (rc) return rc;
    if (log_n == 0) return BN254_OK;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return merkle_run(ctx, d_leaves, log_n, d_nodes, s); });
}
int bn254_fr_merkle_tree(bn254_ctx *ctx, const bn_fr *leaves, int log_n, bn_fr *nodes) {
    int rc = bn_merkle_check(leaves, log_n, nodes); if (rc) return rc;
    if (log_n == 0) return BN254_OK;
    BnHost h(ctx); if (h.rc) return h.rc;
    const size_t n = (size_t)1 << log_n;
    return bn_staged(ctx, {leaves, n * sizeof(bn_fr)}, {nullptr, 0}, nodes, (n - 1) * sizeof(bn_fr), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_fr_merkle_tree_dev(ctx, d.in[0], log_n, d.out, ctx->stream); });
}

// internal (not in the header; tests and tools/time_poseidon.py): an override of the sub-launch size of all three calls (0 restores BN_LAUNCH_MAX) so
// that a test reaches the seam between two sub-launches with a handful of lanes, and whether the matrix rows are the fused product-sum
int bn254_fr_poseidon_set_launch_max(size_t lanes) { return g_psd_launch_max.set(lanes); }
int bn254_fr_poseidon_fused_row(void) {
#if BN254_POSEIDON_FUSED_ROW
    return 1;
#else
    return 0;
#endif
}

}  // extern "C"
