// Measurement and synthetic-input kernels of the BN254 engine (include/bn254_hip.h "measurement" / "synthetic benchmark inputs"): nothing on
// the pairing path calls into this unit, except that the record-copy kernel has a gather instance (bn254_launch_gather_K) which the small
// route of bn254_pairing_product_batch_prepared_native uses to line up the G2 points its pairs name.
//   * bn254_ubench_mac32(_ex): the v_mad_u64_u32 issue-rate microbenchmark behind bench.py's same-run `roofline.peak` (tools/ubench.hip is the
//     long form; the multiplier's rate depends on its DATA - profiles/r04_ubench_mad_data_dependence.txt -, hence the operand-width argument:
//     32 random bits for `peak`, the engine's own 29-bit limbs for `peak_at_kernel_occupancy`);
//   * bn254_synthetic_scalars_dev: the on-device generator of the synthetic Fr scalars (SplitMix64 -> 512 bits -> mod r -> Montgomery form),
//     word for word bn_amd.distributed.synthetic_scalars; the kernel is a launch of fr_ops.hpp's fr_synthetic_body, which the host
//     simulation runs too - this unit has no Fr arithmetic of its own;
//   * bn254_tile_dev: one record repeated n times (the generator bases the scalars multiply).
#include <cstdint>
#include <mutex>

#include "fr_ops.hpp"
#include "host_ctx.hpp"

namespace {

// 16 independent-ish v_mad_u64_u32 per iteration on 8 accumulators: the issue-rate ceiling of the instruction every field
// multiplication of the engine is built from (tools/ubench.hip is the long form of this experiment)
__global__ void __launch_bounds__(256) bn254_ubench_mad_k(uint32_t *out, uint32_t seed, int iters, uint32_t operand_mask) {
    uint32_t a = (threadIdx.x * 2654435761u + seed) & operand_mask, b = (a ^ 0x9e3779b9u) & operand_mask;
    uint64_t acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = a + i;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 16; ++u) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[u & 7]) : "v"(a), "v"(b) : "vcc");
    }
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i];
    if (s == 0x1234567) out[threadIdx.x] = (uint32_t)s;
}

// out[j] = Montgomery image of (512-bit SplitMix64 draw of stream 2*(lo+j)+which) mod r   (bn_amd.distributed.synthetic_scalars)
__global__ void __launch_bounds__(64) bn254_synthetic_scalars_k(uint64_t lo, uint32_t n, uint32_t which, uint64_t seed, uint32_t *out) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j < n) bn254::fr_synthetic_body(seed, lo, j, which, out);
}
// out[i] = src[0]  (tiles one point/record of `words` u32 over n records: the generator bases of the synthetic inputs)
// GATHER: out[i] = src[index[i]] - record i of the output is record index[i] of the `records` source records, or all zero (for a point: z = 0,
// the point at infinity) when the index is out of range.  The small route of bn254_pairing_product_batch_prepared_native: the G2 points a
// handle keeps, gathered by the pairs' indices for the general kernels.
template <bool GATHER>
__global__ void __launch_bounds__(256) bn254_tile_k(const uint32_t *src, uint32_t words, uint64_t total, uint32_t *out, const uint64_t *index, uint64_t records) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if constexpr (GATHER) {
        const uint64_t r = index[i / words];
        out[i] = r < records ? src[r * words + i % words] : 0u;
    } else {
        out[i] = src[i % words];
    }
}

}  // namespace

extern "C" {

// G MAC32/s (lane multiply-accumulates per second) of a pure v_mad_u64_u32 stream at `waves_per_simd` resident waves on operands of
// `operand_bits` random bits (32: any words; 29: the engine's limbs - the instruction is ~3 % faster on them)
int bn254_ubench_mac32_ex(bn254_ctx *ctx, int waves_per_simd, int iters, int operand_bits, double *gmac_per_s, double *ms_out) {
    int rc = bn_get_ctx(ctx); if (rc) return rc;
    if (waves_per_simd < 1 || waves_per_simd > 8 || iters < 1 || operand_bits < 1 || operand_bits > 32 || !gmac_per_s) return BN254_E_BAD_ARG;
    const uint32_t mask = operand_bits == 32 ? 0xffffffffu : ((1u << operand_bits) - 1u);
    std::lock_guard<std::mutex> lk(ctx->mu);
    BnDeviceGuard dev_guard;
    HIP_TRY(hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    const int blocks = prop.multiProcessorCount * waves_per_simd;          // 256 threads = one wave on each of a CU's 4 SIMDs
    if ((rc = ctx->stage[0].reserve(4096))) return rc;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    hipLaunchKernelGGL(bn254_ubench_mad_k, dim3(blocks), dim3(256), 0, ctx->stream, (uint32_t *)ctx->stage[0].p, 1u, iters / 8 + 1, mask);   // warm-up
    HIP_TRY(hipEventRecord(e0, ctx->stream));
    hipLaunchKernelGGL(bn254_ubench_mad_k, dim3(blocks), dim3(256), 0, ctx->stream, (uint32_t *)ctx->stage[0].p, 2u, iters, mask);
    HIP_TRY(hipEventRecord(e1, ctx->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    *gmac_per_s = (double)blocks * 256.0 * 16.0 * iters / (ms * 1e-3) / 1e9;
    if (ms_out) *ms_out = ms;
    return BN254_OK;
}
int bn254_ubench_mac32(bn254_ctx *ctx, int waves_per_simd, int iters, double *gmac_per_s, double *ms_out) {
    return bn254_ubench_mac32_ex(ctx, waves_per_simd, iters, 32, gmac_per_s, ms_out);
}

int bn254_synthetic_scalars_dev(bn254_ctx *ctx, uint64_t seed, uint64_t lo, size_t n, int which, void *d_out, void *stream) {
    int rc = bn_get_ctx(ctx); if (rc) return rc;
    if (n == 0) return BN254_OK;
    if (!d_out || n > 0x7fffffffu / 8 || (which != 0 && which != 1)) return BN254_E_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bn254_synthetic_scalars_k, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, lo, (uint32_t)n, (uint32_t)which, seed, (uint32_t *)d_out);
    return (int)hipGetLastError();
}
int bn254_tile_dev(bn254_ctx *ctx, const void *d_record, size_t record_bytes, size_t n, void *d_out, void *stream) {
    int rc = bn_get_ctx(ctx); if (rc) return rc;
    if (n == 0) return BN254_OK;
    if (!d_record || !d_out || record_bytes == 0 || record_bytes % 4) return BN254_E_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t total = (uint64_t)n * (record_bytes / 4);
    hipLaunchKernelGGL(bn254_tile_k<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)d_record, (uint32_t)(record_bytes / 4), total, (uint32_t *)d_out,
                       (const uint64_t *)nullptr, (uint64_t)0);
    return (int)hipGetLastError();
}
// d_out[i] = d_records[d_index[i]] for i < n (records of record_bytes, a multiple of 4; an index >= `records` gives an all-zero record); n * record_bytes / 4 < 2^40
int bn254_launch_gather_K(const void *d_records, size_t records, size_t record_bytes, const void *d_index, size_t n, void *d_out, hipStream_t s) {
    const uint64_t total = (uint64_t)n * (record_bytes / 4);
    hipLaunchKernelGGL(bn254_tile_k<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const uint32_t *)d_records, (uint32_t)(record_bytes / 4), total, (uint32_t *)d_out,
                       (const uint64_t *)d_index, (uint64_t)records);
    return (int)hipGetLastError();
}

}  // extern "C"
