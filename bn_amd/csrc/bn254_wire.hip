// The wire format of the BN254 engine (include/bn254_hip.h; io_wire.hpp): encode / decode kernels, one record per lane, their host-buffer
// entry points, the byte streams of variable-length records built on them, and the compressed encodings (io_compress.hpp): their kernels are
// Ops of lane_launch.hpp's bn254_fr_decode_k and - G2 decompression, which carries the subgroup test (io_wire.hpp BN254_G2_SUBGROUP_ENDO) - of this
// unit's bn254_g2_decode_k<Op>; their eight entry points are a kind table and a launch switch on record_call.hpp's one path.
// Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "curve.hpp"
#include "io.hpp"
#include "io_wire.hpp"
#include "io_compress.hpp"
#include "host_ctx.hpp"
#include "lane_launch.hpp"
#include "record_call.hpp"

using namespace bn254;

// ======================================================================================================== kernels
namespace {

constexpr int BLOCK = 64;

// wire format (io_wire.hpp): one record per lane; byte-granular global accesses (65/129-byte strides), not a hot path
__global__ void __launch_bounds__(BLOCK) bn254_g1_encode_k(const uint32_t *p, uint8_t *out, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    uint32_t w[24];
    for (int i = 0; i < 24; ++i) w[i] = p[24u * idx + i];
    g1_encode_record(w, out + 65u * idx);
}
__global__ void __launch_bounds__(BLOCK) bn254_g2_encode_k(const uint32_t *p, uint8_t *out, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    uint32_t w[48];
    for (int i = 0; i < 48; ++i) w[i] = p[48u * idx + i];
    g2_encode_record(w, out + 129u * idx);
}
__global__ void __launch_bounds__(BLOCK) bn254_g1_decode_k(const uint8_t *in, uint32_t *out, int32_t *status, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    uint8_t b[65];
    for (int i = 0; i < 65; ++i) b[i] = in[65u * idx + i];
    status[idx] = g1_decode_record(b, out + 24u * idx);
}
__global__ void __launch_bounds__(BLOCK) bn254_g2_decode_k(const uint8_t *in, uint32_t *out, int32_t *status, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    uint8_t b[129];
    for (int i = 0; i < 129; ++i) b[i] = in[129u * idx + i];
    status[idx] = g2_decode_record(b, out + 48u * idx);
}

__global__ void __launch_bounds__(BLOCK) bn254_fr_encode_k(const uint32_t *k, uint8_t *out, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    uint32_t w[8];
    for (int i = 0; i < 8; ++i) w[i] = k[8u * idx + i];
    fr_encode_record(w, out + 32u * idx);
}
__global__ void __launch_bounds__(BLOCK) bn254_fr_decode_k(const uint8_t *in, uint32_t *out, int32_t *status, uint32_t n) {
    uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= n) return;
    uint8_t b[32];
    for (int i = 0; i < 32; ++i) b[i] = in[32u * idx + i];
    status[idx] = fr_decode_record(b, out + 8u * idx);
}

// compressed encodings (io_compress.hpp): lanes [lo, lo + n) of a call, one record per lane
struct G1CompressOp {
    const uint32_t *p; uint8_t *out; uint64_t lo; uint32_t n; int format;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
        if (i >= n) return;
        uint32_t w[24];
        for (int j = 0; j < 24; ++j) w[j] = p[24 * (lo + i) + j];
        g1_compress_record(w, format, out + BN254_G1_COMPRESSED_BYTES * (lo + i));
    }
};
struct G2CompressOp {
    const uint32_t *p; uint8_t *out; uint64_t lo; uint32_t n; int format;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
        if (i >= n) return;
        uint32_t w[48];
        for (int j = 0; j < 48; ++j) w[j] = p[48 * (lo + i) + j];
        g2_compress_record(w, format, out + BN254_G2_COMPRESSED_BYTES * (lo + i));
    }
};
struct G1DecompressOp {
    const uint8_t *in; uint32_t *out; int32_t *status; uint64_t lo; uint32_t n; int format;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
        if (i >= n) return;
        status[lo + i] = g1_decompress_record(in + BN254_G1_COMPRESSED_BYTES * (lo + i), format, out + 24 * (lo + i));
    }
};
struct G2DecompressOp {
    const uint8_t *in; uint32_t *out; int32_t *status; uint64_t lo; uint32_t n; int format;
    __device__ __forceinline__ void operator()() const {
        const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
        if (i >= n) return;
        status[lo + i] = g2_decompress_record(in + BN254_G2_COMPRESSED_BYTES * (lo + i), format, out + 48 * (lo + i));
    }
};
// the one Op with a shell of its own name: G2DecompressOp, held under the spill ceiling of bn254_g2_decode_k (the wire decoder above shares the name)
template <class Op>
__global__ void __launch_bounds__(BLOCK) bn254_g2_decode_k(Op op) { op(); }

}  // namespace

// wire format: host buffers in, host buffers out
static int wire_host(bn254_ctx *ctx, int g, int decode, const void *in, void *out, int32_t *status, size_t n) {
    if (n == 0) return BN254_OK;
    if (!in || !out || (decode && !status) || n > 0x7fffffffu / 129) return BN254_E_BAD_ARG;
    BnHost h(ctx); if (h.rc) return h.rc;
    const size_t ps = g == 0 ? sizeof(bn_fr) : g == 1 ? sizeof(bn_g1) : sizeof(bn_g2), rs = g == 0 ? BN254_FR_WIRE_BYTES : g == 1 ? BN254_G1_WIRE_BYTES : BN254_G2_WIRE_BYTES;
    return bn_staged(ctx, {in, n * (decode ? rs : ps)}, {}, out, n * (decode ? ps : rs), decode ? status : nullptr, n * sizeof(int32_t), [&](const BnStaged &d) -> int {
        BnScope sc(ctx, ctx->stream, decode ? "wire_decode" : "wire_encode");
        dim3 grid((unsigned)((n + BLOCK - 1) / BLOCK)), block(BLOCK);
        if (g == 0 && !decode) hipLaunchKernelGGL(bn254_fr_encode_k, grid, block, 0, ctx->stream, (const uint32_t *)d.in[0], (uint8_t *)d.out, (uint32_t)n);
        if (g == 0 && decode) hipLaunchKernelGGL(bn254_fr_decode_k, grid, block, 0, ctx->stream, (const uint8_t *)d.in[0], (uint32_t *)d.out, (int32_t *)d.out2, (uint32_t)n);
        if (g == 1 && !decode) hipLaunchKernelGGL(bn254_g1_encode_k, grid, block, 0, ctx->stream, (const uint32_t *)d.in[0], (uint8_t *)d.out, (uint32_t)n);
        if (g == 2 && !decode) hipLaunchKernelGGL(bn254_g2_encode_k, grid, block, 0, ctx->stream, (const uint32_t *)d.in[0], (uint8_t *)d.out, (uint32_t)n);
        if (g == 1 && decode) hipLaunchKernelGGL(bn254_g1_decode_k, grid, block, 0, ctx->stream, (const uint8_t *)d.in[0], (uint32_t *)d.out, (int32_t *)d.out2, (uint32_t)n);
        if (g == 2 && decode) hipLaunchKernelGGL(bn254_g2_decode_k, grid, block, 0, ctx->stream, (const uint8_t *)d.in[0], (uint32_t *)d.out, (int32_t *)d.out2, (uint32_t)n);
        return (int)hipGetLastError();
    });
}

extern "C" {

int bn254_fr_encode_batch(bn254_ctx *ctx, const bn_fr *k, uint8_t *out, size_t n) { return wire_host(ctx, 0, 0, k, out, nullptr, n); }
int bn254_fr_decode_batch(bn254_ctx *ctx, const uint8_t *in, bn_fr *out, int32_t *status, size_t n) { return wire_host(ctx, 0, 1, in, out, status, n); }
int bn254_g1_encode_batch(bn254_ctx *ctx, const bn_g1 *p, uint8_t *out, size_t n) { return wire_host(ctx, 1, 0, p, out, nullptr, n); }
int bn254_g2_encode_batch(bn254_ctx *ctx, const bn_g2 *p, uint8_t *out, size_t n) { return wire_host(ctx, 2, 0, p, out, nullptr, n); }
int bn254_g1_decode_batch(bn254_ctx *ctx, const uint8_t *in, bn_g1 *out, int32_t *status, size_t n) { return wire_host(ctx, 1, 1, in, out, status, n); }
int bn254_g2_decode_batch(bn254_ctx *ctx, const uint8_t *in, bn_g2 *out, int32_t *status, size_t n) { return wire_host(ctx, 2, 1, in, out, status, n); }
// ---- the crate's actual byte STREAM (groups/mod.rs:143-205): a point at infinity is the lone byte 0, a finite point is 4 followed by
// its coordinates - records of variable length.  The stream is cut into records on the host (a tag decides the length), the fixed
// records go through the batch kernels above.
static int stream_encode(bn254_ctx *ctx, int g, const void *p, size_t n, uint8_t *out, size_t cap, size_t *written) {
    if (!written || (n && (!p || !out))) return BN254_E_BAD_ARG;
    const size_t rs = g == 1 ? BN254_G1_WIRE_BYTES : BN254_G2_WIRE_BYTES;
    return bn_no_throw([&]() -> int {
        std::vector<uint8_t> fixed(n * rs);
        int rc = g == 1 ? bn254_g1_encode_batch(ctx, (const bn_g1 *)p, fixed.data(), n) : bn254_g2_encode_batch(ctx, (const bn_g2 *)p, fixed.data(), n);
        if (rc) return rc;
        size_t w = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t *r = fixed.data() + i * rs;
            const size_t len = r[0] == 0 ? 1 : rs;
            if (w + len > cap) return BN254_E_BAD_ARG;
            memcpy(out + w, r, len);
            w += len;
        }
        *written = w;
        return BN254_OK;
    });
}
static int stream_decode(bn254_ctx *ctx, int g, const uint8_t *in, size_t len, void *out, int32_t *status, size_t max_points, size_t *count, size_t *consumed) {
    if (!count || !consumed || (len && !in) || (max_points && (!out || !status))) return BN254_E_BAD_ARG;
    const size_t rs = g == 1 ? BN254_G1_WIRE_BYTES : BN254_G2_WIRE_BYTES;
    { int rc0 = bn_get_ctx(ctx); if (rc0) return rc0; }
    return bn_no_throw([&]() -> int {
        std::vector<uint8_t> fixed;
        std::vector<size_t> ends;                                   // stream position behind every record
        size_t pos = 0, n = 0;
        while (pos < len && n < max_points) {
            // tag 0: one byte; tag 4: a full record; any other tag is the crate's "invalid leading byte" - it consumes the byte it read
            const size_t rec = in[pos] == 4 ? rs : 1;
            if (pos + rec > len) break;                         // truncated record: stop in front of it
            fixed.resize((n + 1) * rs, 0);
            memcpy(fixed.data() + n * rs, in + pos, rec);
            pos += rec; ++n;
            ends.push_back(pos);
        }
        int rc = g == 1 ? bn254_g1_decode_batch(ctx, fixed.data(), (bn_g1 *)out, status, n) : bn254_g2_decode_batch(ctx, fixed.data(), (bn_g2 *)out, status, n);
        if (rc) return rc;
        if (bn_opt(ctx, BN254_OPT_STREAM_STOP_AT_ERROR) == 1)      // the crate's own behaviour: Decodable returns Err at the first bad record
            for (size_t i = 0; i < n; ++i)
                if (status[i] != 0) { n = i + 1; pos = ends[i]; break; }
        *count = n; *consumed = pos;
        return BN254_OK;
    });
}
int bn254_g1_encode_stream(bn254_ctx *ctx, const bn_g1 *p, size_t n, uint8_t *out, size_t cap, size_t *written) { return stream_encode(ctx, 1, p, n, out, cap, written); }
int bn254_g2_encode_stream(bn254_ctx *ctx, const bn_g2 *p, size_t n, uint8_t *out, size_t cap, size_t *written) { return stream_encode(ctx, 2, p, n, out, cap, written); }
int bn254_g1_decode_stream(bn254_ctx *ctx, const uint8_t *in, size_t len, bn_g1 *out, int32_t *status, size_t max_points, size_t *count, size_t *consumed) {
    return stream_decode(ctx, 1, in, len, out, status, max_points, count, consumed);
}
int bn254_g2_decode_stream(bn254_ctx *ctx, const uint8_t *in, size_t len, bn_g2 *out, int32_t *status, size_t max_points, size_t *count, size_t *consumed) {
    return stream_decode(ctx, 2, in, len, out, status, max_points, count, consumed);
}

}  // extern "C"

// ---- compressed encodings -------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t WIRE_N_MAX = 0x7fffffffu / 129;            // the wire layer's limit on the records of one call
BnLaunchMax g_compress_launch_max;          // tests only: the sub-launch size

// the family's kinds (record_call.hpp): scope, the input and the bytes of one record of it, of the output, of the decoders' status
enum { CMP_G1_COMPRESS, CMP_G2_COMPRESS, CMP_G1_DECOMPRESS, CMP_G2_DECOMPRESS, CMP_KINDS };
constexpr BnRecordKind CMP_KIND[CMP_KINDS] = {{"g1_compress", 1, {sizeof(bn_g1)}, BN254_G1_COMPRESSED_BYTES, 0}, {"g2_compress", 1, {sizeof(bn_g2)}, BN254_G2_COMPRESSED_BYTES, 0},
                                              {"g1_decompress", 1, {BN254_G1_COMPRESSED_BYTES}, sizeof(bn_g1), sizeof(int32_t)}, {"g2_decompress", 1, {BN254_G2_COMPRESSED_BYTES}, sizeof(bn_g2), sizeof(int32_t)}};
struct CompressLaunch {
    int what, format;
    int operator()(const BnRecordArgs &a, size_t lo, size_t cnt, hipStream_t s) const {
        switch (what) {
        case CMP_G1_COMPRESS: return bn_lane_launch<BLOCK>(G1CompressOp{(const uint32_t *)a.in[0], (uint8_t *)a.out, (uint64_t)lo, (uint32_t)cnt, format}, cnt, s);
        case CMP_G2_COMPRESS: return bn_lane_launch<BLOCK>(G2CompressOp{(const uint32_t *)a.in[0], (uint8_t *)a.out, (uint64_t)lo, (uint32_t)cnt, format}, cnt, s);
        case CMP_G1_DECOMPRESS: return bn_lane_launch<BLOCK>(G1DecompressOp{(const uint8_t *)a.in[0], (uint32_t *)a.out, (int32_t *)a.out2, (uint64_t)lo, (uint32_t)cnt, format}, cnt, s);
        default:
            hipLaunchKernelGGL(bn254_g2_decode_k<G2DecompressOp>, dim3((unsigned)((cnt + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                               G2DecompressOp{(const uint8_t *)a.in[0], (uint32_t *)a.out, (int32_t *)a.out2, (uint64_t)lo, (uint32_t)cnt, format});
            return (int)hipGetLastError();
        }
    }
};
// the two forms of a call of kind `what`: the format first, then the shared checks (up to the wire layer's limit), sub-launches and staging
bool compress_format_ok(int format) { return format == BN254_COMPRESSED_ARK || format == BN254_COMPRESSED_GNARK; }
int compress_host(bn254_ctx *ctx, int what, int format, const BnRecordArgs &a, size_t n) {
    return compress_format_ok(format) ? bn_record_host(ctx, CMP_KIND[what], g_compress_launch_max, a, n, CompressLaunch{what, format}, WIRE_N_MAX) : BN254_E_BAD_ARG;
}
int compress_dev(bn254_ctx *ctx, int what, int format, const BnRecordArgs &a, size_t n, void *stream) {
    return compress_format_ok(format) ? bn_record_dev(ctx, CMP_KIND[what], g_compress_launch_max, a, n, stream, CompressLaunch{what, format}, WIRE_N_MAX) : BN254_E_BAD_ARG;
}
}  // namespace

extern "C" {

int bn254_g1_compress_batch(bn254_ctx *ctx, const bn_g1 *p, int format, uint8_t *out, size_t n) { return compress_host(ctx, CMP_G1_COMPRESS, format, {{p}, out}, n); }
int bn254_g2_compress_batch(bn254_ctx *ctx, const bn_g2 *p, int format, uint8_t *out, size_t n) { return compress_host(ctx, CMP_G2_COMPRESS, format, {{p}, out}, n); }
int bn254_g1_decompress_batch(bn254_ctx *ctx, const uint8_t *in, int format, bn_g1 *out, int32_t *status, size_t n) { return compress_host(ctx, CMP_G1_DECOMPRESS, format, {{in}, out, status}, n); }
int bn254_g2_decompress_batch(bn254_ctx *ctx, const uint8_t *in, int format, bn_g2 *out, int32_t *status, size_t n) { return compress_host(ctx, CMP_G2_DECOMPRESS, format, {{in}, out, status}, n); }
int bn254_g1_compress_batch_dev(bn254_ctx *ctx, const void *d_p, int format, void *d_out, size_t n, void *stream) { return compress_dev(ctx, CMP_G1_COMPRESS, format, {{d_p}, d_out}, n, stream); }
int bn254_g2_compress_batch_dev(bn254_ctx *ctx, const void *d_p, int format, void *d_out, size_t n, void *stream) { return compress_dev(ctx, CMP_G2_COMPRESS, format, {{d_p}, d_out}, n, stream); }
int bn254_g1_decompress_batch_dev(bn254_ctx *ctx, const void *d_in, int format, void *d_out, void *d_status, size_t n, void *stream) { return compress_dev(ctx, CMP_G1_DECOMPRESS, format, {{d_in}, d_out, d_status}, n, stream); }
int bn254_g2_decompress_batch_dev(bn254_ctx *ctx, const void *d_in, int format, void *d_out, void *d_status, size_t n, void *stream) { return compress_dev(ctx, CMP_G2_DECOMPRESS, format, {{d_in}, d_out, d_status}, n, stream); }

// internal (not in the header; tests and tools/time_compress.py): an override of the sub-launch size of the eight calls above (0 restores
// BN_LAUNCH_MAX) so that a test reaches the seam between two sub-launches with a handful of records, and which chain form the square roots run
int bn254_compress_set_launch_max(size_t lanes) { return g_compress_launch_max.set(lanes); }
int bn254_compress_sqrt_window(void) { return BN254_SQRT_WINDOW; }
// internal (tools/time_validate.py): which membership test the G2 decoders of this library run - 1 the endomorphism test, 0 the r - 1 chain
int bn254_wire_subgroup_endo(void) { return BN254_G2_SUBGROUP_ENDO; }

}  // extern "C"
