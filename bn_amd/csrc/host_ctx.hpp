// Host-side internals shared by the translation units that implement include/bn254_hip.h (bn254_hip.hip: contexts, options, launch
// policy and the single-device entry points of pairing, Miller loop, final exponentiation and products; bn254_seg.hip: the segmented
// multi-pairings and the multi-scalar multiplications; bn254_wire.hip: the wire format; bn254_multi.hip: pipelined host-buffer path,
// multi-device fan-out, RCCL exchange; bn254_{fr,ntt,dot,scan,mle,poseidon,hash,babyjub,grumpkin}.hip: the families of integer kernels over Fr, hash-to-curve and the curves over Fr,
// each with its Ops and entry points).  The host arithmetic that needs no device is host_plan.hpp; the kernel shell, the launchers and the
// overrides of the integer kernels are lane_launch.hpp; the one call path of the record-per-lane families is record_call.hpp.  Not part of the ABI.
//
// Concurrency contract (what the header promises and these structures implement):
//   * any number of host threads may call the HOST-BUFFER entry points of one context - including the process-wide default
//     contexts behind ctx == NULL (one per HIP device) - and get the reference's re-entrant behaviour (`pairing` is a pure
//     function, `Group: Send + Sync`, src/lib.rs:55-61): the batch entry points (pairing_batch, g*_mul_batch) lease one of two
//     pipeline slots per call (own stream, staging and table; multi-chunk batches lease all slots), the others lock the context;
//   * the asynchronous *_dev entry points share context-owned scratch (final-exponentiation table, product workspace).
//     Each use is bracketed by an event: a launch on another stream first waits for the previous user's event, so two
//     streams on one context serialise on the scratch instead of racing on it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <map>
#include <new>
#include <optional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bn254_hip.h"
#include "host_plan.hpp"

#define HIP_TRY(expr)                             \
    do {                                          \
        hipError_t e__ = (expr);                  \
        if (e__ != hipSuccess) return (int)e__;   \
    } while (0)

// restores the calling thread's current HIP device when an entry point returns (the library switches to the context's device)
struct BnDeviceGuard {
    int prev = -1;
    BnDeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~BnDeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};
// nothing may unwind across the C ABI: entry points that create threads / containers run their body through this
template <class Fn>
int bn_no_throw(Fn &&fn) {
    try { return fn(); } catch (const std::bad_alloc &) { return BN254_E_ALLOC; } catch (...) { return BN254_E_INTERNAL; }
}

#ifndef BN254_HAVE_QUAD
#define BN254_HAVE_QUAD 1        // the four-lanes-per-pairing kernels (bn254_kernels_q.hip) are linked in
#endif
constexpr int BN_MAX_SLOTS = 4;            // chunks in flight in the pipelined host-buffer path (2 used; the rest for experiments)

// grow-only buffer, device or pinned host
struct BnBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    int reserve(size_t need) {
        if (need == 0) need = 1;
        if (bytes >= need) return BN254_OK;
        release();
        hipError_t e = pinned ? hipHostMalloc(&p, need, hipHostMallocDefault) : hipMalloc(&p, need);
        if (e != hipSuccess) { p = nullptr; return BN254_E_ALLOC; }
        bytes = need;
        return BN254_OK;
    }
    void release() {
        if (p) { if (pinned) hipHostFree(p); else hipFree(p); }
        p = nullptr; bytes = 0;
    }
};

// one chunk in flight: its own stream, device staging and final-exponentiation table
struct BnSlot {
    hipStream_t stream = nullptr;
    BnBuf d_in[2], d_out, tbl;
};

// Fixed-base tables of bn254_g{1,2}_mul_base_batch: per group a small LRU of device tables keyed by the raw bytes of the base they were built
// from (and the window width).  Context-owned scratch like ws / exp_tbl: looked up, built and read under the BnScratchGuard of the call, so a
// slot is rebuilt only by a stream that has waited for the last launch that may read it.
constexpr int BN_BASE_SLOTS = 4;
// signed window width of the tables, per group: the fastest of the measured 8 / 10 / 12 (profiles/r11_mul_base.txt: G1 2^20 scalars
// 2.84 / 2.41 / 2.13 ms, G2 2^18 scalars 2.06 / 1.71 / 1.50 ms of kernel time)
constexpr unsigned BN_BASE_WINDOW_G1 = 12, BN_BASE_WINDOW_G2 = 12;
struct BnBaseSlot {
    BnBuf table;                        // W * 2^(c-1) entries of 80 (G1) / 160 (G2) bytes (group_ops.hpp base_mul_body)
    unsigned char key[sizeof(bn_g2)];   // the base as the caller passed it: 96 or 192 bytes
    unsigned c = 0;                     // window width the table was built for
    bool valid = false;
    uint64_t used = 0;                  // tick of the last call that used it
};
struct BnBaseCache {
    BnBaseSlot slot[BN_BASE_SLOTS];     // tables are allocated on first use
    uint64_t tick = 0;
    BnBuf scal;                         // the scalars d * 2^(c w) the tables are built with, for window width scal_c ...
    std::vector<uint64_t> scal_host;    // ... and their host image (kept while the copy may be in flight)
    long scal_c = -1;
};

struct bn254_ctx {
    int device = 0;
    int cus = 256;                      // compute units of the device (sizes one "round" of the lane-pair kernels: bn_round_pairs)
    std::atomic<long> opt[BN254_OPT_COUNT_];   // bn254_ctx_set_option: raw values, < 0 = "derive the default from the device" (bn_opt)
    std::mutex mu;                      // host-buffer entry points hold it for the whole call
    std::mutex scratch_mu;              // guards the scratch bookkeeping below (held only while enqueueing)
    hipStream_t stream = nullptr;       // the context's own stream (host-buffer entry points)
    BnBuf ws;                           // workspace (Miller values, product-tree levels)
    BnBuf exp_tbl;                      // odd-power tables of the windowed exponentiation by u (final_exp_B)
    BnBuf pow_tbl;                      // window tables of Gt::pow (gt_pow_B)
    BnBuf mul_tbl;                      // affine window tables of the scalar-multiplication kernels (one sub-launch)
    BnBuf miller_state;                 // running points of the shared-accumulator Miller loop (miller_shared*_B), one round
    hipEvent_t scratch_ev = nullptr;    // completion of the last launch that used ws / exp_tbl ...
    hipStream_t scratch_stream = nullptr;   // ... and the stream it ran on
    bool scratch_used = false;
    BnBuf seg_plan;                     // work lists of the segmented fold (bn254_pairing_product_batch*, behind them the Miller pieces of ..._prepared_native) and of bn254_fr_dot_batch and bn254_fr_scan_batch, device side ...
    BnBuf seg_plan_host{nullptr, 0, true};  // ... and their pinned staging, rewritten only after seg_plan_ev (its last copy) completed
    hipEvent_t seg_plan_ev = nullptr;
    BnBuf msm_ws;                       // bucket route of bn254_g{1,2}_msm: counts, sorted indices and keys, buckets, partial sums, tail terms
    BnBuf msm_scal;                     // ... and the tail's scalars (Montgomery images of 2^(c w) and base * 2^(c w)) for window width msm_scal_c
    std::vector<uint64_t> msm_scal_host;    // their host image (kept while the copy may be in flight; rebuilt only when the width changes)
    long msm_scal_c = -1;
    BnBuf msmp_scal;                    // bn254_g{1,2}_msm_prepared: the tail's scalars (base + 1 and 1) for window width msmp_scal_c, kept like msm_scal
    std::vector<uint64_t> msmp_scal_host;
    long msmp_scal_c = -1;
    BnBaseCache base_cache[2];          // bn254_g{1,2}_mul_base_batch: [0] G1, [1] G2
    BnBuf norm_prefix;                  // bn254_g{1,2}_normalize_batch: the prefix products of one sub-launch (48 / 96 bytes per point)
    BnBuf fr_prefix;                    // bn254_fr_inverse_batch: the prefix products of one sub-launch (32 bytes per element)
    BnBuf ntt_tbl;                      // bn254_fr_ntt_batch: two table pairs of 2 * 2^12 Fr (ntt_ops.hpp) - the powers of w_24, built once, ...
    bool ntt_root_ready = false;
    uint64_t ntt_shift_key[5] = {};     // ... and the powers of the coset shift the second pair was built for (forward: the shift; inverse: shift and size)
    bool ntt_shift_valid = false;
    BnBuf ntt_ws;                       // the arrays between the passes of one group of transforms (one, or two for an odd number of passes in place)
    BnBuf gntt_ws;                      // bn254_g{1,2}_ntt_batch: the array of Jacobian points between the stages of one group of transforms
    BnBuf dot_ws;                       // bn254_fr_dot_batch: the partial sums of the segments longer than one piece (32 bytes each; its work list travels through seg_plan)
    BnBuf scan_ws;                      // bn254_fr_scan_batch: per scratch slot of its plan a map (A, B) and a carry, three arrays of 32-byte records (its work list travels through seg_plan)
    BnBuf grk_ws;                       // bn254_grumpkin_msm_batch: the projective partial sums of the segments of more than one term (96 bytes each; its work list travels through seg_plan)
    BnBuf mle_ws;                       // bn254_fr_sumcheck_round: the partial sums of the round kernel's lanes and of the sum levels, [t][lane] per level (32 bytes each)
    BnBuf psd_wide_tbl[16];             // bn254_fr_poseidon_ex_batch / _chain_batch: the constants of width t = 2 .. 17 ([t - 2]; poseidon_wide_table.hpp), derived and
    bool psd_wide_ready[16] = {};       // ... uploaded with a blocking copy at the first use of the width, under psd_wide_mu; read-only afterwards
    std::mutex psd_wide_mu;             // (its own mutex: the host-buffer forms hold `mu` while they call their _dev twins)
    BnBuf base_stage;                   // the base of a table build on the device ...
    BnBuf base_stage_host{nullptr, 0, true};    // ... and its pinned staging, rewritten only after base_stage_ev (its last copy) completed
    hipEvent_t base_stage_ev = nullptr;
    BnBuf stage[4];                     // device staging of the small host-buffer entry points (bn_staged_n: [0] the inputs, [2] and [3] the outputs; [0] and [1] also serve the calls that stage by hand)
    BnSlot slot[BN_MAX_SLOTS];          // pipelined path (bn254_multi.hip)
    // leases of those slots: a batch of up to one chunk takes ONE of the first two (two callers overlap on the GPU - the number
    // of streams the hardware overlaps without loss), a multi-chunk batch takes all of them
    std::mutex slot_mu;
    std::condition_variable slot_cv;
    unsigned slot_busy = 0;             // bit i: slot i is leased
    int slot_waiting_all = 0;           // callers waiting for every slot (new single leases queue behind them)
    std::atomic<bool> profile{false};   // read by every launch helper, possibly from several host threads
    std::mutex prof_mu;                 // recs / folded (worker threads of the pipelined path launch concurrently)
    struct Rec { std::string name; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::map<std::string, std::pair<double, uint64_t>> folded;     // totals of records already consumed (events recycled)
};

// bn254_g2_prepare: the native line table of `nq` G2 points (bn254_kernels_b.hip NativeTableMem) and their infinity flags, in device memory
struct bn254_g2_prepared {
    int device = 0;
    size_t nq = 0;
    void *table = nullptr;
    void *inf = nullptr;
    size_t bytes = 0;
    // the points themselves (192 B each; ONE point: repeated `small_max` times), for calls small enough that the one-pairing-per-wave kernels of
    // the general path beat the lane-pair latency of the native Miller loop (bn254_pairing_prepared_native_batch_dev)
    void *q = nullptr;
    size_t small_max = 0;
};

// bn254_g{1,2}_msm_prepare: the affine multiples 2^(c w) P_i of `count` points (entry (w, i) at index w * count + i, the records of
// group_ops.hpp) and the normalised points themselves, in device memory.  Behind the header's `void *`.
struct bn254_msm_prepared {
    int device = 0;
    int group = 0;                      // 1 or 2
    unsigned c = 0, W = 0;              // window width, windows
    size_t count = 0;
    void *table = nullptr;              // W * count entries
    void *pts = nullptr;                // count points of 96 / 192 bytes: the small route's
    size_t table_bytes = 0;
};
// terms from which bn254_g{1,2}_msm_prepared take their bucket route while BN254_OPT_MSM_BUCKET_MIN is not set: the smallest measured size
// from which the route's [min, max] of kernel time lies wholly below the small route's at that size and at every larger one
// (tools/time_msm_prepared.py --crossover, profiles/r29_msm_prepared.txt, every power of two from 2^10 to 2^20 at the default width:
// G1 bucket / small 1.08 at 2^18, 0.72 at 2^19, 0.54 at 2^20; G2 1.00 at 2^17 - the two ranges overlap -, 0.66 at 2^18, 0.35 at 2^20)
constexpr long BN_MSMP_BUCKET_MIN_DEFAULT = (long)1 << 19, BN_MSMP_BUCKET_MIN_DEFAULT_G2 = (long)1 << 18;

// lease of pipeline slots for one host-buffer call (see bn254_ctx::slot_busy)
struct BnSlotLease {
    bn254_ctx *c; unsigned mask; int first;
    BnSlotLease(bn254_ctx *c_, bool all) : c(c_), mask(0), first(0) {
        std::unique_lock<std::mutex> lk(c->slot_mu);
        if (all) {
            ++c->slot_waiting_all;
            c->slot_cv.wait(lk, [&] { return c->slot_busy == 0; });
            --c->slot_waiting_all;
            mask = (1u << BN_MAX_SLOTS) - 1;
        } else {
            c->slot_cv.wait(lk, [&] { return c->slot_waiting_all == 0 && (c->slot_busy & 3u) != 3u; });
            first = (c->slot_busy & 1u) ? 1 : 0;
            mask = 1u << first;
        }
        c->slot_busy |= mask;
    }
    ~BnSlotLease() {
        { std::lock_guard<std::mutex> lk(c->slot_mu); c->slot_busy &= ~mask; }
        c->slot_cv.notify_all();
    }
};

// brackets one kernel launch with events when profiling is on
struct BnScope {
    bn254_ctx *c; hipStream_t s; bool on; hipEvent_t a, b; const char *name;
    BnScope(bn254_ctx *c_, hipStream_t s_, const char *n);
    ~BnScope();
};

int bn_get_ctx(bn254_ctx *&ctx);                                   // NULL -> the default context of the current device
long bn_opt(const bn254_ctx *c, int key);                          // EFFECTIVE value of a BN254_OPT_* tunable (defaults from the CU count)
int bn_debug_multi_exchange();                                     // BN254_EXCHANGE_AUTO unless the debug environment forces one (read once)
bool bn_debug_multi_affinity();                                    // false only when the debug environment says BN254_MULTI_AFFINITY=0
// scratch guard: lives across the enqueueing of work that reads/writes ctx->ws / ctx->exp_tbl on stream `s`
struct BnScratchGuard {
    bn254_ctx *c; hipStream_t s; int rc;
    BnScratchGuard(bn254_ctx *c_, hipStream_t s_);       // locks the bookkeeping, makes `s` wait for the previous user
    ~BnScratchGuard();                                   // records the completion event on `s`, unlocks
};

// kernel launch helpers (bn254_hip.hip); `table` = caller-provided final-exponentiation table or NULL for the context's own
size_t bn_round_pairs(const bn254_ctx *c);                        // pairings in one full-machine launch of the lane-pair kernels
size_t bn_sub_launch(const bn254_ctx *c, size_t n);                // sub-launch size for a batch of n (equal parts, none above one round)
int bn_launch_miller(bn254_ctx *c, const void *p, const void *q, void *f, size_t n, hipStream_t s, bool naf);
int bn_launch_pairing(bn254_ctx *c, const void *p, const void *q, void *out, size_t n, hipStream_t s, BnBuf *table);
int bn_launch_final_exp(bn254_ctx *c, const void *f, void *out, size_t n, hipStream_t s, BnBuf *table);
int bn_launch_product_final_exp(bn254_ctx *c, const void *in, size_t m, void *out, hipStream_t s);   // scratch guard held by the caller
int bn_launch_product(bn254_ctx *c, const void *in, size_t n, void *out, void *tmp, hipStream_t s);
size_t bn_product_tmp_bytes(const bn254_ctx *c, size_t n);
// table: the caller's own buffer (pipelined path: the slot's) or NULL for the context's (then under a BnScratchGuard)
int bn_mul_dev(bn254_ctx *ctx, int g, const void *d_p, const void *d_k, void *d_out, size_t n, hipStream_t s, int normalize, BnBuf *table = nullptr);
// terms from which bn254_g{1,2}_msm take the bucket route while BN254_OPT_MSM_BUCKET_MIN is not set: the smallest measured size from which
// the route is faster in kernel time than the one-segment bn254_g{1,2}_msm_batch and stays faster above (profiles/r10_msm_bucket.txt: G1
// 0.73 x at 2^18, 1.06 x at 2^19, 1.33 x at 2^20; G2 0.77 x at 2^17, 1.14 x at 2^18, 1.55 x at 2^19).  bn254_ctx_get_option reports G1's.
constexpr long BN_MSM_BUCKET_MIN_DEFAULT = (long)1 << 19, BN_MSM_BUCKET_MIN_DEFAULT_G2 = (long)1 << 18;
// The normalising kernels keep every lane's window table (640 B) in a buffer the sub-launches reuse.  Sub-launches of 2^20 lanes (671 MB; rounds
// 2-5: 2^18): these kernels run three resident waves per SIMD under plain oldest-first arbitration, a launch ends with every SIMD draining its last
// wave alone, and that tail is paid once per launch - 2^20 G1 multiplications in ONE launch of 16 waves per SIMD: 91.1 against 86.7 M/s in four
// launches on the same box, G2 +2 % (profiles/r06_ab_mul_launch_size.txt).
constexpr size_t BN_MUL_LANES_PER_LAUNCH = (size_t)1 << 20;
size_t bn_wave_pairing_max(const bn254_ctx *c);                    // BN254_OPT_WAVE_PAIRING_MAX: up to this many pairings per call run one per wave
size_t bn_wave_fe_max(const bn254_ctx *c);                         // BN254_OPT_WAVE_FE_MAX: the same for final exponentiations
// calls over a prepared handle of up to this many pairs take the general path on the points kept with the handle
size_t bn_prepared_small_max(const bn254_ctx *c, const bn254_g2_prepared *prep);

// Prologue of the *_dev entry points: `BnDev d(...); if (!d.go) return d.rc;` makes the context's device current until the entry point
// returns (the caller's is restored then) and gives the caller's stream.  The second form is the order of the plain batch entry points:
// context, empty batch (nothing to do: rc = BN254_OK), arguments, device.
struct BnDev {
    std::optional<BnDeviceGuard> guard;
    int rc = BN254_OK;
    bool go = false;
    hipStream_t s = nullptr;
    BnDev() {}
    BnDev(bn254_ctx *ctx, void *stream) { enter(ctx, (hipStream_t)stream); }
    BnDev(bn254_ctx *&ctx, void *stream, size_t n, bool bad_arg, size_t limit) {
        if ((rc = bn_get_ctx(ctx)) || n == 0) return;
        if (bad_arg || n > limit) { rc = BN254_E_BAD_ARG; return; }
        enter(ctx, (hipStream_t)stream);
    }
    void enter(bn254_ctx *ctx, hipStream_t stream) {
        guard.emplace();
        rc = (int)hipSetDevice(ctx->device);
        go = !rc; s = stream;
    }
};
// The _dev prologue after the argument checks: context, device, the scratch guard where the call uses context-owned scratch, then
// fn(stream) with nothing thrown across the ABI (nothing waits, nothing is read back)
template <class Fn>
int bn_dev_entry(bn254_ctx *&ctx, void *stream, bool scratch, Fn fn) {
    int rc = bn_get_ctx(ctx); if (rc) return rc;
    BnDev d(ctx, stream); if (!d.go) return d.rc;
    if (!scratch) return bn_no_throw([&] { return fn(d.s); });
    BnScratchGuard g(ctx, d.s); if (g.rc) return g.rc;
    return bn_no_throw([&] { return fn(d.s); });
}
// Work lists (ctx->seg_plan): ONE copy of a || b per call through the context's pinned staging, which is rewritten only after its previous
// copy completed - so the caller's host arrays may be freed as soon as the call returns.  Scratch guard held by the caller (bn254_hip.hip;
// hidden: the library's list of dynamic symbols stays what it was).
__attribute__((visibility("hidden"))) int bn_plan_upload(bn254_ctx *c, const void *a, size_t a_bytes, const void *b, size_t b_bytes, hipStream_t s);
// The twiddle tables of bn254_fr_ntt_batch for the transforms over G1 / G2 (bn254_ntt.hip; hidden like bn_plan_upload): builds the root pair
// on first use and, for a shift, the shift pair when its key changed.  ctx->ntt_tbl holds the root pair, then the shift pair, of
// 2 * 2^12 records each (ntt_ops.hpp).  Scratch guard held by the caller.
__attribute__((visibility("hidden"))) int bn_ntt_tables(bn254_ctx *c, int log_n, int inverse, const bn_fr *shift, hipStream_t s);
// Prologue of the host-buffer entry points that lock the context: looks the context up, holds its mutex for the whole call - concurrent
// callers of one context (in particular of the default context behind ctx == NULL) are serialised, never interleaved on the staging
// memory -, makes its device current.  `BnHost h(ctx); if (h.rc) return h.rc;`
struct BnHost {
    std::unique_lock<std::mutex> lock;
    BnDev dev;
    int rc;
    explicit BnHost(bn254_ctx *&ctx) {
        if ((rc = bn_get_ctx(ctx))) return;
        lock = std::unique_lock<std::mutex>(ctx->mu);
        dev.enter(ctx, ctx->stream);
        rc = dev.rc;
    }
};
// The body of a host-buffer entry point of the shape copy-in, device calls, copy-out, synchronise, on the context's stream under a BnHost:
// the inputs (skipped when NULL; nothing copied for zero bytes) are staged one after the other in ctx->stage[0], each at a multiple of
// BN_STAGE_ALIGN bytes - an allocation's own alignment, so an input of any size leaves the next one as aligned as a buffer of its own -,
// body(d) enqueues the work on the staged inputs d.in[] (NULL for a skipped one) and the device buffers d.out / d.out2 (ctx->stage[2],
// ctx->stage[3]), then `out` (and `out2` when given) are copied back.
// On an error the stream is drained first: copies that read or write the caller's buffers may still be in flight.
// bn_staged_n is the one implementation of that sequence; bn_staged is its form for up to three inputs written out as arguments.
constexpr int BN_STAGE_INS = 4;
constexpr size_t BN_STAGE_ALIGN = 256;
struct BnStageIn { const void *p; size_t bytes; };
struct BnStaged { void *in[BN_STAGE_INS], *out, *out2; };
template <class Body>
int bn_staged_n(bn254_ctx *ctx, const BnStageIn *in, int n_in, void *out, size_t out_bytes, void *out2, size_t out2_bytes, Body body) {
    const hipStream_t s = ctx->stream;
    if (n_in > BN_STAGE_INS) return BN254_E_INTERNAL;
    auto run = [&]() -> int {
        int rc;
        size_t at[BN_STAGE_INS], total = 0;
        for (int i = 0; i < n_in; ++i) {
            at[i] = total;
            if (in[i].p) total += (in[i].bytes + BN_STAGE_ALIGN - 1) / BN_STAGE_ALIGN * BN_STAGE_ALIGN;
        }
        if ((rc = ctx->stage[0].reserve(total)) || (rc = ctx->stage[2].reserve(out_bytes)) || (out2 && (rc = ctx->stage[3].reserve(out2_bytes)))) return rc;
        BnStaged d = {};
        d.out = ctx->stage[2].p; d.out2 = out2 ? ctx->stage[3].p : nullptr;
        for (int i = 0; i < n_in; ++i) {
            if (!in[i].p) continue;
            d.in[i] = (char *)ctx->stage[0].p + at[i];
            if (in[i].bytes) HIP_TRY(hipMemcpyAsync(d.in[i], in[i].p, in[i].bytes, hipMemcpyHostToDevice, s));
        }
        if ((rc = body(d))) return rc;
        HIP_TRY(hipMemcpyAsync(out, d.out, out_bytes, hipMemcpyDeviceToHost, s));
        if (out2) HIP_TRY(hipMemcpyAsync(out2, d.out2, out2_bytes, hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}
template <class Body>
int bn_staged(bn254_ctx *ctx, BnStageIn in0, BnStageIn in1, void *out, size_t out_bytes, void *out2, size_t out2_bytes, Body body, BnStageIn in2 = {nullptr, 0}) {
    const BnStageIn in[3] = {in0, in1, in2};
    return bn_staged_n(ctx, in, 3, out, out_bytes, out2, out2_bytes, body);
}

extern "C" {
// bn254_kernels_b.hip
int bn254_launch_miller_B(const void *p, const void *q, void *f, size_t n, int naf, hipStream_t s);
size_t bn254_miller_shared_state_bytes_B(size_t n, int m);
int bn254_launch_miller_shared_B(const void *p, const void *q, void *f, size_t n, int m, void *state, hipStream_t s);
int bn254_launch_final_exp_B(const void *f, void *out, size_t n, void *table, hipStream_t s);
size_t bn254_final_exp_table_bytes_B(size_t n);
int bn254_launch_g2_precompute_B(const void *q, void *coeffs, size_t n, hipStream_t s);
int bn254_launch_miller_prepared_B(const void *p, const void *coeffs, int shared, void *f, size_t n, hipStream_t s);
size_t bn254_native_table_bytes_B(size_t nq);
int bn254_native_lines_B(void);
int bn254_launch_g2_prepare_native_B(const void *q, void *table, void *q_inf, size_t nq, hipStream_t s);
int bn254_launch_miller_native_B(const void *p, const void *table, const void *q_inf, size_t nq, size_t q_lo, int shared, void *f, size_t n, hipStream_t s);
int bn254_launch_miller_native_shared_B(const void *p, const void *table, const void *q_inf, size_t nq, size_t q_lo, int shared, void *f, size_t n, int m, hipStream_t s);
int bn254_launch_miller_native_seg_B(const void *p, const void *table, const void *q_inf, size_t nq, const void *q_index, size_t q_lo, int shared, const void *pieces, size_t count, void *f, hipStream_t s);
int bn254_launch_gt_mul_B(const void *a, const void *b, void *out, size_t n, hipStream_t s);
int bn254_launch_gt_fold_seg_B(const void *pieces, size_t count, hipStream_t s);
size_t bn254_gt_pow_table_bytes_B(size_t n);
int bn254_launch_gt_pow_B(const void *a, const void *k, void *out, size_t n, void *table, int mode, hipStream_t s);
int bn254_launch_gt_inverse_B(const void *a, void *out, size_t n, hipStream_t s);
int bn254_launch_exp_by_neg_z_B(const void *a, void *out, size_t n, hipStream_t s);
// bn254_kernels_w.hip: one Fq12 per wave (wave.hpp)
int bn254_launch_wave_ubench_W(int which, int iters, void *out, hipStream_t s);
int bn254_launch_final_exp_W(const void *f, void *out, size_t n, hipStream_t s);
int bn254_launch_pairing_W(const void *p, const void *q, void *out, size_t n, int final_exp, hipStream_t s);
int bn254_launch_gt_tail_W(const void *in, size_t groups, unsigned m, void *out, int final_exp, hipStream_t s);
int bn254_launch_gt_tail_seg_W(const void *pieces, size_t count, hipStream_t s);
void bn254_gt_reduce_sizes_W(size_t n, unsigned chunk, unsigned per_wave, size_t *grid, size_t *scratch_bytes, size_t *counter_words);
int bn254_launch_gt_reduce_W(const void *in, size_t n, unsigned chunk, unsigned per_wave, unsigned bfly, void *scratch, void *counters, void *out, hipStream_t s);
// bn254_kernels_q.hip: one pairing per quad of lanes (quad.hpp)
int bn254_launch_miller_Q(const void *p, const void *q, void *f, size_t n, hipStream_t s);
size_t bn254_final_exp_table_bytes_Q(size_t n);
int bn254_launch_final_exp_Q(const void *f, void *out, size_t n, void *table, hipStream_t s);
// bn254_kernels_mul.hip
size_t bn254_mul_table_bytes_M(int g, size_t n);
int bn254_launch_g1_mul_M(const void *p, const void *k, void *out, size_t n, int normalize, void *table, hipStream_t s);
int bn254_launch_g2_mul_M(const void *p, const void *k, void *out, size_t n, int normalize, void *table, hipStream_t s);
int bn254_launch_g1_add_M(const void *a, const void *b, void *out, size_t n, int negate_b, hipStream_t s);
int bn254_launch_g2_add_M(const void *a, const void *b, void *out, size_t n, int negate_b, hipStream_t s);
int bn254_launch_msm_mul_M(int g, const void *p, const void *k, void *out, size_t n, void *table, hipStream_t s);
int bn254_launch_msm_fold_M(int g, const void *pieces, size_t count, hipStream_t s);
int bn254_launch_msm_digits_M(const void *k, size_t n, unsigned c, unsigned W, void *counts, void *idx, void *keys, int scatter, hipStream_t s);
int bn254_launch_msm_scan_M(void *counts, size_t total, void *tiles, void *n0, hipStream_t s);
unsigned bn254_msm_piece_M(void);
int bn254_launch_msm_bucket_M(int g, const void *pts, const void *idx, const void *keys, const void *n0, unsigned level, void *out_pts, void *out_keys, void *buckets,
                              size_t lanes, hipStream_t s);
int bn254_launch_msm_reduce_M(int g, const void *buckets, unsigned G, unsigned groups, unsigned c, size_t count, void *terms, hipStream_t s);
int bn254_launch_msmp_digits_M(const void *k, size_t n, unsigned c, unsigned W, size_t count, size_t first, void *counts, void *idx, void *keys, int scatter, hipStream_t s);
int bn254_launch_msmp_bucket_M(int g, const void *table, const void *idx, const void *keys, const void *n0, void *out_pts, void *out_keys, void *buckets, size_t lanes, hipStream_t s);
int bn254_launch_msmp_double_M(int g, void *d_pts, unsigned c, size_t n, hipStream_t s);
size_t bn254_msmp_entry_bytes_M(int g);
size_t bn254_mul_base_table_bytes_M(int g, unsigned c);
int bn254_launch_mul_base_M(int g, const void *table, unsigned c, const void *k, void *out, size_t n, hipStream_t s);
int bn254_launch_mul_base_tile_M(int g, const void *d_base, void *d_out, size_t n, hipStream_t s);
int bn254_launch_mul_base_repack_M(int g, const void *d_pts, void *table, size_t n, hipStream_t s);
unsigned bn254_normalize_run_M(void);
size_t bn254_normalize_prefix_bytes_M(int g, size_t n);
int bn254_launch_normalize_M(int g, const void *d_p, void *d_out, size_t n, void *prefix, hipStream_t s);
int bn254_launch_eq_M(int g, const void *d_a, const void *d_b, void *d_out, size_t n, hipStream_t s);
int bn254_launch_group_ntt_stage_M(int g, const void *d_src, void *d_dst, const void *wtbl, unsigned log_n, unsigned stage, int inverse, size_t lo, size_t n, void *table, hipStream_t s);
int bn254_launch_group_ntt_scale_M(int g, const void *d_src, void *d_dst, const void *stbl, unsigned log_n, const uint64_t *scale, size_t lo, size_t n, void *table, hipStream_t s);
// bn254_measure.hip
int bn254_launch_gather_K(const void *d_records, size_t records, size_t record_bytes, const void *d_index, size_t n, void *d_out, hipStream_t s);
}
