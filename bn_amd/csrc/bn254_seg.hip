// Segmented operations of the BN254 engine (include/bn254_hip.h): the batched multi-pairings bn254_pairing_product_batch*, the segmented
// multi-scalar multiplications bn254_g{1,2}_msm_batch* and the one large sum bn254_g{1,2}_msm* with its bucket route; the fixed-base scalar multiplication bn254_g{1,2}_mul_base_batch* with its
// table cache; the batched normalisation bn254_g{1,2}_normalize_batch* and comparison bn254_g{1,2}_eq_batch*.  Host code only: the
// plans are host_plan.hpp's, the kernels live in bn254_kernels_{b,w,mul}.hip.  Compiled like every unit (bn254_hip.hip: the flags).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "host_ctx.hpp"
#include "lane_launch.hpp"      // BN_LAUNCH_MAX and the overrides; this unit launches through bn254_kernels_{b,w,mul}.hip

// ---- one executor for a segmented plan
// The values (Fq12 / Jacobian points, V bytes each) are cut into chunks of at most `chunk`; a segment that crosses a cut carries its partial
// result into value slot 0 of the next chunk, in front of that chunk's values.  Per chunk: produce(chunk index, chunk, slot 1, extra) writes
// the values, then the levels of the segmented fold - every piece folds at most `fold` consecutive values; a segment with more values is cut into
// pieces whose partial results the next level folds, so no lane runs a chain longer than fold - 1 operations and a segment of L values takes
// ceil(log_fold L) levels - or, `small`, the ragged tail, then the carry copy.  The host builds every level's work list up front.
// The work lists: ONE copy per call (bn_plan_upload: the caller's `offsets` may be freed as soon as the call returns); cut(chunks) may name
// Miller pieces to place behind the fold's pieces in the same copy (bn254_pairing_product_batch_prepared_native; `extra`: where they are on
// the device) or return NULL.
namespace {
struct BnSegSpec { size_t V, fold, chunk; bool snap, small; };
int bn_seg_upload(bn254_ctx *c, const std::vector<BnSegPiece> &pieces, hipStream_t s, const std::vector<BnMillerPiece> *miller) {
    return bn_plan_upload(c, pieces.data(), pieces.size() * sizeof(BnSegPiece), miller ? miller->data() : nullptr, miller ? miller->size() * sizeof(BnMillerPiece) : 0, s);
}
// fold(tail, pieces, count) enqueues one launch over `count` pieces of the device-side work list; off is HOST memory; scratch guard held by the caller
template <class Cut, class Produce, class Fold>
int bn_seg_run(bn254_ctx *c, const BnSegSpec &sp, const size_t *off, size_t m, void *d_out, hipStream_t s, Cut cut, Produce produce, Fold fold) {
    int rc = c->ws.reserve(seg_ws_values(sp.chunk, sp.fold) * sp.V); if (rc) return rc;
    char *const ws = (char *)c->ws.p;
    std::vector<BnSegPiece> pieces;
    std::vector<SegChunk> chunks;
    if (!seg_plan(off, m, sp.chunk, sp.small, ws, (char *)d_out, pieces, chunks, sp.V, sp.fold, sp.snap)) return BN254_E_INTERNAL;
    if ((rc = bn_seg_upload(c, pieces, s, cut(chunks)))) return rc;
    const BnSegPiece *list = (const BnSegPiece *)c->seg_plan.p;
    const void *extra = list + pieces.size();
    const size_t carry_slot = sp.chunk + 1 + seg_partials_max(sp.chunk, sp.fold);
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const SegChunk &ch = chunks[ci];
        if ((rc = produce(ci, ch, ws + sp.V, extra))) return rc;
        for (const SegLaunch &l : ch.launches) {
            if (l.tail) rc = fold(true, list + l.first, l.count);
            else rc = bn_for_parts(l.count, BN_LAUNCH_MAX, [&](size_t lo, size_t cnt) { return fold(false, list + l.first + lo, cnt); });
            if (rc) return rc;
        }
        if (ch.carry_out)                 // the segment that goes on: its partial result becomes value slot 0 of the next chunk
            HIP_TRY(hipMemcpyAsync(ws, ws + carry_slot * sp.V, sp.V, hipMemcpyDeviceToDevice, s));
    }
    return BN254_OK;
}
const auto bn_no_cut = [](const std::vector<SegChunk> &) -> const std::vector<BnMillerPiece> * { return nullptr; };
// the fold of Fq12 values: lane pairs (bn254_gt_mul_B<true>) or, in the ragged tail, one wave per piece, product and exponentiation (bn254_gt_tail_W<true>)
auto bn_gt_fold(bn254_ctx *c, hipStream_t s) {
    return [c, s](bool tail, const BnSegPiece *list, size_t cnt) -> int {
        BnScope sc(c, s, tail ? "gt_tail_seg" : "gt_segment");
        return tail ? bn254_launch_gt_tail_seg_W(list, cnt, s) : bn254_launch_gt_fold_seg_B(list, cnt, s);
    };
}
}  // namespace

// ---- batched multi-pairing: m independent products over CSR segments (bn254_pairing_product_batch*)
// The pairs are cut into chunks of at most one machine round (bn_round_pairs), at the last segment boundary inside the round when there
// is one.  Per chunk: the Miller values (bn_launch_miller, NAF: they only meet a final exponentiation), then the fold in pieces of BN_SEG_FOLD.
// Small route: one chunk whose Miller values come from the one-per-wave kernel and at most BN254_OPT_WAVE_FE_MAX segments - the last
// piece of every segment (at most BN_TAIL_SEG_MAX values; longer segments are first folded down to that) is multiplied AND exponentiated by
// one wave: a verifier's handful of 4-pair checks is two launches.  Otherwise the last fold level writes every
// segment's un-exponentiated product to out[j] and bn_launch_final_exp exponentiates the m values in place.
// out[j] = final_exponentiation(prod of the Miller values of pairs [off[j], off[j+1])) for j < m; off is HOST memory; scratch guard held by the caller
static int bn_launch_product_batch(bn254_ctx *c, const void *d_p, const void *d_q, const size_t *off, size_t m, void *d_out, hipStream_t s) {
    const size_t n = off[m];
    if (bn_seg_all_ones(off, m)) return bn_launch_pairing(c, d_p, d_q, d_out, n, s, nullptr);           // every segment one pair: bn254_pairing_batch's kernels
    const size_t chunk_pairs = bn_round_pairs(c);
    const bool small = n <= chunk_pairs && n <= bn_wave_pairing_max(c) && m <= bn_wave_fe_max(c);
    int rc = bn_seg_run(c, {sizeof(bn_gt), BN_SEG_FOLD, chunk_pairs, true, small}, off, m, d_out, s, bn_no_cut, [&](size_t, const SegChunk &ch, char *values, const void *) -> int {
        if (ch.hi == ch.lo) return BN254_OK;
        return bn_launch_miller(c, (const char *)d_p + ch.lo * sizeof(bn_g1), (const char *)d_q + ch.lo * sizeof(bn_g2), values, ch.hi - ch.lo, s, true);
    }, bn_gt_fold(c, s));
    if (rc) return rc;
    return small ? BN254_OK : bn_launch_final_exp(c, d_out, d_out, m, s, nullptr);
}

// ---- batched multi-pairing over prepared points with per-pair indices (bn254_pairing_product_batch_prepared_native*)
// Every segment of L pairs is cut into ceil(L / 4) PIECES of at most four consecutive pairs; a lane pair runs one piece on ONE Miller accumulator
// over the native tables (bn254_miller_native_shared4_B<true>: the line products of its pairs, a quarter of the squarings) and writes one
// un-exponentiated Fq12.  Pieces go out in sub-launches of at most one machine round of lane pairs (host_plan.hpp miller_cut).
//   * no segment above four pairs (a block of Groth16 checks): piece j IS segment j (an empty segment is a piece of no pairs, whose four
//     identity columns give exactly one) - the kernel writes out[j], the final exponentiation runs in place, nothing is folded;
//   * otherwise the pieces' values are the values of a segmented Fq12 fold whose segment j holds ceil(L_j / 4) of them: the plan of
//     bn254_pairing_product_batch (chunks of one round of VALUES, carry, levels of BN_SEG_FOLD) over the derived offsets.
// Small calls (n <= bn_prepared_small_max): the general path on the points kept with the handle, gathered by
// index into the workspace (q_index == NULL: used in place), like the other prepared entry points.
// d_qi: 64-bit indices in device memory or NULL; off is HOST memory; scratch guard held by the caller.
static_assert(sizeof(size_t) == sizeof(uint64_t), "q_index travels to the device as 64-bit words");
static int bn_launch_product_batch_prepared(bn254_ctx *c, const void *d_p, const bn254_g2_prepared *h, const void *d_qi, const size_t *off, size_t m, void *d_out, hipStream_t s) {
    const size_t n = off[m], chunk_pairs = bn_round_pairs(c);
    const int shared = h->nq == 1;
    int rc;
    if (n <= bn_prepared_small_max(c, h)) {
        const void *q = h->q;
        if (d_qi && n) {
            const size_t q_at = seg_ws_values(chunk_pairs) * sizeof(bn_gt);          // behind everything bn_launch_product_batch keeps in the workspace
            if ((rc = c->ws.reserve(q_at + n * sizeof(bn_g2)))) return rc;
            BnScope sc(c, s, "g2_gather");
            if ((rc = bn254_launch_gather_K(h->q, shared ? h->small_max : h->nq, sizeof(bn_g2), d_qi, n, (char *)c->ws.p + q_at, s))) return rc;
            q = (const char *)c->ws.p + q_at;
        }
        return bn_launch_product_batch(c, d_p, q, off, m, d_out, s);
    }
    const bool direct = bn_seg_longest(off, m) <= 4;
    MillerCut mc;
    auto cut = [&](const std::vector<SegChunk> &chunks) {
        mc = miller_cut(off, m, direct, chunks, [&](size_t count) { return bn_sub_launch(c, count); });
        return &mc.pieces;
    };
    // the sub-launches of chunk `ci` (its pieces start at `chunk_lo`) over the uploaded pieces `mlist`: piece k of the chunk writes values[k]
    auto miller = [&](size_t ci, size_t chunk_lo, char *values, const void *mlist) -> int {
        for (size_t i = mc.chunk_subs[ci]; i < mc.chunk_subs[ci + 1]; ++i) {
            const MillerSub &u = mc.subs[i];
            BnScope sc(c, s, "miller_native_seg");
            rc = bn254_launch_miller_native_seg_B((const char *)d_p + u.base * sizeof(bn_g1), h->table, h->inf, h->nq, d_qi && n ? (const char *)d_qi + u.base * sizeof(uint64_t) : nullptr,
                                                  shared ? 0 : u.base, shared, (const BnMillerPiece *)mlist + u.lo, u.cnt, values + (u.lo - chunk_lo) * sizeof(bn_gt), s);
            if (rc) return rc;
        }
        return BN254_OK;
    };
    if (direct) {
        if ((rc = bn_seg_upload(c, {}, s, cut({{0, m, false, {}}}))) || (rc = miller(0, 0, (char *)d_out, c->seg_plan.p))) return rc;
    } else {
        const std::vector<size_t> voff = miller_value_offsets(off, m);
        rc = bn_seg_run(c, {sizeof(bn_gt), BN_SEG_FOLD, chunk_pairs, true, false}, voff.data(), m, d_out, s, cut,
                        [&](size_t ci, const SegChunk &ch, char *values, const void *mlist) { return miller(ci, ch.lo, values, mlist); }, bn_gt_fold(c, s));
        if (rc) return rc;
    }
    return bn_launch_final_exp(c, d_out, d_out, m, s, nullptr);
}

// ---- segmented multi-scalar multiplication: out[j] = normalize(sum of p[i] * k[i] over i in [off[j], off[j+1])) (bn254_g{1,2}_msm_batch*)
// The plan of the batched multi-pairing with points for Fq12 values.  Terms are cut into chunks of at most one sub-launch of the
// multiplication kernels (BN_MUL_LANES_PER_LAUNCH lanes: 2^20 G1 / 2^19 G2 terms, every launch but the last one full, like bn_mul_dev); a
// segment that crosses a cut carries its partial sum - Jacobian - into value slot 0 of the next chunk.  Per chunk: the term kernel
// (bn254_g{1,2}_mul_M<true>: the GLV / GLS chain, NO normalisation) writes Jacobian points to the workspace, then the levels of the segmented
// fold (bn254_g{1,2}_add_M<true>): every lane (G2: lane pair) adds one piece of at most BN_MSM_FOLD consecutive values with the complete
// addition, ceil(log_BN_MSM_FOLD L) levels for a segment of L terms, and the piece that completes a segment normalises: one inversion per
// segment instead of one per term.
// BN_MSM_FOLD = 4, from the sweep over 4 / 8 / 16 / 32 in profiles/r08_msm.txt (tools/time_msm.py --sweep): a narrow piece keeps more lanes
// busy and its serial chain short, a wide one saves levels (launches and a round trip of the partial sums through memory) - the fold of
// 16 x 3001 terms takes 0.27 / 0.37 / 0.49 / 0.74 ms, of 2^14 x 16 terms 0.17 / 0.16 / 0.22 / 0.23 ms.  (seg_partials_max needs >= 4.)
constexpr size_t BN_MSM_FOLD = 4;
static_assert(BN_MSM_FOLD >= 4, "seg_partials_max bounds the partial sums for fold widths from 4");
// off is HOST memory; scratch guard held by the caller
static int bn_launch_msm(bn254_ctx *c, int g, const void *d_p, const void *d_k, const size_t *off, size_t m, void *d_out, hipStream_t s) {
    const size_t n = off[m], V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    if (bn_seg_all_ones(off, m)) return bn_mul_dev(c, g, d_p, d_k, d_out, n, s, 1);         // every segment one term: bn254_g{1,2}_mul_batch's launches
    const size_t step = BN_MUL_LANES_PER_LAUNCH / (g == 1 ? 1 : 2), chunk = std::max<size_t>(1, std::min(n, step));
    int rc = c->mul_tbl.reserve(bn254_mul_table_bytes_M(g, chunk)); if (rc) return rc;
    return bn_seg_run(c, {V, BN_MSM_FOLD, chunk, false, false}, off, m, d_out, s, bn_no_cut, [&](size_t, const SegChunk &ch, char *values, const void *) -> int {
        if (ch.hi == ch.lo) return BN254_OK;
        BnScope sc(c, s, g == 1 ? "g1_msm_mul" : "g2_msm_mul");
        return bn254_launch_msm_mul_M(g, (const char *)d_p + ch.lo * V, (const char *)d_k + ch.lo * sizeof(bn_fr), values, ch.hi - ch.lo, c->mul_tbl.p, s);
    }, [&](bool, const BnSegPiece *list, size_t cnt) -> int {
        BnScope sc(c, s, g == 1 ? "g1_msm_fold" : "g2_msm_fold");
        return bn254_launch_msm_fold_M(g, list, cnt, s);
    });
}

// ---- one large multi-scalar multiplication: out = normalize(sum of p[i] * k[i] over all n terms) (bn254_g{1,2}_msm*)
// Below BN254_OPT_MSM_BUCKET_MIN terms: bn_launch_msm on the one segment {0, n}.  From there on the bucket (Pippenger) method with unsigned
// c-bit windows (BN254_OPT_MSM_WINDOW_BITS; W = ceil(254 / c) windows, 2^c buckets per window of which bucket 0 stays empty), in chunks of at
// most BN254_OPT_MSM_CHUNK terms.  Per chunk (kernels and their invariants: bn254_kernels_mul.hip):
//   digits   count the terms per (window, digit), scan the W * 2^c counts, scatter (term index, key) into key order     scope g*_msm_digits
//   bucket   levels of the accumulation: every lane adds at most MSM_PIECE consecutive entries; a run of one key that ends inside a lane is
//            added to its bucket, the pieces of a longer run go to the next, eight times shorter level.  The entry count is known on the
//            device only; the host launches every level for its upper bound W * terms (lanes past the real count retire at once), so
//            nothing is read back and the call stays asynchronous                                                          scope g*_msm_bucket
// The buckets collect over the chunks.  Then ONE reduction (scope g*_msm_reduce): groups of 16 consecutive buckets give S = sum B_b and
// T = sum (b - base) B_b, and the window sums sum_groups (T + base S) weighted by 2^(c w) are the one-segment bn_launch_msm over these
// 2 * W * 2^c / 16 Jacobian terms with the scalars base * 2^(c w) and 2^(c w) - host-known, built once per window width - which folds,
// normalises once and writes out.
// Workspace (context-owned, under the scratch guard; host_plan.hpp msm_bucket_plan), for t = min(n, chunk) terms and V = 96 / 192 bytes per
// point: W t entries of 8 bytes (index, key), W 2^c counts of 4 bytes and buckets of V bytes, the partial sums of the levels (at most
// W t / 7 + 64 slots of V + 4 bytes), 2 W 2^c / 16 tail terms of V + 32 bytes.
// scratch guard held by the caller
static int bn_launch_msm_bucket(bn254_ctx *c, int g, const void *d_p, const void *d_k, size_t n, void *d_out, hipStream_t s) {
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2), L = bn254_msm_piece_M();
    const unsigned cb = bn_msm_window_bits(bn_opt(c, BN254_OPT_MSM_WINDOW_BITS), n);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(n, (size_t)bn_opt(c, BN254_OPT_MSM_CHUNK)));
    const MsmBucketPlan bp = msm_bucket_plan(cb, chunk, V, L);
    int rc;
    if ((rc = c->msm_ws.reserve(bp.bytes))) return rc;
    char *ws = (char *)c->msm_ws.p;
    if (c->msm_scal_c != (long)cb) {
        std::vector<uint64_t> &h = c->msm_scal_host;
        HIP_TRY(hipStreamSynchronize(s));                    // the previous image may still be on its way
        msm_tail_scalars(cb, h);
        if ((rc = c->msm_scal.reserve(h.size() * 8))) return rc;
        c->msm_scal_c = -1;
        HIP_TRY(hipMemcpyAsync(c->msm_scal.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        c->msm_scal_c = (long)cb;
    }
    HIP_TRY(hipMemsetAsync(ws + bp.o_buckets, 0, bp.K * V, s));   // z = 0: every bucket starts as the point at infinity
    rc = bn_for_parts(n, chunk, [&](size_t lo, size_t len) -> int {
        const char *pk = (const char *)d_k + lo * sizeof(bn_fr), *pp = (const char *)d_p + lo * V;
        {
            BnScope sc(c, s, g == 1 ? "g1_msm_digits" : "g2_msm_digits");
            HIP_TRY(hipMemsetAsync(ws + bp.o_counts, 0, bp.K * 4, s));
            if ((rc = bn254_launch_msm_digits_M(pk, len, cb, bp.W, ws + bp.o_counts, nullptr, nullptr, 0, s))) return rc;
            if ((rc = bn254_launch_msm_scan_M(ws + bp.o_counts, bp.K, ws + bp.o_tiles, ws + bp.o_n0, s))) return rc;
            if ((rc = bn254_launch_msm_digits_M(pk, len, cb, bp.W, ws + bp.o_counts, ws + bp.o_idx, ws + bp.o_keys, 1, s))) return rc;
        }
        BnScope sc(c, s, g == 1 ? "g1_msm_bucket" : "g2_msm_bucket");
        const char *pts = pp, *idx = ws + bp.o_idx, *keys = ws + bp.o_keys;
        size_t N = (size_t)bp.W * len;
        for (unsigned level = 0;; ++level) {
            if (level >= bp.o_level.size()) return BN254_E_INTERNAL;
            char *opts = ws + bp.o_level[level].first, *okeys = ws + bp.o_level[level].second;
            if ((rc = bn254_launch_msm_bucket_M(g, pts, idx, keys, ws + bp.o_n0, level, opts, okeys, ws + bp.o_buckets, (N + L - 1) / L, s))) return rc;
            if (N <= L) return BN254_OK;
            N = 2 * ((N + L - 1) / L); pts = opts; idx = nullptr; keys = okeys;
        }
    });
    if (rc) return rc;
    {
        BnScope sc(c, s, g == 1 ? "g1_msm_reduce" : "g2_msm_reduce");
        if ((rc = bn254_launch_msm_reduce_M(g, ws + bp.o_buckets, bp.G, bp.groups, cb, bp.count, ws + bp.o_terms, s))) return rc;
    }
    const size_t off[2] = {0, 2 * bp.count};
    return bn_launch_msm(c, g, ws + bp.o_terms, c->msm_scal.p, off, 1, d_out, s);
}
// the route of one call: the one-segment launch sequence of bn254_g{1,2}_msm_batch below BN254_OPT_MSM_BUCKET_MIN terms
static bool bn_msm_bucket_route(const bn254_ctx *c, int g, size_t n) {
    const long set = c->opt[BN254_OPT_MSM_BUCKET_MIN].load(std::memory_order_relaxed);
    return n >= (size_t)(set >= 0 ? set : g == 1 ? BN_MSM_BUCKET_MIN_DEFAULT : BN_MSM_BUCKET_MIN_DEFAULT_G2);
}

// ---- fixed-base scalar multiplication: out[i] = normalize(base * k[i]) with ONE base for the whole call (bn254_g{1,2}_mul_base_batch*)
// Everything bn254_g{1,2}_mul_batch redoes per scalar - GLV / GLS split, window table, ~128 doublings - depends on the base alone.  Here
// a table of the affine points d * 2^(c w) * base (W = ceil(254 / c) windows, d = 1 .. 2^(c-1); kernels and layout: bn254_kernels_mul.hip
// BaseMulArgs) turns a multiplication into at most W mixed additions and the normalisation (scope g*_mul_base; sub-launches of at most
// BN_LAUNCH_MAX scalars).
// The tables live in the context: BN_BASE_SLOTS per group, least recently used first out, keyed by the caller's bytes of the base (another
// Jacobian representation of the same point is another key - and gives the same table, the entries are normalised).  EVERY miss builds
// (scope g*_base_table): the base goes to the device through pinned staging, is tiled, multiplied by the host-known scalars d * 2^(c w) with
// the shipped normalising kernel bn254_g{1,2}_mul_M and repacked into device limbs; a base at infinity gives a table of flagged entries
// and every result (0, 1, 0).  Lookup, build and launches run under the caller's scratch guard, which is what orders a rebuild on one
// stream behind the readers on another.
namespace {
BnOverride<unsigned> g_base_window[2];        // measurement only (bn254_mul_base_set_window): the window width
unsigned bn_base_window(int g) { return g_base_window[g - 1].get(g == 1 ? BN_BASE_WINDOW_G1 : BN_BASE_WINDOW_G2); }
// the scalars of a table build on the device, rebuilt only when the window width changes (as msm_scal)
int bn_base_scalars(BnBaseCache &bc, unsigned cb, hipStream_t s) {
    if (bc.scal_c == (long)cb) return BN254_OK;
    int rc;
    HIP_TRY(hipStreamSynchronize(s));                        // the previous image may still be on its way
    base_table_scalars(cb, bc.scal_host);
    if ((rc = bc.scal.reserve(bc.scal_host.size() * 8))) return rc;
    bc.scal_c = -1;
    HIP_TRY(hipMemcpyAsync(bc.scal.p, bc.scal_host.data(), bc.scal_host.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    bc.scal_c = (long)cb;
    return BN254_OK;
}
// the slot that holds the table of `base` (HOST memory, read here), built on `s` if no slot has it; scratch guard held by the caller
int bn_base_table(bn254_ctx *c, int g, const void *base, hipStream_t s, BnBaseSlot **out) {
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    const unsigned cb = bn_base_window(g);
    BnBaseCache &bc = c->base_cache[g - 1];
    ++bc.tick;
    BnBaseSlot *victim = nullptr;
    for (BnBaseSlot &sl : bc.slot) {
        if (sl.valid && sl.c == cb && !memcmp(sl.key, base, V)) { sl.used = bc.tick; *out = &sl; return BN254_OK; }
        if (!victim || (victim->valid && (!sl.valid || sl.used < victim->used))) victim = &sl;
    }
    victim->valid = false;
    int rc;
    const size_t E = bn_base_entries(cb);
    if ((rc = bn_base_scalars(bc, cb, s))) return rc;
    if (c->base_stage_ev) HIP_TRY(hipEventSynchronize(c->base_stage_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->base_stage_ev, hipEventDisableTiming));
    if ((rc = c->base_stage_host.reserve(sizeof(bn_g2))) || (rc = c->base_stage.reserve(sizeof(bn_g2)))) return rc;
    if ((rc = c->ws.reserve(2 * E * V)) || (rc = c->mul_tbl.reserve(bn254_mul_table_bytes_M(g, E)))) return rc;
    if ((rc = victim->table.reserve(bn254_mul_base_table_bytes_M(g, cb)))) return rc;
    memcpy(c->base_stage_host.p, base, V);
    HIP_TRY(hipMemcpyAsync(c->base_stage.p, c->base_stage_host.p, V, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->base_stage_ev, s));
    char *tiled = (char *)c->ws.p, *pts = tiled + E * V;
    {
        BnScope sc(c, s, g == 1 ? "g1_base_table" : "g2_base_table");
        if ((rc = bn254_launch_mul_base_tile_M(g, c->base_stage.p, tiled, E, s))) return rc;
        if ((rc = g == 1 ? bn254_launch_g1_mul_M(tiled, bc.scal.p, pts, E, 1, c->mul_tbl.p, s) : bn254_launch_g2_mul_M(tiled, bc.scal.p, pts, E, 1, c->mul_tbl.p, s))) return rc;
        if ((rc = bn254_launch_mul_base_repack_M(g, pts, victim->table.p, E, s))) return rc;
    }
    memcpy(victim->key, base, V);
    victim->c = cb; victim->used = bc.tick; victim->valid = true;
    *out = victim;
    return BN254_OK;
}
// base is HOST memory; scratch guard held by the caller
int bn_launch_mul_base(bn254_ctx *c, int g, const void *base, const void *d_k, void *d_out, size_t n, hipStream_t s) {
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    BnBaseSlot *sl = nullptr;
    int rc = bn_base_table(c, g, base, s, &sl); if (rc) return rc;
    return bn_for_parts(n, BN_LAUNCH_MAX, [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, g == 1 ? "g1_mul_base" : "g2_mul_base");
        return bn254_launch_mul_base_M(g, sl->table.p, sl->c, (const char *)d_k + lo * sizeof(bn_fr), (char *)d_out + lo * V, cnt, s);
    });
}

// ---- batched normalisation and projective equality (bn254_g{1,2}_normalize_batch*, bn254_g{1,2}_eq_batch*)
// normalize: sub-launches of at most BN_LAUNCH_MAX points (a multiple of every run length), every lane (G2: lane pair) a run of
// bn254_normalize_run_M() consecutive points with one inversion (group_ops.hpp normalize_body); the last run of a sub-launch is the short
// one.  The prefix products of a sub-launch - one field element per point - are context-owned scratch, reused by the next sub-launch on the
// same stream.  eq: one lane (lane pair) per pair of points, no scratch.
BnLaunchMax g_norm_launch_max;                // tests only (bn254_normalize_set_launch_max): the sub-launch size
// scratch guard held by the caller
int bn_launch_normalize(bn254_ctx *c, int g, const void *d_p, void *d_out, size_t n, hipStream_t s) {
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2), step = g_norm_launch_max.step();
    int rc = c->norm_prefix.reserve(bn254_normalize_prefix_bytes_M(g, std::min(n, step))); if (rc) return rc;
    return bn_for_parts(n, step, [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, g == 1 ? "g1_normalize" : "g2_normalize");
        return bn254_launch_normalize_M(g, (const char *)d_p + lo * V, (char *)d_out + lo * V, cnt, c->norm_prefix.p, s);
    });
}
int bn_launch_eq(bn254_ctx *c, int g, const void *d_a, const void *d_b, void *d_out, size_t n, hipStream_t s) {
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    return bn_for_parts(n, BN_LAUNCH_MAX, [&](size_t lo, size_t cnt) -> int {
        BnScope sc(c, s, g == 1 ? "g1_eq" : "g2_eq");
        return bn254_launch_eq_M(g, (const char *)d_a + lo * V, (const char *)d_b + lo * V, (char *)d_out + lo * sizeof(int32_t), cnt, s);
    });
}
}  // namespace

// ---- multi-scalar multiplication against prepared bases (bn254_g{1,2}_msm_prepare*, bn254_g{1,2}_msm_prepared*)
// Everything bn254_g{1,2}_msm redoes per call that depends on the points alone is in the handle: the affine multiples 2^(c w) P_i
// (group_ops.hpp: records, layout, bodies).
// The build (scope g*_msmp_table), window by window over scratch of two count-sized arrays in the context's workspace: a running Jacobian
// copy of the points is normalised (bn_launch_normalize: one inversion per NORM_RUN points) into the second array, whose points are repacked
// into the window's records (window 0: and kept as the handle's points); the running copy is then doubled c times in place.  The entries
// are normalised, so the table does not depend on how it was built.
// scratch guard held by the caller
static int bn_msmp_build(bn254_ctx *c, bn254_msm_prepared *h, const void *d_p, hipStream_t s) {
    const int g = h->group;
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2), n = h->count, E = bn254_msmp_entry_bytes_M(g);
    if (n == 0) return BN254_OK;
    int rc = c->ws.reserve(2 * n * V); if (rc) return rc;
    char *run = (char *)c->ws.p, *norm = run + n * V;
    HIP_TRY(hipMemcpyAsync(run, d_p, n * V, hipMemcpyDeviceToDevice, s));
    for (unsigned w = 0; w < h->W; ++w) {
        if ((rc = bn_launch_normalize(c, g, run, norm, n, s))) return rc;
        BnScope sc(c, s, g == 1 ? "g1_msmp_table" : "g2_msmp_table");
        if (w == 0) HIP_TRY(hipMemcpyAsync(h->pts, norm, n * V, hipMemcpyDeviceToDevice, s));
        rc = bn_for_parts(n, BN_LAUNCH_MAX / 2, [&](size_t lo, size_t cnt) -> int {
            if (int e = bn254_launch_mul_base_repack_M(g, norm + lo * V, (char *)h->table + ((size_t)w * n + lo) * E, cnt, s)) return e;
            return w + 1 < h->W ? bn254_launch_msmp_double_M(g, run + lo * V, h->c, cnt, s) : BN254_OK;
        });
        if (rc) return rc;
    }
    return BN254_OK;
}
static void bn_msmp_free(bn254_msm_prepared *h) {
    if (h->table) hipFree(h->table);
    if (h->pts) hipFree(h->pts);
    delete h;
}
// d_p: device memory; the checks that need no device are the caller's
static int bn_msmp_prepare_dev(bn254_ctx *ctx, int g, const void *d_p, size_t n, int window_bits, void **out, void *stream) {
    *out = nullptr;
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) -> int {
        bn254_msm_prepared *h = new (std::nothrow) bn254_msm_prepared();
        if (!h) return BN254_E_ALLOC;
        h->device = ctx->device; h->group = g; h->count = n;
        h->c = window_bits ? (unsigned)window_bits : bn_msm_prepared_window_bits(n);
        h->W = bn_msm_prepared_windows(h->c);
        h->table_bytes = (size_t)h->W * n * bn254_msmp_entry_bytes_M(g);
        if (n && (hipMalloc(&h->table, h->table_bytes) != hipSuccess || hipMalloc(&h->pts, n * (g == 1 ? sizeof(bn_g1) : sizeof(bn_g2))) != hipSuccess)) {
            (void)hipGetLastError();
            bn_msmp_free(h);
            return BN254_E_ALLOC;
        }
        if (int rc = bn_msmp_build(ctx, h, d_p, s)) { (void)hipStreamSynchronize(s); bn_msmp_free(h); return rc; }
        *out = h;
        return BN254_OK;
    });
}
// The call from the crossover on, per chunk of at most BN254_OPT_MSM_CHUNK terms (all chunks into the same buckets):
//   digits   count the terms per |digit| (MsmSignedDigitsOp), scan the 2^(c-1) counts, scatter (table index | sign, key)     scope g*_msmp_digits
//   bucket   level 0 from the records (msm_acc_prep_body), levels 1 .. of Jacobian partial sums (msm_acc_body), launched for the
//            upper bound W * terms of the entry count: nothing is read back                                                  scope g*_msmp_bucket
// then ONE reduction over the one window of 2^(c-1) buckets (scope g*_msmp_reduce) and the one-segment bn_launch_msm over its
// 2 * 2^(c-1) / 16 terms with the scalars base + 1 and 1.  Workspace: msm_ws (host_plan.hpp msm_prepared_plan).
// scratch guard held by the caller
static int bn_launch_msmp_bucket(bn254_ctx *c, const bn254_msm_prepared *h, size_t first, const void *d_k, size_t n, void *d_out, hipStream_t s) {
    const int g = h->group;
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2), L = bn254_msm_piece_M();
    const unsigned cb = h->c;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(n, (size_t)bn_opt(c, BN254_OPT_MSM_CHUNK)));
    const MsmBucketPlan bp = msm_prepared_plan(cb, chunk, V, L);
    int rc;
    if ((rc = c->msm_ws.reserve(bp.bytes))) return rc;
    char *ws = (char *)c->msm_ws.p;
    if (c->msmp_scal_c != (long)cb) {
        std::vector<uint64_t> &hs = c->msmp_scal_host;
        HIP_TRY(hipStreamSynchronize(s));                    // the previous image may still be on its way
        msm_prepared_tail_scalars(cb, hs);
        if ((rc = c->msmp_scal.reserve(hs.size() * 8))) return rc;
        c->msmp_scal_c = -1;
        HIP_TRY(hipMemcpyAsync(c->msmp_scal.p, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        c->msmp_scal_c = (long)cb;
    }
    HIP_TRY(hipMemsetAsync(ws + bp.o_buckets, 0, bp.K * V, s));   // z = 0: every bucket starts as the point at infinity
    rc = bn_for_parts(n, chunk, [&](size_t lo, size_t len) -> int {
        const char *pk = (const char *)d_k + lo * sizeof(bn_fr);
        {
            BnScope sc(c, s, g == 1 ? "g1_msmp_digits" : "g2_msmp_digits");
            HIP_TRY(hipMemsetAsync(ws + bp.o_counts, 0, bp.K * 4, s));
            if ((rc = bn254_launch_msmp_digits_M(pk, len, cb, bp.W, h->count, first + lo, ws + bp.o_counts, nullptr, nullptr, 0, s))) return rc;
            if ((rc = bn254_launch_msm_scan_M(ws + bp.o_counts, bp.K, ws + bp.o_tiles, ws + bp.o_n0, s))) return rc;
            if ((rc = bn254_launch_msmp_digits_M(pk, len, cb, bp.W, h->count, first + lo, ws + bp.o_counts, ws + bp.o_idx, ws + bp.o_keys, 1, s))) return rc;
        }
        BnScope sc(c, s, g == 1 ? "g1_msmp_bucket" : "g2_msmp_bucket");
        const char *pts = nullptr, *keys = ws + bp.o_keys;
        size_t N = (size_t)bp.W * len;
        for (unsigned level = 0;; ++level) {
            if (level >= bp.o_level.size()) return BN254_E_INTERNAL;
            char *opts = ws + bp.o_level[level].first, *okeys = ws + bp.o_level[level].second;
            const size_t lanes = (N + L - 1) / L;
            if (level == 0) rc = bn254_launch_msmp_bucket_M(g, h->table, ws + bp.o_idx, keys, ws + bp.o_n0, opts, okeys, ws + bp.o_buckets, lanes, s);
            else rc = bn254_launch_msm_bucket_M(g, pts, nullptr, keys, ws + bp.o_n0, level, opts, okeys, ws + bp.o_buckets, lanes, s);
            if (rc) return rc;
            if (N <= L) return BN254_OK;
            N = 2 * lanes; pts = opts; keys = okeys;
        }
    });
    if (rc) return rc;
    {
        BnScope sc(c, s, g == 1 ? "g1_msmp_reduce" : "g2_msmp_reduce");
        if ((rc = bn254_launch_msm_reduce_M(g, ws + bp.o_buckets, bp.G, bp.groups, cb - 1, bp.count, ws + bp.o_terms, s))) return rc;
    }
    const size_t off[2] = {0, 2 * bp.count};
    return bn_launch_msm(c, g, ws + bp.o_terms, c->msmp_scal.p, off, 1, d_out, s);
}
// the route of one call: below the crossover the one-segment launch sequence of bn254_g{1,2}_msm_batch on the handle's points
static bool bn_msmp_bucket_route(const bn254_ctx *c, int g, size_t n) {
    const long set = c->opt[BN254_OPT_MSM_BUCKET_MIN].load(std::memory_order_relaxed);
    return n >= (size_t)(set >= 0 ? set : g == 1 ? BN_MSMP_BUCKET_MIN_DEFAULT : BN_MSMP_BUCKET_MIN_DEFAULT_G2);
}
static int msmp_dev(bn254_ctx *ctx, int g, const void *prep, size_t first, const void *d_k, size_t n, void *d_out, void *stream) {
    const bn254_msm_prepared *h = (const bn254_msm_prepared *)prep;
    if (int e = bn_msm_prepared_check(h != nullptr, h ? h->group : 0, g, h ? h->count : 0, first, d_k, n, d_out)) return e;      // before any device lookup
    int rc = bn_get_ctx(ctx); if (rc) return rc;
    if (h->device != ctx->device) return BN254_E_BAD_ARG;
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) -> int {
        if (bn_msmp_bucket_route(ctx, g, n)) return bn_launch_msmp_bucket(ctx, h, first, d_k, n, d_out, s);
        const size_t off[2] = {0, n}, V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
        return bn_launch_msm(ctx, g, (const char *)h->pts + first * V, d_k, off, 1, d_out, s);
    });
}
static int msmp_prepare_host(bn254_ctx *ctx, int g, const void *p, size_t n, int window_bits, void **out) {
    if (int e = bn_msm_prepare_check(p, n, window_bits, out)) return e;          // before any device lookup
    *out = nullptr;
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    BnHost h(ctx); if (h.rc) return h.rc;
    BnBuf &dp = ctx->stage[0];
    int rc;
    if ((rc = dp.reserve(n * V))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(dp.p, p, n * V, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = bn_msmp_prepare_dev(ctx, g, dp.p, n, window_bits, out, ctx->stream))) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { bn254_msm_prepared_destroy(*out); *out = nullptr; return (int)e; }
    return BN254_OK;
}
static int msmp_host(bn254_ctx *ctx, int g, const void *prep, size_t first, const bn_fr *k, size_t n, void *out) {
    const bn254_msm_prepared *hp = (const bn254_msm_prepared *)prep;
    if (int e = bn_msm_prepared_check(hp != nullptr, hp ? hp->group : 0, g, hp ? hp->count : 0, first, k, n, out)) return e;     // before any device lookup
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {k, n * sizeof(bn_fr)}, {nullptr, 0}, out, V, nullptr, 0,
                     [&](const BnStaged &d) { return msmp_dev(ctx, g, prep, first, d.in[0], n, d.out, ctx->stream); });
}

// argument checks of bn254_pairing_product_batch_prepared_native* for m > 0 that need no device: the CSR rules, the handle, and - where the
// indices are host memory - every index
// (`indexed`: the pairs carry indices; `q_index`: those indices where the host can read them)
static int bn_prep_seg_check(const void *p, const bn254_g2_prepared *prep, bool indexed, const size_t *q_index, const size_t *offsets, size_t m, const void *out) {
    if (int e = bn_seg_check(p, p, offsets, m, out)) return e;
    if (!prep) return BN254_E_BAD_ARG;
    const size_t n = offsets[m];
    if (!indexed) return prep->nq != 1 && n > prep->nq ? BN254_E_BAD_ARG : BN254_OK;
    for (size_t i = 0; q_index && i < n; ++i)
        if (q_index[i] >= prep->nq) return BN254_E_BAD_ARG;
    return BN254_OK;
}

// the *_dev entry points below run under the scratch guard (bn_dev_entry): workspaces, window tables and work lists are context-owned scratch

extern "C" {

// ---------------------------------------------------------------------------------------------- device-resident API
int bn254_pairing_product_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, const size_t *offsets, size_t m, void *d_out, void *stream) {
    if (m == 0) return BN254_OK;
    if (int e = bn_seg_check(d_p, d_q, offsets, m, d_out)) return e;          // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return bn_launch_product_batch(ctx, d_p, d_q, offsets, m, d_out, s); });
}
int bn254_pairing_product_batch_prepared_native_dev(bn254_ctx *ctx, const void *d_p, const bn254_g2_prepared *prep, const void *d_q_index, const size_t *offsets, size_t m, void *d_out, void *stream) {
    if (m == 0) return BN254_OK;
    if (int e = bn_prep_seg_check(d_p, prep, d_q_index != nullptr, nullptr, offsets, m, d_out)) return e;          // before any device lookup
    int rc = bn_get_ctx(ctx); if (rc) return rc;
    if (prep->device != ctx->device) return BN254_E_BAD_ARG;
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return bn_launch_product_batch_prepared(ctx, d_p, prep, d_q_index, offsets, m, d_out, s); });
}
static int msm_dev(bn254_ctx *ctx, int g, const void *d_p, const void *d_k, const size_t *offsets, size_t m, void *d_out, void *stream) {
    if (m == 0) return BN254_OK;
    if (int e = bn_msm_check(d_p, d_k, offsets, m, d_out)) return e;          // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return bn_launch_msm(ctx, g, d_p, d_k, offsets, m, d_out, s); });
}
int bn254_g1_msm_batch_dev(bn254_ctx *c, const void *p, const void *k, const size_t *offsets, size_t m, void *o, void *s) { return msm_dev(c, 1, p, k, offsets, m, o, s); }
int bn254_g2_msm_batch_dev(bn254_ctx *c, const void *p, const void *k, const size_t *offsets, size_t m, void *o, void *s) { return msm_dev(c, 2, p, k, offsets, m, o, s); }
static int msm1_dev(bn254_ctx *ctx, int g, const void *d_p, const void *d_k, size_t n, void *d_out, void *stream) {
    if (int e = bn_msm1_check(d_p, d_k, n, d_out)) return e;                   // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) -> int {
        if (bn_msm_bucket_route(ctx, g, n)) return bn_launch_msm_bucket(ctx, g, d_p, d_k, n, d_out, s);
        const size_t off[2] = {0, n};
        return bn_launch_msm(ctx, g, d_p, d_k, off, 1, d_out, s);
    });
}
int bn254_g1_msm_dev(bn254_ctx *c, const void *p, const void *k, size_t n, void *o, void *s) { return msm1_dev(c, 1, p, k, n, o, s); }
int bn254_g2_msm_dev(bn254_ctx *c, const void *p, const void *k, size_t n, void *o, void *s) { return msm1_dev(c, 2, p, k, n, o, s); }
int bn254_g1_msm_prepare_dev(bn254_ctx *ctx, const void *d_p, size_t n, int window_bits, void **out, void *stream) {
    if (int e = bn_msm_prepare_check(d_p, n, window_bits, out)) return e;        // before any device lookup
    return bn_msmp_prepare_dev(ctx, 1, d_p, n, window_bits, out, stream);
}
int bn254_g2_msm_prepare_dev(bn254_ctx *ctx, const void *d_p, size_t n, int window_bits, void **out, void *stream) {
    if (int e = bn_msm_prepare_check(d_p, n, window_bits, out)) return e;        // before any device lookup
    return bn_msmp_prepare_dev(ctx, 2, d_p, n, window_bits, out, stream);
}
void bn254_msm_prepared_destroy(void *prep) {
    bn254_msm_prepared *h = (bn254_msm_prepared *)prep;
    if (!h) return;
    BnDeviceGuard dev_guard;
    hipSetDevice(h->device);
    bn_msmp_free(h);
}
size_t bn254_msm_prepared_count(const void *prep) { return prep ? ((const bn254_msm_prepared *)prep)->count : 0; }
size_t bn254_msm_prepared_bytes(const void *prep) {
    const bn254_msm_prepared *h = (const bn254_msm_prepared *)prep;
    return h ? h->table_bytes + h->count * (h->group == 1 ? sizeof(bn_g1) : sizeof(bn_g2)) : 0;
}
int bn254_msm_prepared_group(const void *prep) { return prep ? ((const bn254_msm_prepared *)prep)->group : 0; }
int bn254_msm_prepared_window_bits(const void *prep) { return prep ? (int)((const bn254_msm_prepared *)prep)->c : 0; }
int bn254_g1_msm_prepared_dev(bn254_ctx *c, const void *prep, size_t first, const void *k, size_t n, void *o, void *s) { return msmp_dev(c, 1, prep, first, k, n, o, s); }
int bn254_g2_msm_prepared_dev(bn254_ctx *c, const void *prep, size_t first, const void *k, size_t n, void *o, void *s) { return msmp_dev(c, 2, prep, first, k, n, o, s); }
// internal (not in the header; tests and tools/time_msm_prepared.py): the default window width of a handle of n points and the default
// crossover of a group
unsigned bn254_msm_prepared_default_window_bits(size_t n) { return bn_msm_prepared_window_bits(n); }
long bn254_msm_prepared_default_min(int g) { return g == 1 ? BN_MSMP_BUCKET_MIN_DEFAULT : BN_MSMP_BUCKET_MIN_DEFAULT_G2; }
// order of the checks: empty batch, arguments, then context and device
static int mul_base_dev(bn254_ctx *ctx, int g, const void *base, const void *d_k, void *d_out, size_t n, void *stream) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !base || !d_k || !d_out) return BN254_E_BAD_ARG;          // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return bn_launch_mul_base(ctx, g, base, d_k, d_out, n, s); });
}
int bn254_g1_mul_base_batch_dev(bn254_ctx *c, const bn_g1 *base, const void *k, void *o, size_t n, void *s) { return mul_base_dev(c, 1, base, k, o, n, s); }
int bn254_g2_mul_base_batch_dev(bn254_ctx *c, const bn_g2 *base, const void *k, void *o, size_t n, void *s) { return mul_base_dev(c, 2, base, k, o, n, s); }
// order of the checks: empty batch, arguments, then context and device
static int normalize_dev(bn254_ctx *ctx, int g, const void *d_p, void *d_out, size_t n, void *stream) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !d_p || !d_out) return BN254_E_BAD_ARG;                    // before any device lookup
    return bn_dev_entry(ctx, stream, true, [&](hipStream_t s) { return bn_launch_normalize(ctx, g, d_p, d_out, n, s); });
}
int bn254_g1_normalize_batch_dev(bn254_ctx *c, const void *p, void *o, size_t n, void *s) { return normalize_dev(c, 1, p, o, n, s); }
int bn254_g2_normalize_batch_dev(bn254_ctx *c, const void *p, void *o, size_t n, void *s) { return normalize_dev(c, 2, p, o, n, s); }
// no context-owned scratch: no scratch guard
static int eq_dev(bn254_ctx *ctx, int g, const void *d_a, const void *d_b, void *d_out, size_t n, void *stream) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !d_a || !d_b || !d_out) return BN254_E_BAD_ARG;            // before any device lookup
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return bn_launch_eq(ctx, g, d_a, d_b, d_out, n, s); });
}
int bn254_g1_eq_batch_dev(bn254_ctx *c, const void *a, const void *b, void *o, size_t n, void *s) { return eq_dev(c, 1, a, b, o, n, s); }
int bn254_g2_eq_batch_dev(bn254_ctx *c, const void *a, const void *b, void *o, size_t n, void *s) { return eq_dev(c, 2, a, b, o, n, s); }
// internal (not in the header; tests and tools/time_normalize.py): the shipped run length of the normalisation, and an override of its
// sub-launch size (0 restores BN_LAUNCH_MAX), so that a test reaches the seam between two sub-launches with a handful of points
unsigned bn254_normalize_run(void) { return bn254_normalize_run_M(); }
int bn254_normalize_set_launch_max(size_t points) { return g_norm_launch_max.set(points); }
// internal (not in the header; tests and tools/time_mul_base.py): the shipped window width of a group, the device bytes of one table, the
// slots per group, the scalars a table is built with (returns their count; writes 4 words each when `cap_words` suffices), and - for the
// width sweep only - a process-wide override of the width (0 restores the shipped one; tables of another width are rebuilt on use)
unsigned bn254_mul_base_window(int g) { return g == 1 ? BN_BASE_WINDOW_G1 : BN_BASE_WINDOW_G2; }
size_t bn254_mul_base_table_bytes(int g) { return bn254_mul_base_table_bytes_M(g, bn254_mul_base_window(g)); }
unsigned bn254_mul_base_slots(void) { return BN_BASE_SLOTS; }
size_t bn254_mul_base_table_scalars(unsigned c, uint64_t *out, size_t cap_words) {
    if (c < 3 || c > 16) return 0;
    size_t count = 0;
    (void)bn_no_throw([&]() -> int {
        std::vector<uint64_t> h;
        base_table_scalars(c, h);
        if (out && cap_words >= h.size()) memcpy(out, h.data(), h.size() * 8);
        count = h.size() / 4;
        return BN254_OK;
    });
    return count;
}
int bn254_mul_base_set_window(int g, unsigned c) {      // c = 2: W c = 254, the top window would carry
    return (g != 1 && g != 2) || (c != 0 && (c < 3 || c > 16)) ? BN254_E_BAD_ARG : g_base_window[g - 1].set(c);
}

// ---------------------------------------------------------------------------------------------- host-buffer API (BnHost: the context's mutex for the call)
int bn254_pairing_product_batch(bn254_ctx *ctx, const bn_g1 *p, const bn_g2 *q, const size_t *offsets, size_t m, bn_gt *out) {
    if (m == 0) return BN254_OK;
    if (int e = bn_seg_check(p, q, offsets, m, out)) return e;                // before any device lookup
    const size_t n = offsets[m];
    if (bn_seg_all_ones(offsets, m)) return bn254_pairing_batch(ctx, p, q, out, n);                 // every segment one pair: the pipelined batch path itself
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {p, n * sizeof(bn_g1)}, {q, n * sizeof(bn_g2)}, out, m * sizeof(bn_gt), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_pairing_product_batch_dev(ctx, d.in[0], d.in[1], offsets, m, d.out, ctx->stream); });
}
int bn254_pairing_product_batch_prepared_native(bn254_ctx *ctx, const bn_g1 *p, const bn254_g2_prepared *prep, const size_t *q_index, const size_t *offsets, size_t m, bn_gt *out) {
    if (m == 0) return BN254_OK;
    if (int e = bn_prep_seg_check(p, prep, q_index != nullptr, q_index, offsets, m, out)) return e;                // before any device lookup
    const size_t n = offsets[m];
    BnHost h(ctx); if (h.rc) return h.rc;
    if (prep->device != ctx->device) return BN254_E_BAD_ARG;
    return bn_staged(ctx, {p, n * sizeof(bn_g1)}, {q_index, n * sizeof(uint64_t)}, out, m * sizeof(bn_gt), nullptr, 0,
                     [&](const BnStaged &d) { return bn254_pairing_product_batch_prepared_native_dev(ctx, d.in[0], prep, d.in[1], offsets, m, d.out, ctx->stream); });
}
static int msm_host(bn254_ctx *ctx, int g, const void *p, const bn_fr *k, const size_t *offsets, size_t m, void *out) {
    if (m == 0) return BN254_OK;
    if (int e = bn_msm_check(p, k, offsets, m, out)) return e;                // before any device lookup
    const size_t n = offsets[m], V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    if (bn_seg_all_ones(offsets, m))                                          // every segment one term: the pipelined batch path itself
        return g == 1 ? bn254_g1_mul_batch(ctx, (const bn_g1 *)p, k, (bn_g1 *)out, n) : bn254_g2_mul_batch(ctx, (const bn_g2 *)p, k, (bn_g2 *)out, n);
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {p, n * V}, {k, n * sizeof(bn_fr)}, out, m * V, nullptr, 0,
                     [&](const BnStaged &d) { return msm_dev(ctx, g, d.in[0], d.in[1], offsets, m, d.out, ctx->stream); });
}
int bn254_g1_msm_batch(bn254_ctx *ctx, const bn_g1 *p, const bn_fr *k, const size_t *offsets, size_t m, bn_g1 *out) { return msm_host(ctx, 1, p, k, offsets, m, out); }
int bn254_g2_msm_batch(bn254_ctx *ctx, const bn_g2 *p, const bn_fr *k, const size_t *offsets, size_t m, bn_g2 *out) { return msm_host(ctx, 2, p, k, offsets, m, out); }
static int msm1_host(bn254_ctx *ctx, int g, const void *p, const bn_fr *k, size_t n, void *out) {
    if (int e = bn_msm1_check(p, k, n, out)) return e;                         // before any device lookup
    int rc = bn_get_ctx(ctx); if (rc) return rc;
    if (!bn_msm_bucket_route(ctx, g, n)) {
        const size_t off[2] = {0, n};
        return msm_host(ctx, g, p, k, off, 1, out);
    }
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {p, n * V}, {k, n * sizeof(bn_fr)}, out, V, nullptr, 0,
                     [&](const BnStaged &d) { return msm1_dev(ctx, g, d.in[0], d.in[1], n, d.out, ctx->stream); });
}
int bn254_g1_msm(bn254_ctx *ctx, const bn_g1 *p, const bn_fr *k, size_t n, bn_g1 *out) { return msm1_host(ctx, 1, p, k, n, out); }
int bn254_g2_msm(bn254_ctx *ctx, const bn_g2 *p, const bn_fr *k, size_t n, bn_g2 *out) { return msm1_host(ctx, 2, p, k, n, out); }
int bn254_g1_msm_prepare(bn254_ctx *ctx, const bn_g1 *p, size_t n, int window_bits, void **out) { return msmp_prepare_host(ctx, 1, p, n, window_bits, out); }
int bn254_g2_msm_prepare(bn254_ctx *ctx, const bn_g2 *p, size_t n, int window_bits, void **out) { return msmp_prepare_host(ctx, 2, p, n, window_bits, out); }
int bn254_g1_msm_prepared(bn254_ctx *ctx, const void *prep, size_t first, const bn_fr *k, size_t n, bn_g1 *out) { return msmp_host(ctx, 1, prep, first, k, n, out); }
int bn254_g2_msm_prepared(bn254_ctx *ctx, const void *prep, size_t first, const bn_fr *k, size_t n, bn_g2 *out) { return msmp_host(ctx, 2, prep, first, k, n, out); }
// (not bn_staged: one copy out of the handle's table, nothing staged)
int bn254_msm_prepared_export(bn254_ctx *ctx, const void *prep, void *host_table, size_t bytes) {
    const bn254_msm_prepared *hp = (const bn254_msm_prepared *)prep;
    if (!hp || bytes != hp->table_bytes || (bytes && !host_table)) return BN254_E_BAD_ARG;
    BnHost h(ctx); if (h.rc) return h.rc;
    if (hp->device != ctx->device) return BN254_E_BAD_ARG;
    if (bytes) HIP_TRY(hipMemcpyAsync(host_table, hp->table, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return BN254_OK;
}
static int mul_base_host(bn254_ctx *ctx, int g, const void *base, const bn_fr *k, void *out, size_t n) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !base || !k || !out) return BN254_E_BAD_ARG;              // before any device lookup
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {k, n * sizeof(bn_fr)}, {nullptr, 0}, out, n * V, nullptr, 0,
                     [&](const BnStaged &d) { return mul_base_dev(ctx, g, base, d.in[0], d.out, n, ctx->stream); });
}
int bn254_g1_mul_base_batch(bn254_ctx *ctx, const bn_g1 *base, const bn_fr *k, bn_g1 *out, size_t n) { return mul_base_host(ctx, 1, base, k, out, n); }
int bn254_g2_mul_base_batch(bn254_ctx *ctx, const bn_g2 *base, const bn_fr *k, bn_g2 *out, size_t n) { return mul_base_host(ctx, 2, base, k, out, n); }
static int normalize_host(bn254_ctx *ctx, int g, const void *p, void *out, size_t n) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !p || !out) return BN254_E_BAD_ARG;                        // before any device lookup
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {p, n * V}, {nullptr, 0}, out, n * V, nullptr, 0,
                     [&](const BnStaged &d) { return normalize_dev(ctx, g, d.in[0], d.out, n, ctx->stream); });
}
int bn254_g1_normalize_batch(bn254_ctx *ctx, const bn_g1 *p, bn_g1 *out, size_t n) { return normalize_host(ctx, 1, p, out, n); }
int bn254_g2_normalize_batch(bn254_ctx *ctx, const bn_g2 *p, bn_g2 *out, size_t n) { return normalize_host(ctx, 2, p, out, n); }
static int eq_host(bn254_ctx *ctx, int g, const void *a, const void *b, int32_t *out, size_t n) {
    if (n == 0) return BN254_OK;
    if (n > BN_N_MAX || !a || !b || !out) return BN254_E_BAD_ARG;                  // before any device lookup
    const size_t V = g == 1 ? sizeof(bn_g1) : sizeof(bn_g2);
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_staged(ctx, {a, n * V}, {b, n * V}, out, n * sizeof(int32_t), nullptr, 0,
                     [&](const BnStaged &d) { return eq_dev(ctx, g, d.in[0], d.in[1], d.out, n, ctx->stream); });
}
int bn254_g1_eq_batch(bn254_ctx *ctx, const bn_g1 *a, const bn_g1 *b, int32_t *out, size_t n) { return eq_host(ctx, 1, a, b, out, n); }
int bn254_g2_eq_batch(bn254_ctx *ctx, const bn_g2 *a, const bn_g2 *b, int32_t *out, size_t n) { return eq_host(ctx, 2, a, b, out, n); }

}  // extern "C"
