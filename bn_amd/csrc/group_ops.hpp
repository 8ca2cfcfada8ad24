// The per-lane bodies of the group kernels (bn254_kernels_mul.hip): point I/O, the 80-byte table record, the complete addition, the segmented
// fold of bn254_g{1,2}_msm_batch, the accumulation levels and the reduction of the bucket method (bn254_g{1,2}_msm), the fixed-base chain
// (bn254_g{1,2}_mul_base_batch), the table build and level 0 of the prepared bases (bn254_g{1,2}_msm_prepared), the shared-inversion normalisation (bn254_g{1,2}_normalize_batch) and the projective comparison
// (bn254_g{1,2}_eq_batch).  Everything here is pure and takes plain pointers and a lane (G2: lane pair) index, so the host simulation
// (tests/hostsim/hostsim.cpp) runs the very same bodies over host arrays; what needs a wave, a workgroup or a launch stays in the .hip.
#pragma once
#include "curve.hpp"
#include "io.hpp"
#include <type_traits>

#if defined(BN_HOSTSIM)
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return {x, y, z, w}; }
inline uint32_t min(uint32_t a, uint32_t b) { return a < b ? a : b; }
#endif

// The argument records of the generic kernels bn254_g{1,2}_add_M<Args>.  They are template arguments of those kernels, so their names are part
// of the kernels' symbols: they stay in the unnamed namespace, where they were first declared.
namespace {
struct MsmAccArgs {          // one accumulation level of the bucket method (msm_acc_body)
    const uint32_t *pts, *idx, *keys, *n0; uint32_t level; uint32_t *out_pts, *out_keys, *buckets;
};
struct MsmReduceArgs {       // the bucket reduction (msm_reduce_body)
    const uint32_t *buckets; uint32_t G, groups, log2B, count; uint32_t *terms;       // terms: S of every lane, then T of every lane
};
struct MsmAccPrepArgs {      // level 0 of the accumulation over a prepared table (msm_acc_prep_body)
    const uint4 *table; const uint32_t *idx, *keys, *n0; uint32_t *out_pts, *out_keys, *buckets;
};
struct MsmPrepDoubleArgs {   // one window step of a prepared table's build (msm_prep_double_body)
    uint32_t *pts; uint32_t c;
};
struct BaseMulArgs {         // the fixed-base chain (base_mul_body)
    const uint32_t *k; uint32_t *out; const uint4 *table; uint32_t c, W;
};
struct NormalizeArgs {       // the normalisation with one inversion per run of points (normalize_body); out may be p itself
    const uint32_t *p; uint32_t *out; uint4 *prefix; uint32_t n;
};
struct EqArgs {              // the projective comparison (eq_body)
    const uint32_t *a, *b; int32_t *out;
};
}  // namespace

namespace bn254 {
// ---- a Jacobian point <-> its 24 (G1) / 48 (G2) words, for every Fq2 mapping
template <class F> struct PointIo;
template <> struct PointIo<FqField> {
    static constexpr uint32_t WORDS = 24;
    BN_FN Jac<FqField> operator()(const uint32_t *w) const { return Jac<FqField>{fe_from_u32x8(w), fe_from_u32x8(w + 8), fe_from_u32x8(w + 16)}; }
    BN_FN void operator()(const Jac<FqField> &r, uint32_t *o) const { fe_to_u32x8(r.x, o); fe_to_u32x8(r.y, o + 8); fe_to_u32x8(r.z, o + 16); }
    BN_FN Fe z(const uint32_t *w) const { return fe_from_u32x8(w + 16); }           // the z coordinate alone
};
template <class F2> struct PointIo<Fq2Field<F2>> {
    typedef Fq2Field<F2> F;
    static constexpr uint32_t WORDS = 48;
    BN_FN Jac<F> operator()(const uint32_t *w) const { return Jac<F>{f2_load((const F2 *)nullptr, w), f2_load((const F2 *)nullptr, w + 16), f2_load((const F2 *)nullptr, w + 32)}; }
    BN_FN void operator()(const Jac<F> &r, uint32_t *o) const { f2_store(r.x, o); f2_store(r.y, o + 16); f2_store(r.z, o + 32); }
    BN_FN F2 z(const uint32_t *w) const { return f2_load((const F2 *)nullptr, w + 32); }
};
// the canonical integer of the scalar at k (8 words in Montgomery form)
BN_FN void fr_load_raw(const uint32_t *k, uint32_t raw[8]) {
    uint32_t kw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kw[i] = k[i];
    fr_from_mont(kw, raw);
}
// ---- the 80-byte record of an affine table entry: the 9 + 9 limbs of (x, y) - Fe, or one lane's components of an Fq2B pair - and two words,
// read and written as five 16-byte groups.  Word 18 is a flag (the fixed-base tables mark an entry at infinity), word 19 is zero.
// 16-byte groups per entry: 5 = packed (80 B: an entry may straddle two 128-byte lines; one whole line per entry measured no faster, a
// prefetch one window ahead 2 % slower: profiles/r04c_ab_g1mul.txt)
constexpr uint32_t AFF_ENTRY_U4 = 5, AFF_LANE_U4 = 8 * AFF_ENTRY_U4;                 // 80 B per entry, 640 B per lane
template <class Index>
BN_FN void aff_record_pack(const Fe &x, const Fe &y, uint32_t flag, uint4 *table, Index entry) {          // record `entry` of `table`
    uint32_t w[20];
#pragma unroll
    for (int i = 0; i < 9; ++i) { w[i] = x.l[i]; w[9 + i] = y.l[i]; }
    w[18] = flag; w[19] = 0;
    uint4 *rec = table + entry * AFF_ENTRY_U4;
#pragma unroll
    for (int g = 0; g < 5; ++g) rec[g] = make_uint4(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]);
}
BN_FN uint32_t aff_record_unpack(const uint4 *rec, Fe &x, Fe &y) {                  // returns the flag
    uint32_t w[20];
#pragma unroll
    for (int g = 0; g < 5; ++g) { const uint4 v = rec[g]; w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w; }
#pragma unroll
    for (int i = 0; i < 9; ++i) { x.l[i] = w[i]; y.l[i] = w[9 + i]; }
    BN_SETB(x, 1, 2); BN_SETB(y, 1, 2);                                              // what is packed is a product (fe_mul, fe_from_u32x8)
    BN_VERIFY(x, "aff_record_unpack"); BN_VERIFY(y, "aff_record_unpack");
    return w[18];
}
// The affine window table of a lane in global memory: [lane][entry 1..8][record] - a lane reads the entry of ITS digit as five 16-byte
// loads from one or two cache lines (curve.hpp AffTableVars explains why not a private array).
// G1: (x, y) are Fe; G2 in the lane-pair mapping: this lane's components of (x, y)
template <class F>
struct AffTableMem {
    uint4 *base;             // this lane's 8 entries
    BN_FN void put(int i, const Aff<F> &v) const {
        if constexpr (std::is_same<F, FqField>::value) aff_record_pack(v.x, v.y, 0, base, (uint32_t)(i - 1));
        else aff_record_pack(v.x.v, v.y.v, 0, base, (uint32_t)(i - 1));
    }
    BN_FN Aff<F> get(int i) const {
        const uint4 *e = base + (uint32_t)(i - 1) * AFF_ENTRY_U4;
        Aff<F> r;
        if constexpr (std::is_same<F, FqField>::value) aff_record_unpack(e, r.x, r.y);
        else aff_record_unpack(e, r.x.v, r.y.v);
        return r;
    }
};
// ---- a[i] + b[i]  (or a[i] - b[i] = a[i] + (-b[i]): lib.rs:103-114,146-157, groups/mod.rs:275-347): the reference's add-2007-bl
// with its zero / equal-point branches, so the Jacobian limbs returned are the reference's own
template <class F>
BN_FN Jac<F> add_body(const Jac<F> &a, Jac<F> b, int negate_b) {
    const bool bz = F::is_zero(b.z);
    if (negate_b) b.y = F::select(bz, F::template lc3<-1, 0, 0>(b.y, b.y, b.y), b.y);     // neg(0) = 0 (groups/mod.rs:334-346)
    return jac_add_flags<F>(a, b, F::is_zero(a.z), bz);
}
// One level of the segmented fold of bn254_g{1,2}_msm_batch: lane (G2: lane pair) i adds the pieces[i].cnt consecutive Jacobian points at
// pieces[i].src in index order - a serial chain chosen by the host (at most BN_MSM_FOLD = 4 values) - into pieces[i].dst; an empty piece is
// the point at infinity.  The COMPLETE addition: two equal terms of a segment double, P*k + P*(r-k) cancels, and a partial sum at infinity is
// the left operand of the next addition.  pieces[i].last: the sum of a whole segment, normalised (infinity: G::zero() = (0, 1, 0)).
// The caller stores the result at pc.dst (a clamped lane pair of G2 computes it and keeps it to itself).
template <class F>
BN_FN Jac<F> msm_fold_body(const BnSegPiece &pc) {
    const PointIo<F> io;
    Jac<F> acc = {F::zero(), F::one(), F::zero()};
    if (pc.cnt) acc = io(pc.src);
#pragma unroll 1
    for (uint32_t j = 1; j < pc.cnt; ++j) {
        const Jac<F> q = io(pc.src + PointIo<F>::WORDS * j);
        acc = jac_add_flags<F>(acc, q, F::is_zero(acc.z), F::is_zero(q.z));
    }
    if (pc.last) acc = jac_normalize<F>(acc);
    return acc;
}
// ---- bucket (Pippenger) method of bn254_g{1,2}_msm: one large sum (bn254_hip.hip bn_launch_msm_bucket plans the launches)
// A scalar is cut into W = ceil(254 / c) unsigned c-bit digits; term i belongs to bucket KEY = w * 2^c + digit for every window w whose digit
// is not zero.  The integer kernels (bn254_kernels_mul.hip MsmDigitsOp, MsmScanOp) count the terms per key, scan the counts and scatter
// (term index, key) into key order - a counting sort, arbitrary order inside a key.
constexpr uint32_t MSM_NONE = 0x7fffffffu;        // key of an unused entry
constexpr uint32_t MSM_SKIP = 0x80000000u;        // key flag: the entry belongs to the run of its key but carries no point
constexpr uint32_t MSM_PIECE = 16;                // entries per lane of one accumulation level: the longest serial chain, whatever the data
constexpr uint32_t MSM_TILE = 1024;               // counts per workgroup of the scan (256 threads x 4)
BN_FN uint32_t msm_digit(const uint32_t *raw, uint32_t w, uint32_t c) {
    const uint32_t bit = w * c, word = bit >> 5;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) { if (i == word) lo = raw[i]; if (i == word + 1) hi = raw[i]; }      // selects: `raw` stays in registers
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (bit & 31u)) & ((1u << c) - 1u);
}
// One level of the bucket accumulation.  The input is a sequence of N entries in key order (level 0: the sorted terms, their points gathered
// by index; level l > 0: the partial sums level l - 1 wrote); lane (G2: lane pair) i adds the entries [i * MSM_PIECE, (i + 1) * MSM_PIECE) with
// the complete addition, run by run.  A run of one key that lies inside the lane's entries is complete: buckets[key] += sum (the buckets
// collect over the chunks of a call).  A run that began before the lane's first entry or goes on behind its last one is a piece of a longer
// run: its sum becomes an entry of the next level - slot 2i for a run that began earlier, slot 2i + 1 for one that goes on (a run over ALL of
// the lane's entries takes slot 2i and marks 2i + 1 MSM_SKIP, so that the key's run stays contiguous) - and the next level, eight times
// shorter, does the same.  So no lane's chain exceeds 2 * MSM_PIECE additions (every entry a run of its own) whatever the scalars are: 2^20 equal scalars are 2^16 lanes of
// 16 terms, then 2^13, ... - never one chain of 2^20.  N = the level-0 count on the device (*n0) taken through the levels.
// A lane past the level's entries has nothing to do (both lanes of a pair alike).
BN_FN uint32_t msm_level_len(uint32_t n, uint32_t level) {
    for (uint32_t l = 0; l < level; ++l) n = 2u * ((n + MSM_PIECE - 1) / MSM_PIECE);
    return n;
}
template <class F>
BN_FN void msm_acc_body(const MsmAccArgs &g, uint32_t i) {
    constexpr uint32_t WORDS = PointIo<F>::WORDS;
    const PointIo<F> io;
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
            const Jac<F> q = io(src);
            acc = jac_add_flags<F>(acc, q, F::is_zero(acc.z), F::is_zero(q.z));
        }
        if (dst) io(acc, dst);
        if (at_end) break;
        if (flush) { first_run = false; acc = {F::zero(), F::one(), F::zero()}; cur = key; }
        else ++j;
    }
}
// The bucket reduction: lane (lane pair) t = w * groups + g walks the G buckets [base, base + G) of window w from the top with a running sum,
// two additions per bucket, and leaves S = sum B_b and T = sum (b - base) B_b as two terms of the tail - the one-segment bn254_g{1,2}_msm_batch
// over 2 * W * groups terms whose scalars the host knows: base * 2^(c w) for S, 2^(c w) for T.
template <class F>
BN_FN void msm_reduce_body(const MsmReduceArgs &g, uint32_t t) {
    constexpr uint32_t WORDS = PointIo<F>::WORDS;
    const PointIo<F> io;
    const uint32_t w = t / g.groups, base = (w << g.log2B) + (t % g.groups) * g.G;
    Jac<F> run = {F::zero(), F::one(), F::zero()}, T = run;
#pragma unroll 1
    for (uint32_t b = g.G; b-- > 0;) {
        const Jac<F> q = io(g.buckets + (size_t)(base + b) * WORDS);
        run = jac_add_flags<F>(run, q, F::is_zero(run.z), F::is_zero(q.z));
        if (b) T = jac_add_flags<F>(T, run, F::is_zero(T.z), F::is_zero(run.z));
    }
    io(run, g.terms + (size_t)t * WORDS);
    io(T, g.terms + (size_t)(g.count + t) * WORDS);
}
// ---- fixed-base scalar multiplication of bn254_g{1,2}_mul_base_batch: out[i] = normalize(B * k[i]) for ONE base B per call
// (bn254_seg.hip bn_launch_mul_base keeps the tables and plans the launches).  The table of a base holds the AFFINE points d * 2^(c w) * B for
// w < W = ceil(254 / c) and d = 1 .. 2^(c-1), entry (w, d) at index w * 2^(c-1) + d - 1, as the records above - G1 one record per entry,
// G2 two (component c0 for the even lane of a pair, c1 for the odd one).  The flag of a record is not zero when the entry is the point at
// infinity (the base was).
// The chain: the canonical integer of the scalar is recoded, low window first, into W signed c-bit digits in [-2^(c-1), 2^(c-1)] with a
// carry (the top window of a scalar below r < 2^254 <= 2^(c W - 1) never carries), and every non-zero digit is ONE mixed addition of the
// entry |d| of its window, y negated for d < 0 - no doubling, and the accumulator starts at infinity.  The partial sum below window w is
// smaller than 2^(c w) in absolute value, so it never equals +- the entry of window w as an INTEGER; mod r that argument holds up to the
// top window only: k = r - 2 (r mod 2^(c (W-1))) recodes (when the low part carries, as it does for c = 8, 10 and 12) to a partial sum -t B and a top entry
// (r - t) B, the same point.  The additions are therefore the complete ones (jac_madd_signed / jac_madd_flags: equal points double,
// opposite points and an accumulator at infinity are followed by flags).
template <class F>
BN_FN Aff<F> base_entry(const uint4 *rec, bool &inf) {
    Aff<F> r;
    Fe x, y;
    inf = aff_record_unpack(rec, x, y) != 0;
    if constexpr (std::is_same<F, FqField>::value) { r.x = x; r.y = y; } else { r.x.v = x; r.y.v = y; }
    return r;
}
// Where a lane finds entry e of the table (the counterpart of AffTableMem / AffTableVars for the window tables): the kernels read ONE record,
// G1 the entry's only one, a G2 lane the one of its component comp = lane & 1 - both lanes of a pair walk the same digits.  (A simulated
// lane pair holds both components in one value and fetches both records: tests/hostsim/hostsim.cpp.)  The caller hands in `io` like the table.
template <class F>
struct BaseTableMem {
    static constexpr uint32_t REC = std::is_same<F, FqField>::value ? AFF_ENTRY_U4 : 2 * AFF_ENTRY_U4;            // 16-byte groups per table entry
    const uint4 *table; uint32_t comp;
    BN_FN Aff<F> get(uint32_t e, bool &inf) const { return base_entry<F>(table + (size_t)e * REC + comp * AFF_ENTRY_U4, inf); }
};
template <class F, class Tab>
BN_FN void base_mul_body(const BaseMulArgs &g, uint32_t i, Tab tab, PointIo<F> io) {
    constexpr bool G1 = std::is_same<F, FqField>::value;
    uint32_t raw[8];
    fr_load_raw(g.k + 8u * i, raw);
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
        const Aff<F> q = tab.get(w * half + (ad ? ad - 1u : 0u), e_inf);
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
    io(jac_normalize<F>(acc), g.out + (size_t)i * io.WORDS);
}
// ---- multi-scalar multiplication against prepared bases: bn254_g{1,2}_msm_prepare / bn254_g{1,2}_msm_prepared (bn254_seg.hip keeps the handle
// and plans the launches).  The handle's table holds the AFFINE points 2^(c w) P_i for w < W = ceil(254 / c), entry (w, i) at index
// w * count + i, as the records of the fixed-base tables (G2 two per entry, BaseTableMem reads them).  A scalar is recoded into the W signed
// digits of base_mul_body; digit d != 0 of window w puts entry (w, i), y negated for d < 0, into bucket |d| - 1 - ONE set of 2^(c-1) buckets
// for all windows, since the weights 2^(c w) are in the entries - and the sum is sum_b (b + 1) B_b.
// Digit w of the recoding, low window first: returns |d| <= 2^(c-1), `neg` for d < 0; `carry` (0 before window 0) goes from window to
// window: v > 2^(c-1) carries.  The top window of a scalar below r < 2^254 <= 2^(c W - 1) leaves no carry.
BN_FN uint32_t msm_signed_digit(const uint32_t *raw, uint32_t w, uint32_t c, uint32_t &carry, bool &neg) {
    const uint32_t half = 1u << (c - 1), v = msm_digit(raw, w, c) + carry;
    carry = v > half ? 1u : 0u;
    neg = carry != 0;
    return carry ? 2u * half - v : v;
}
constexpr uint32_t MSM_NEG = 0x80000000u;         // index flag of a sorted entry: the table entry is subtracted
// The build of a table, window by window: lane (G2: lane pair) i doubles the running Jacobian point i c times in place,
// 2^(c w) P_i -> 2^(c (w + 1)) P_i (infinity stays infinity: z3 = 2 y z); the host normalises and repacks every window's points.
template <class F>
BN_FN void msm_prep_double_body(const MsmPrepDoubleArgs &g, uint32_t i, PointIo<F> io) {
    uint32_t *w = g.pts + (size_t)i * io.WORDS;
    Jac<F> p = io(w);
#pragma unroll 1
    for (uint32_t j = 0; j < g.c; ++j) p = jac_double(p);
    io(p, w);
}
// Level 0 of the accumulation over a prepared table: the runs, slots and MSM_SKIP markers of msm_acc_body (N = *n0 entries in key order,
// MSM_PIECE per lane), but entry j is ONE record - table entry idx[j] & ~MSM_NEG, subtracted when idx[j] & MSM_NEG - and joins its run by
// the COMPLETE mixed addition: the same point twice in a bucket doubles, P and -P cancel, a flagged record (a base at infinity) is skipped.
// A complete run joins its bucket by the full Jacobian addition; the pieces of longer runs are Jacobian entries of level 1, which is
// msm_acc_body.  `tab`: where a lane finds a record (BaseTableMem; a simulated lane pair fetches both components).
template <class F, class Tab>
BN_FN void msm_acc_prep_body(const MsmAccPrepArgs &g, uint32_t i, Tab tab) {
    constexpr uint32_t WORDS = PointIo<F>::WORDS;
    const PointIo<F> io;
    const uint32_t N = *g.n0, a = i * MSM_PIECE;
    if (a >= N) return;
    const uint32_t b = min(a + MSM_PIECE, N);
    const uint32_t prev = a ? g.keys[a - 1] & ~MSM_SKIP : 0xffffffffu, next = b < N ? g.keys[b] & ~MSM_SKIP : 0xffffffffu;
    g.out_keys[2 * i] = MSM_NONE; g.out_keys[2 * i + 1] = MSM_NONE;
    Jac<F> acc = {F::zero(), F::one(), F::zero()};
    bool acc_inf = true;
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
            if (src) {
                const Jac<F> q = io(src);
                acc = jac_add_flags<F>(acc, q, F::is_zero(acc.z), F::is_zero(q.z));
            }
            if (dst) io(acc, dst);
        } else if (!(kj & MSM_SKIP) && key != MSM_NONE) {
            const uint32_t e = g.idx[j];
            const bool neg = (e & MSM_NEG) != 0;
            bool e_inf;
            const Aff<F> q = tab.get(e & ~MSM_NEG, e_inf);
            if constexpr (std::is_same<F, FqField>::value) {
                acc = jac_madd_signed(acc, q, neg, acc_inf, e_inf);
            } else {
                Aff<F> qs = q;
                qs.y = F::select(neg, q.y, F::template lc3<-1, 0, 0>(q.y, q.y, q.y));
                acc = jac_madd_flags<F>(acc, qs, acc_inf, e_inf);
                acc_inf = F::is_zero_std(acc.z);
            }
        }
        if (at_end) break;
        if (flush) { first_run = false; acc = {F::zero(), F::one(), F::zero()}; acc_inf = true; cur = key; }
        else ++j;
    }
}
// ---- normalisation of bn254_g{1,2}_normalize_batch: out[i] = (x / z^2, y / z^3, 1), the point at infinity (z == 0, whatever x and y hold)
// as G::zero() = (0, 1, 0) - jac_normalize (curve.hpp) with ONE inversion per run of points (Montgomery's trick) instead of one per point.
// Lane (G2: lane pair) i owns the run of the at most K consecutive points [i K, min(n, (i + 1) K)):
//   forward    prefix[j] = z'_a z'_(a+1) ... z'_j, with z' = z, or one where z == 0 - a point at infinity must not zero the product of its run
//   inversion  of the run's product (safegcd, fe_inverse)
//   backward   j from the run's end: 1 / z_j = inv * prefix[j - 1], inv *= z'_j, the point from (1 / z_j)^2 and (1 / z_j)^3, (0, 1, 0) selected
//              where z == 0
// 3 products per point on top of the 4 of jac_normalize, and 1 / K of an inversion.  The prefix products live in memory - one field element
// per point, `prefix`: scratch of the caller -, not in registers: K live field elements are 9 K VGPRs of a kernel that may not spill, and
// the loops need no unrolling.  The backward pass reads point j completely before it writes out[j], and no lane reads
// another lane's points, so out may be p.  The inverse of a field element is unique and the stores are canonical: the bytes do not depend
// on K, and they are those of jac_normalize.
// A prefix record: the 9 limbs of the product (a product: normalized, below 2q) in three 16-byte groups; a G2 point has two, component c0
// for the even lane of the pair and c1 for the odd one, like the table records above.
constexpr uint32_t NORM_PREFIX_U4 = 3;
constexpr uint32_t NORM_RUN = 8;                  // points per inversion, one constant for both groups: of 1 / 4 / 8 / 16 the fastest for G2, within 4 % of 16 for G1 (profiles/r12_normalize.txt)
BN_FN void prefix_record_put(const Fe &a, uint4 *rec) {
    rec[0] = make_uint4(a.l[0], a.l[1], a.l[2], a.l[3]); rec[1] = make_uint4(a.l[4], a.l[5], a.l[6], a.l[7]); rec[2] = make_uint4(a.l[8], 0, 0, 0);
}
BN_FN Fe prefix_record_get(const uint4 *rec) {
    const uint4 u = rec[0], v = rec[1], w = rec[2];
    Fe a;
    a.l[0] = u.x; a.l[1] = u.y; a.l[2] = u.z; a.l[3] = u.w; a.l[4] = v.x; a.l[5] = v.y; a.l[6] = v.z; a.l[7] = v.w; a.l[8] = w.x;
    BN_SETB(a, 1, 2);                                                                // what is stored is a product (fe_mul, fe_from_u32x8)
    BN_VERIFY(a, "prefix_record_get");
    return a;
}
// Where a lane keeps the prefix product of point j (the counterpart of BaseTableMem): G1 the one record of the point, a G2 lane the record of
// its component comp = lane & 1.  (A simulated lane pair holds both components in one value and keeps both records:
// tests/hostsim/hostsim_normalize.cpp.)
template <class F>
struct PrefixMem {
    static constexpr uint32_t REC = std::is_same<F, FqField>::value ? NORM_PREFIX_U4 : 2 * NORM_PREFIX_U4;        // 16-byte groups per point
    uint4 *base; uint32_t comp;
    BN_FN void put(uint32_t j, const typename F::T &a) const {
        if constexpr (std::is_same<F, FqField>::value) prefix_record_put(a, base + (size_t)j * REC);
        else prefix_record_put(a.v, base + (size_t)j * REC + comp * NORM_PREFIX_U4);
    }
    BN_FN typename F::T get(uint32_t j) const {
        typename F::T r;
        if constexpr (std::is_same<F, FqField>::value) r = prefix_record_get(base + (size_t)j * REC);
        else r.v = prefix_record_get(base + (size_t)j * REC + comp * NORM_PREFIX_U4);
        return r;
    }
};
template <class F, class Pre>
BN_FN void normalize_body(const NormalizeArgs &g, uint32_t i, uint32_t K, Pre pre, PointIo<F> io) {
    using T = typename F::T;
    const uint32_t a = i * K;
    if (a >= g.n) return;
    const uint32_t b = min(a + K, g.n);
    T acc = F::one();
#pragma unroll 1
    for (uint32_t j = a; j < b; ++j) {
        const T z = io.z(g.p + (size_t)j * io.WORDS);                                // a product: is_zero_std applies
        const T zs = F::select(F::is_zero_std(z), z, F::one());
        acc = j == a ? zs : F::mul(acc, zs);
        if (j + 1 < b) pre.put(j, acc);
    }
    T inv = F::inverse(acc);
#pragma unroll 1
    for (uint32_t j = b; j-- > a;) {
        const Jac<F> p = io(g.p + (size_t)j * io.WORDS);
        const bool inf = F::is_zero_std(p.z);
        T zi = inv;
        if (j > a) {
            zi = F::mul(inv, pre.get(j - 1));
            inv = F::mul(inv, F::select(inf, p.z, F::one()));
        }
        const T zi2 = F::sqr(zi);
        Jac<F> r = {F::mul(p.x, zi2), F::mul(p.y, F::mul(zi2, zi)), F::one()};
        r.x = F::select(inf, r.x, F::zero()); r.y = F::select(inf, r.y, F::one()); r.z = F::select(inf, r.z, F::zero());
        io(r, g.out + (size_t)j * io.WORDS);
    }
}
// ---- a[i] == b[i] as group elements (PartialEq for G<P>, groups/mod.rs:83-109): both at infinity - equal; exactly one - not; otherwise
// x1 z2^2 == x2 z1^2 and y1 z2^3 == y2 z1^3.  Two squarings and six products, no inversion.  The two sides are lazy residues (below 2q), so
// what is compared with zero is their fully reduced difference (the equal-point test of jac_add_flags), never the limbs of the two products.
template <class F>
BN_FN int32_t eq_body(const Jac<F> &p, const Jac<F> &q) {
    using T = typename F::T;
    const bool pz = F::is_zero_std(p.z), qz = F::is_zero_std(q.z);                   // loaded coordinates are products
    const T z1s = F::sqr(p.z), z2s = F::sqr(q.z);
    const T u1 = F::mul(p.x, z2s), u2 = F::mul(q.x, z1s);
    const T s1 = F::mul(p.y, F::mul(q.z, z2s)), s2 = F::mul(q.y, F::mul(p.z, z1s));
    const T h = F::template lc3<1, -1, 0>(u2, u1, u1), sd = F::template lc3<1, -1, 0>(s2, s1, s1);
    const bool same = F::is_zero_std(h) && F::is_zero_std(sd);
    return (pz || qz) ? (pz && qz ? 1 : 0) : (same ? 1 : 0);
}
}  // namespace bn254
