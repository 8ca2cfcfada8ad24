// The per-lane bodies of the segmented scans over Fr (bn254_scan.hip): bn254_fr_scan_batch and its _dev twin, the first-order linear recurrence
//     out[t] = a[t] * prev + b[t],   prev = out[t-1], or init[j] at the first term of segment j
// (a == NULL: prefix sums, b == NULL: prefix products, one a per segment: powers, Horner's rule, synthetic division).  A term is the affine
// map y -> a y + b, and "(A, B) then (A', B')" = (A A', A' B + B') is associative, so the host (host_plan.hpp bn_scan_plan) cuts every segment
// into PIECES of at most P consecutive terms and a lane owns one piece of the work list (io.hpp BnScanPiece):
//   reduce  composes the terms of a piece into its map (A, B) - two products per term; without b the map is A alone, without a it is B alone
//   up      composes at most F consecutive maps of one segment into one, level after level until at most F are left
//   down    takes the value in front of its group (at the top: init[j] or the default) and walks its at most F maps, leaving in front of
//           every child the value the recurrence has there
//   apply   runs the recurrence over a piece from the value in front of it - one product per term - and writes out; a segment of at most P
//           terms is one such lane and nothing else ("direct": it starts from init[j])
// so the length of a lane's serial chain is a constant of the plan, never a property of the data, and no lane waits for another: the order
// between the levels is the order of the launches on their stream.  Every product and every sum is canonical (fr.hpp), hence the bytes are
// those of the Python-integer recurrence whichever way the plan cuts a segment.  Everything is pure and takes plain pointers and a lane
// index, so the host simulation (tests/hostsim/hostsim_scan.cpp) runs the very same bodies over host arrays.
#pragma once
#include "fr_ops.hpp"
#include "io.hpp"

namespace bn254 {

// The shipped choices (plain constants; bn254_scan.hip carries a run-time override of the piece length for the sweep of tools/time_scan.py
// only).  Terms per piece: the rule fixed before measuring is "the fastest of 8 / 16 / 32 / 64 on ONE segment of 2^22 terms ships"; that is
// 32, which is also the fastest on the two other measured shapes (profiles/r16_scan.txt).  Maps per lane of an up or down level: not swept.
constexpr uint32_t FR_SCAN_PIECE = 32;
constexpr uint32_t FR_SCAN_FAN = 16;

// the flags of the C ABI (include/bn254_hip.h BN254_SCAN_*)
constexpr uint32_t FR_SCAN_REVERSE = 1, FR_SCAN_EXCLUSIVE = 2, FR_SCAN_A_PER_SEGMENT = 4;

// The arrays of one call.  a, b, init: the caller's (a or b may be NULL, never both; init may be NULL); map_a, map_b: the maps of the pieces
// and of the groups above them, one record per scratch slot (map_a is read only with a, map_b only with b); carry: the value in front of
// every slot; out: the caller's.
struct FrScanArrays {
    const uint32_t *a, *b, *init;
    uint32_t *map_a, *map_b, *carry, *out;
    uint32_t flags;
};

// init[j], or its default: Fr::zero() for a recurrence with b (sums start from nothing), Fr::one() for plain products
BN_FN Fr fr_scan_init(const FrScanArrays &s, uint64_t seg) { return s.init ? fr_load(s.init, seg) : (s.b ? fr_zero() : fr_one()); }
// term j of a piece that starts at term `first`: a REVERSE scan walks its segment from the last term to the first
BN_FN uint64_t fr_scan_term(const FrScanArrays &s, uint64_t first, uint32_t j) { return (s.flags & FR_SCAN_REVERSE) ? first - j : first + j; }

// Terms a lane loads before it computes on them: four records are one 128-byte line.  Neighbouring lanes are a whole piece apart, so a
// lane that took one record per step would touch every line of its piece four times, with all the other lanes' lines in between.
constexpr uint32_t FR_SCAN_CHUNK = 4;

// (A, B) = the maps xa[at], xb[at] for at = first, first + 1, .. (backwards: first - 1, ..) composed in that order: A = prod xa, B = B * xa + xb
// at every one.  With `per_seg` the factor of every term is the one value seg_a and xa is not read.  The caller says which halves exist.
BN_FN void fr_scan_compose(const uint32_t *xa, const uint32_t *xb, const Fr &seg_a, bool per_seg, bool has_a, bool has_b, uint64_t first, uint32_t len, bool backwards, Fr &A,
                           Fr &B) {
    A = fr_one(); B = fr_zero();
#pragma unroll 1
    for (uint32_t j0 = 0; j0 < len; j0 += FR_SCAN_CHUNK) {
        Fr x[FR_SCAN_CHUNK], y[FR_SCAN_CHUNK];
#pragma unroll
        for (uint32_t k = 0; k < FR_SCAN_CHUNK; ++k) {
            x[k] = seg_a; y[k] = fr_zero();
            if (j0 + k < len) {
                const uint64_t at = backwards ? first - (j0 + k) : first + (j0 + k);
                if (has_a && !per_seg) x[k] = fr_load(xa, at);
                if (has_b) y[k] = fr_load(xb, at);
            }
        }
        // spelled out: with two products per step the compiler declines to unroll this loop, and x, y would leave the registers
        auto step = [&](uint32_t k) {
            if (j0 + k < len) {
                if (has_a) {
                    A = fr_mul(A, x[k]);
                    if (has_b) B = fr_mul(B, x[k]);
                }
                if (has_b) B = fr_add(B, y[k]);
            }
        };
        static_assert(FR_SCAN_CHUNK == 4, "four steps are spelled out");
        step(0); step(1); step(2); step(3);
    }
}
// piece `lane` of the reduce level: the map of its terms to scratch slot pc.slot.  The level runs over the work list of the apply level; a
// piece of a segment that needs no carry (direct) has nothing to reduce.
BN_FN void fr_scan_reduce_body(const FrScanArrays &s, const BnScanPiece *list, size_t lane) {
    const BnScanPiece pc = list[lane];
    if (scan_piece_flag(pc)) return;
    Fr A, B, sa = fr_one();
    const bool per_seg = s.a && (s.flags & FR_SCAN_A_PER_SEGMENT);
    if (per_seg) sa = fr_load(s.a, pc.seg);
    fr_scan_compose(s.a, s.b, sa, per_seg, s.a != nullptr, s.b != nullptr, scan_piece_first(pc), scan_piece_len(pc), (s.flags & FR_SCAN_REVERSE) != 0, A, B);
    if (s.a) fr_store(A, s.map_a, pc.slot);
    if (s.b) fr_store(B, s.map_b, pc.slot);
}
// piece `lane` of an up level: the maps of slots [first, first + len) composed into slot pc.slot.  Slots are in the order of the recurrence
// whatever the direction of the scan.
BN_FN void fr_scan_up_body(const FrScanArrays &s, const BnScanPiece *list, size_t lane) {
    const BnScanPiece pc = list[lane];
    Fr A, B;
    fr_scan_compose(s.map_a, s.map_b, fr_one(), false, s.a != nullptr, s.b != nullptr, scan_piece_first(pc), scan_piece_len(pc), false, A, B);
    if (s.a) fr_store(A, s.map_a, pc.slot);
    if (s.b) fr_store(B, s.map_b, pc.slot);
}
// piece `lane` of a down level: from the value in front of its group - init[pc.seg] at the top of a segment (flag), carry[pc.slot] below -
// through the maps of slots [first, first + len), writing in front of every one the value the recurrence has there
BN_FN void fr_scan_down_body(const FrScanArrays &s, const BnScanPiece *list, size_t lane) {
    const BnScanPiece pc = list[lane];
    const uint64_t first = scan_piece_first(pc);
    const uint32_t len = scan_piece_len(pc);
    Fr cur = scan_piece_flag(pc) ? fr_scan_init(s, pc.seg) : fr_load(s.carry, pc.slot);
#pragma unroll 1
    for (uint32_t j = 0; j < len; ++j) {
        fr_store(cur, s.carry, first + j);
        if (s.a) cur = fr_mul(cur, fr_load(s.map_a, first + j));
        if (s.b) cur = fr_add(cur, fr_load(s.map_b, first + j));
    }
}
// piece `lane` of the apply level: the recurrence over its terms from init[pc.seg] (direct: the piece is its whole segment) or from
// carry[pc.slot].  EXCLUSIVE stores the value before the update.  A lane reads its terms (a chunk at a time) before it writes their outputs and
// no other lane touches them, so out may be a or b.
BN_FN void fr_scan_apply_body(const FrScanArrays &s, const BnScanPiece *list, size_t lane) {
    const BnScanPiece pc = list[lane];
    const uint64_t first = scan_piece_first(pc);
    const uint32_t len = scan_piece_len(pc);
    const bool per_seg = s.a && (s.flags & FR_SCAN_A_PER_SEGMENT), exclusive = (s.flags & FR_SCAN_EXCLUSIVE) != 0;
    Fr cur = scan_piece_flag(pc) ? fr_scan_init(s, pc.seg) : fr_load(s.carry, pc.slot);
    Fr seg_a = fr_one();
    if (per_seg) seg_a = fr_load(s.a, pc.seg);
#pragma unroll 1
    for (uint32_t j0 = 0; j0 < len; j0 += FR_SCAN_CHUNK) {
        Fr x[FR_SCAN_CHUNK], y[FR_SCAN_CHUNK];
#pragma unroll
        for (uint32_t k = 0; k < FR_SCAN_CHUNK; ++k) {
            x[k] = seg_a; y[k] = fr_zero();
            if (j0 + k < len) {
                const uint64_t t = fr_scan_term(s, first, j0 + k);
                if (s.a && !per_seg) x[k] = fr_load(s.a, t);
                if (s.b) y[k] = fr_load(s.b, t);
            }
        }
        auto step = [&](uint32_t k) {                                       // y[k] becomes out[t]; spelled out as in fr_scan_compose
            if (j0 + k < len) {
                const Fr before = cur;
                if (s.a) cur = fr_mul(cur, x[k]);
                if (s.b) cur = fr_add(cur, y[k]);
                y[k] = exclusive ? before : cur;
            }
        };
        step(0); step(1); step(2); step(3);
#pragma unroll
        for (uint32_t k = 0; k < FR_SCAN_CHUNK; ++k)
            if (j0 + k < len) fr_store(y[k], s.out, fr_scan_term(s, first, j0 + k));
    }
}

}  // namespace bn254
