// TEST INFRASTRUCTURE - host simulation of bn254_fr_scan_batch: the bodies of bn_amd/csrc/scan_ops.hpp and the planner of host_plan.hpp
// (bn_scan_plan) compiled with g++ for the CPU - the very code the kernels and the entry points run, one loop over lanes per launch, over host
// arrays, for ANY piece length P and fan F.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // scan_ops.hpp and host_plan.hpp reach the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/scan_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT uint32_t hss_shipped_piece() { return FR_SCAN_PIECE; }
EXPORT uint32_t hss_shipped_fan() { return FR_SCAN_FAN; }
// the argument checks of the two entry points
EXPORT int hss_check(const void *a, const void *b, const size_t *off, size_t m, unsigned flags, const void *out) { return bn_scan_check(a, b, off, m, flags, out); }
// the plan as plain words: pieces as (first, len, flag, seg, slot) rows, levels as (kind, first, count) rows.  Returns the number of pieces;
// nothing is written beyond the capacities, so a first call with both at zero sizes the arrays.
EXPORT size_t hss_plan(const size_t *off, size_t m, size_t P, size_t F, int reverse, uint64_t *pieces, size_t piece_cap, uint64_t *levels, size_t level_cap, size_t *n_levels,
                       size_t *slots) {
    const BnScanPlan plan = bn_scan_plan(off, m, P, F, reverse != 0);
    for (size_t i = 0; i < plan.pieces.size() && i < piece_cap; ++i) {
        const BnScanPiece &p = plan.pieces[i];
        pieces[5 * i] = scan_piece_first(p); pieces[5 * i + 1] = scan_piece_len(p); pieces[5 * i + 2] = scan_piece_flag(p); pieces[5 * i + 3] = p.seg; pieces[5 * i + 4] = p.slot;
    }
    for (size_t l = 0; l < plan.levels.size() && l < level_cap; ++l) {
        levels[3 * l] = plan.levels[l].kind; levels[3 * l + 1] = plan.levels[l].first; levels[3 * l + 2] = plan.levels[l].count;
    }
    *n_levels = plan.levels.size(); *slots = plan.slots;
    return plan.pieces.size();
}
// the device form: plan, then level after level in sub-launches of at most `step` lanes, each lane through the body.  The scratch holds
// exactly plan.slots records per array, filled with a pattern no value can be; every piece is checked against the arrays before its lane
// runs (-1: a piece reads or writes outside its segment or the scratch, -2: it reads a map or a carry no earlier level wrote, -3: a map, a
// carry or a term is written twice, -4: a term is never written).  `launches` gets the sub-launches per kind (reduce, up, down, apply).
// out may be a or b.
EXPORT int hss_scan(const uint32_t *a, const uint32_t *b, const uint32_t *init, const size_t *off, size_t m, unsigned flags, size_t P, size_t F, size_t step, uint32_t *out,
                    size_t *launches) {
    const bool reverse = (flags & BN254_SCAN_REVERSE) != 0;
    const BnScanPlan plan = bn_scan_plan(off, m, P, F, reverse);
    const size_t n = off[m], S = plan.slots;
    std::vector<uint32_t> ws(3 * S * 8 + 8, 0xffffffffu);
    std::vector<char> map_done(S, 0), map_now(S, 0), carry_done(S, 0), carry_now(S, 0), term_done(n, 0);
    const FrScanArrays arr = {a, b, init, ws.data(), ws.data() + 8 * S, ws.data() + 16 * S, out, flags};
    for (int k = 0; k < 4; ++k) launches[k] = 0;
    for (const BnScanLevel &lv : plan.levels) {
        for (size_t i = 0; i < lv.count; ++i) {
            const BnScanPiece &p = plan.pieces[lv.first + i];
            const uint64_t first = scan_piece_first(p), len = scan_piece_len(p);
            const bool flag = scan_piece_flag(p);
            if (lv.kind == BN_SCAN_REDUCE || lv.kind == BN_SCAN_APPLY) {
                if (p.seg >= m || len == 0 || len > P) return -1;
                const uint64_t lo = reverse ? first + 1 - len : first, hi = reverse ? first + 1 : first + len;
                if ((reverse && first + 1 < len) || lo < off[p.seg] || hi > off[p.seg + 1]) return -1;
                if (!flag && p.slot >= S) return -1;
                if (lv.kind == BN_SCAN_REDUCE) {
                    if (flag) continue;
                    if (map_now[p.slot] || map_done[p.slot]) return -3;
                    map_now[p.slot] = 1;
                } else {
                    if (!flag && !carry_done[p.slot]) return -2;
                    for (uint64_t t = lo; t < hi; ++t) { if (term_done[t]) return -3; term_done[t] = 1; }
                }
            } else {
                if (len == 0 || len > F || first + len > S) return -1;
                for (uint64_t j = 0; j < len; ++j)
                    if (!map_done[first + j]) return -2;
                if (lv.kind == BN_SCAN_UP) {
                    if (p.slot >= S) return -1;
                    if (map_now[p.slot] || map_done[p.slot]) return -3;
                    map_now[p.slot] = 1;
                } else {
                    if (flag ? p.seg >= m : p.slot >= S) return -1;
                    if (!flag && !carry_done[p.slot]) return -2;
                    for (uint64_t j = 0; j < len; ++j) { if (carry_now[first + j] || carry_done[first + j]) return -3; carry_now[first + j] = 1; }
                }
            }
        }
        const int rc = bn_for_parts(lv.count, step, [&](size_t lo, size_t cnt) -> int {
            const BnScanPiece *list = plan.pieces.data() + lv.first + lo;
            ++launches[lv.kind];
            for (size_t lane = 0; lane < cnt; ++lane) {
                if (lv.kind == BN_SCAN_REDUCE) fr_scan_reduce_body(arr, list, lane);
                else if (lv.kind == BN_SCAN_UP) fr_scan_up_body(arr, list, lane);
                else if (lv.kind == BN_SCAN_DOWN) fr_scan_down_body(arr, list, lane);
                else fr_scan_apply_body(arr, list, lane);
            }
            return 0;
        });
        if (rc) return rc;
        for (size_t k = 0; k < S; ++k) { map_done[k] |= map_now[k]; carry_done[k] |= carry_now[k]; }
    }
    for (size_t t = 0; t < n; ++t)
        if (!term_done[t]) return -4;
    return 0;
}
