// TEST INFRASTRUCTURE - host simulation of bn254_fr_dot_batch: the bodies of bn_amd/csrc/dot_ops.hpp and the planner of host_plan.hpp
// (bn_dot_plan) compiled with g++ for the CPU - the very code the kernels and the entry points run, one loop over lanes per launch, over host
// arrays, for ANY piece length P and fan F.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // dot_ops.hpp and host_plan.hpp reach the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/dot_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT uint32_t hsd_shipped_piece() { return FR_DOT_PIECE; }
EXPORT uint32_t hsd_shipped_fan() { return FR_DOT_FAN; }
// the argument checks of the two entry points (with_index_check: the host-buffer form's)
EXPORT int hsd_check(const void *coeff, const uint64_t *index, int has_index, const void *x, size_t nx, const size_t *off, size_t m, const void *out, int with_index_check) {
    int rc = bn_dot_check(coeff, has_index != 0, x, nx, off, m, out);
    if (!rc && with_index_check) rc = bn_dot_check_index(index, off[m], nx);
    return rc;
}
// the plan as plain words: pieces as (first, len, to_out, dst) quadruples, levels as (first, count) pairs.  Returns the number of pieces;
// nothing is written beyond the capacities, so a first call with both at zero sizes the arrays.
EXPORT size_t hsd_plan(const size_t *off, size_t m, size_t P, size_t F, uint64_t *pieces, size_t piece_cap, uint64_t *levels, size_t level_cap, size_t *n_levels, size_t *slots) {
    const BnDotPlan plan = bn_dot_plan(off, m, P, F);
    for (size_t i = 0; i < plan.pieces.size() && i < piece_cap; ++i) {
        const BnDotPiece &p = plan.pieces[i];
        pieces[4 * i] = dot_piece_first(p); pieces[4 * i + 1] = dot_piece_len(p); pieces[4 * i + 2] = dot_piece_to_out(p); pieces[4 * i + 3] = p.dst;
    }
    for (size_t l = 0; l < plan.levels.size() && l < level_cap; ++l) { levels[2 * l] = plan.levels[l].first; levels[2 * l + 1] = plan.levels[l].count; }
    *n_levels = plan.levels.size(); *slots = plan.slots;
    return plan.pieces.size();
}
// the device form: plan, then level after level in sub-launches of at most `step` lanes, each lane through the body.  The scratch holds
// exactly plan.slots records, filled with a pattern no sum can be; every piece is checked against the arrays before its lane runs (-1: a
// piece reads or writes outside them, -2: a fold piece reads a slot no earlier level wrote, -3: a record is written twice).  `launches`
// gets the number of sub-launches of the product level and of the fold levels.  The index is NOT checked: that is the body's business.
EXPORT int hsd_dot(const uint32_t *coeff, const uint64_t *index, const uint32_t *x, uint64_t nx, const size_t *off, size_t m, size_t P, size_t F, size_t step,
                   uint32_t *out, size_t *launches) {
    const BnDotPlan plan = bn_dot_plan(off, m, P, F);
    const size_t n = off[m];
    std::vector<uint32_t> part(plan.slots * 8 + 8, 0xffffffffu);
    std::vector<char> slot_done(plan.slots, 0), slot_now(plan.slots, 0), out_done(m, 0);
    launches[0] = launches[1] = 0;
    for (size_t l = 0; l < plan.levels.size(); ++l) {
        const BnDotLevel &lv = plan.levels[l];
        for (size_t i = 0; i < lv.count; ++i) {
            const BnDotPiece &p = plan.pieces[lv.first + i];
            const uint64_t first = dot_piece_first(p), len = dot_piece_len(p);
            if (first + len > (l ? plan.slots : n) || p.dst >= (dot_piece_to_out(p) ? m : plan.slots)) return -1;
            for (uint64_t j = 0; l && j < len; ++j)
                if (!slot_done[first + j]) return -2;
            char &done = dot_piece_to_out(p) ? out_done[p.dst] : slot_now[p.dst];
            if (done) return -3;
            done = 1;
        }
        const int rc = bn_for_parts(lv.count, step, [&](size_t lo, size_t cnt) -> int {
            const BnDotPiece *list = plan.pieces.data() + lv.first + lo;
            ++launches[l ? 1 : 0];
            for (size_t lane = 0; lane < cnt; ++lane) {
                if (l) fr_dot_fold_body(list, part.data(), out, lane);
                else fr_dot_piece_body(coeff, index, x, nx, list, part.data(), out, lane);
            }
            return 0;
        });
        if (rc) return rc;
        for (size_t k = 0; k < plan.slots; ++k) slot_done[k] |= slot_now[k];
    }
    for (size_t j = 0; j < m; ++j)
        if (!out_done[j]) return -4;
    return 0;
}
