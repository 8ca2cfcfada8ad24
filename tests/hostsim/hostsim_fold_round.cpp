// TEST INFRASTRUCTURE - host simulation of bn254_fr_sumcheck_fold_round: the fused body of bn_amd/csrc/mle_ops.hpp and the check, the piece
// length and the level arithmetic of host_plan.hpp (bn_sumcheck_fold_check, bn_sumcheck_fold_piece, bn_sumcheck_plan) compiled with g++ for
// the CPU - the very code the kernel and the entry points run, one loop over lanes per launch, over host arrays, for ANY piece length P and
// fan F.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // mle_ops.hpp and host_plan.hpp reach the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/mle_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT uint32_t hfr_shipped_piece() { return FR_SUMCHECK_FOLD_PIECE; }
EXPORT uint32_t hfr_shipped_fan() { return FR_SUMCHECK_FAN; }
EXPORT size_t hfr_fill(size_t cus) { return bn_sumcheck_fold_fill(cus); }
EXPORT size_t hfr_piece(size_t h2, size_t P, size_t fill) { return bn_sumcheck_fold_piece(h2, P, fill); }
// the argument check alone: nothing is dereferenced beyond the group description
EXPORT int hfr_check(const void *tables, size_t n, size_t k, const void *r, const size_t *off, const uint64_t *group_tables, const bn_fr *coeff, size_t g, int degree, const void *folded,
                     const void *out) {
    BnSumcheckDesc desc;
    return bn_sumcheck_fold_check(tables, n, k, r, off, group_tables, coeff, g, degree, folded, out, &desc);
}
template <int D>
static void fold_round_lanes(const uint32_t *tables, const Fr &r, uint32_t *folded, size_t h2, size_t k, const BnSumcheckDesc &desc, size_t lanes, uint32_t *dst, size_t lo, size_t cnt) {
    for (size_t i = 0; i < cnt; ++i) fr_sumcheck_fold_round_body<D>(tables, r, folded, h2, (uint32_t)k, desc, lanes, dst, lo + i);
}
// The device form (folded may be tables).  The scratch holds exactly plan.slots records, filled with a pattern no value can be.  Every level
// is checked against it before its lanes run (-1: a level reads or writes outside the scratch, -2: it reads a slot no earlier level wrote,
// -3: a slot is written twice).  `launches` gets the sub-launches of the fused kernel and of the sum levels.  A positive return is the
// argument check's answer negated.
EXPORT int hfr_fold_round(const uint32_t *tables, size_t n, size_t k, const bn_fr *r, const size_t *off, const uint64_t *group_tables, const bn_fr *coeff, size_t g, int degree, size_t P,
                          size_t F, size_t step, uint32_t *folded, uint32_t *out, size_t *launches) {
    BnSumcheckDesc desc;
    const int rc = bn_sumcheck_fold_check(tables, n, k, r, off, group_tables, coeff, g, degree, folded, out, &desc); if (rc) return -rc;
    const size_t h2 = n / 4, T = (size_t)degree + 1;
    const BnSumcheckPlan plan = bn_sumcheck_plan(h2, (unsigned)degree, P, F);
    const size_t S = plan.slots;
    std::vector<uint32_t> ws(8 * S + 8, 0xffffffffu);
    std::vector<char> done(S, 0);
    Fr rr;
    memcpy(rr.w, r->l, sizeof rr.w);
    launches[0] = launches[1] = 0;
    if (plan.lanes * P < h2 || (plan.lanes - 1) * P >= h2) return -1;
    if (plan.levels.empty() ? (plan.lanes != 1 || S != 0) : (T * plan.lanes > S)) return -1;
    uint32_t *dst = plan.levels.empty() ? out : ws.data();
    bn_for_parts(plan.lanes, step, [&](size_t lo, size_t cnt) -> int {
        ++launches[0];
        switch (degree) {
        case 1: fold_round_lanes<1>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt); break;
        case 2: fold_round_lanes<2>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt); break;
        case 3: fold_round_lanes<3>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt); break;
        default: fold_round_lanes<4>(tables, rr, folded, h2, k, desc, plan.lanes, dst, lo, cnt); break;
        }
        return 0;
    });
    if (!plan.levels.empty())
        for (size_t i = 0; i < T * plan.lanes; ++i) done[i] = 1;
    size_t expect = plan.lanes;
    for (size_t l = 0; l < plan.levels.size(); ++l) {
        const BnSumcheckLevel &lv = plan.levels[l];
        const size_t cnt2 = (lv.cnt + F - 1) / F;
        if (lv.cnt != expect || lv.lanes != T * cnt2 || lv.src + T * lv.cnt > S || lv.to_out != (cnt2 == 1) || lv.to_out != (l + 1 == plan.levels.size())) return -1;
        for (size_t i = 0; i < T * lv.cnt; ++i)
            if (!done[lv.src + i]) return -2;
        if (!lv.to_out) {
            if (lv.dst + lv.lanes > S) return -1;
            for (size_t i = 0; i < lv.lanes; ++i) { if (done[lv.dst + i]) return -3; done[lv.dst + i] = 1; }
        }
        bn_for_parts(lv.lanes, step, [&](size_t lo, size_t cnt) -> int {
            ++launches[1];
            for (size_t i = 0; i < cnt; ++i) fr_sumcheck_sum_body(ws.data() + 8 * lv.src, lv.cnt, (uint32_t)F, lv.to_out ? out : ws.data() + 8 * lv.dst, lo + i);
            return 0;
        });
        expect = cnt2;
    }
    for (size_t i = 0; i < S; ++i)
        if (!done[i]) return -1;                                            // a slot nothing uses
    return 0;
}
