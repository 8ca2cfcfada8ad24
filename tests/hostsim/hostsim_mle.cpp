// TEST INFRASTRUCTURE - host simulation of bn254_fr_mle_eq, bn254_fr_mle_fold and bn254_fr_sumcheck_round: the bodies of bn_amd/csrc/mle_ops.hpp and
// the checks and level arithmetic of host_plan.hpp (bn_sumcheck_check, bn_sumcheck_plan) compiled with g++ for the CPU - the very code the
// kernels and the entry points run, one loop over lanes per launch, over host arrays, for ANY piece length P and fan F.  Never loaded by the
// product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // mle_ops.hpp and host_plan.hpp reach the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/mle_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT uint32_t hsm_shipped_piece() { return FR_SUMCHECK_PIECE; }
EXPORT uint32_t hsm_shipped_fan() { return FR_SUMCHECK_FAN; }
// the plan as plain words: levels as (cnt, lanes, src, dst, to_out) rows.  Returns the number of levels; nothing is written beyond the capacity.
EXPORT size_t hsm_plan(size_t h, unsigned degree, size_t P, size_t F, uint64_t *levels, size_t level_cap, size_t *lanes, size_t *slots) {
    const BnSumcheckPlan plan = bn_sumcheck_plan(h, degree, P, F);
    for (size_t l = 0; l < plan.levels.size() && l < level_cap; ++l) {
        const BnSumcheckLevel &lv = plan.levels[l];
        levels[5 * l] = lv.cnt; levels[5 * l + 1] = lv.lanes; levels[5 * l + 2] = lv.src; levels[5 * l + 3] = lv.dst; levels[5 * l + 4] = lv.to_out;
    }
    *lanes = plan.lanes; *slots = plan.slots;
    return plan.levels.size();
}
// the device forms: sub-launches of at most `step` lanes, each lane through the body; `launches` counts them
EXPORT int hsm_eq(const uint32_t *z, int nv, size_t step, uint32_t *out, size_t *launches) {
    const int rc = bn_mle_eq_check(z, nv, out); if (rc) return rc;
    *launches = 0;
    return bn_for_parts((size_t)1 << nv, step, [&](size_t lo, size_t cnt) -> int {
        ++*launches;
        for (size_t i = 0; i < cnt; ++i) fr_mle_eq_body(z, (uint32_t)nv, out, lo + i);
        return 0;
    });
}
// out may be in
EXPORT int hsm_fold(const uint32_t *in, size_t len, const bn_fr *r, size_t step, uint32_t *out, size_t *launches) {
    *launches = 0;
    if (len == 0) return 0;
    const int rc = bn_mle_fold_check(in, len, r, out); if (rc) return rc;
    Fr rr;
    memcpy(rr.w, r->l, sizeof rr.w);
    return bn_for_parts(len / 2, step, [&](size_t lo, size_t cnt) -> int {
        ++*launches;
        for (size_t i = 0; i < cnt; ++i) fr_mle_fold_body(in, rr, out, len / 2, lo + i);
        return 0;
    });
}
template <int D>
static void round_lanes(const uint32_t *tables, size_t h, size_t k, const BnSumcheckDesc &desc, size_t lanes, uint32_t *dst, size_t lo, size_t cnt) {
    for (size_t i = 0; i < cnt; ++i) fr_sumcheck_round_body<D>(tables, h, (uint32_t)k, desc, lanes, dst, lo + i);
}
// The scratch holds exactly plan.slots records, filled with a pattern no value can be.  Every level is checked against it before its
// lanes run (-1: a level reads or writes outside the scratch, -2: it reads a slot no earlier level wrote, -3: a slot is written twice).
// `launches` gets the sub-launches of the round kernel and of the sum levels.  A positive return is the argument check's answer negated.
EXPORT int hsm_round(const uint32_t *tables, size_t n, size_t k, const size_t *off, const uint64_t *group_tables, const bn_fr *coeff, size_t g, int degree, size_t P, size_t F,
                     size_t step, uint32_t *out, size_t *launches) {
    BnSumcheckDesc desc;
    const int rc = bn_sumcheck_check(tables, n, k, off, group_tables, coeff, g, degree, out, &desc); if (rc) return -rc;
    const size_t h = n / 2, T = (size_t)degree + 1;
    const BnSumcheckPlan plan = bn_sumcheck_plan(h, (unsigned)degree, P, F);
    const size_t S = plan.slots;
    std::vector<uint32_t> ws(8 * S + 8, 0xffffffffu);
    std::vector<char> done(S, 0);
    launches[0] = launches[1] = 0;
    if (plan.lanes * P < h || (plan.lanes - 1) * P >= h) return -1;
    if (plan.levels.empty() ? (plan.lanes != 1 || S != 0) : (T * plan.lanes > S)) return -1;
    uint32_t *dst = plan.levels.empty() ? out : ws.data();
    bn_for_parts(plan.lanes, step, [&](size_t lo, size_t cnt) -> int {
        ++launches[0];
        switch (degree) {
        case 1: round_lanes<1>(tables, h, k, desc, plan.lanes, dst, lo, cnt); break;
        case 2: round_lanes<2>(tables, h, k, desc, plan.lanes, dst, lo, cnt); break;
        case 3: round_lanes<3>(tables, h, k, desc, plan.lanes, dst, lo, cnt); break;
        default: round_lanes<4>(tables, h, k, desc, plan.lanes, dst, lo, cnt); break;
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
