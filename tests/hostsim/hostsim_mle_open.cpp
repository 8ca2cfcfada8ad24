// TEST INFRASTRUCTURE - host simulation of bn254_fr_mle_quotients: the body of bn_amd/csrc/mle_ops.hpp (fr_mle_quotients_body) and the check and
// the passes of host_plan.hpp (bn_mle_quotients_check, bn_mle_quotients_plan) compiled with g++ for the CPU, bounds of fr.hpp enforced - the
// very code the kernel and the entry points run, one loop over lanes per sub-launch, over host arrays, for ANY number of levels per pass.
// Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // mle_ops.hpp and host_plan.hpp reach the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/mle_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT uint32_t hso_shipped_levels() { return FR_MLE_QUOT_LEVELS; }
EXPORT uint32_t hso_levels_max() { return FR_MLE_QUOT_LEVELS_MAX; }
EXPORT int hso_check(const void *a, int nv, const void *z, const void *out) { return bn_mle_quotients_check(a, nv, z, out); }
// the plan as plain words: passes as (levels, vars, lanes, first, last) rows.  Returns the number of passes; nothing is written beyond the capacity.
EXPORT size_t hso_plan(unsigned nv, unsigned rho, uint64_t *rows, size_t cap, size_t *slots) {
    const BnMleQuotPlan plan = bn_mle_quotients_plan(nv, rho);
    for (size_t p = 0; p < plan.passes.size() && p < cap; ++p) {
        const BnMleQuotPass &ps = plan.passes[p];
        rows[5 * p] = ps.levels; rows[5 * p + 1] = ps.vars; rows[5 * p + 2] = ps.lanes; rows[5 * p + 3] = ps.first; rows[5 * p + 4] = ps.last;
    }
    *slots = plan.slots;
    return plan.passes.size();
}
template <int RHO>
static void quot_lanes(const uint32_t *src, const bn_fr *z, unsigned m, uint32_t *fold_dst, uint32_t *out, size_t lo, size_t cnt) {
    Fr zz[RHO];
    for (int k = 0; k < RHO; ++k) memcpy(zz[k].w, z[m - 1 - k].l, sizeof zz[k].w);
    for (size_t i = 0; i < cnt; ++i) fr_mle_quotients_body<RHO>(src, zz, m, fold_dst, out, lo + i);
}
// The device form: the passes of the plan, each as sub-launches of at most `step` lanes.  The scratch holds exactly plan.slots records, and a
// and out exactly 2^nv.  Every pass is checked before its lanes run (-1: its shape is not the plan's contract or it would touch a record
// outside the scratch); `launches` counts the sub-launches.  A positive return is the argument check's answer negated.
EXPORT int hso_quotients(const uint32_t *a, int nv, const bn_fr *z, unsigned rho, size_t step, uint32_t *out, size_t *launches) {
    const int rc = bn_mle_quotients_check(a, nv, z, out); if (rc) return -rc;
    *launches = 0;
    if (nv == 0) { memcpy(out, a, sizeof(bn_fr)); return 0; }
    if (rho < 1 || rho > FR_MLE_QUOT_LEVELS_MAX) return -1;
    const BnMleQuotPlan plan = bn_mle_quotients_plan((unsigned)nv, rho);
    std::vector<uint32_t> ws(8 * plan.slots, 0xffffffffu);
    unsigned vars = (unsigned)nv;
    for (size_t p = 0; p < plan.passes.size(); ++p) {
        const BnMleQuotPass &ps = plan.passes[p];
        if (ps.vars != vars || ps.levels < 1 || ps.levels > rho || ps.levels > vars || ps.lanes != (size_t)1 << (vars - ps.levels)) return -1;
        if (ps.first != (p == 0) || ps.last != (p + 1 == plan.passes.size()) || ps.last != (ps.levels == vars)) return -1;
        if (!ps.first && ((size_t)1 << vars) > plan.slots) return -1;           // reads the scratch
        if (!ps.last && ps.lanes > plan.slots) return -1;                       // writes it
        const uint32_t *src = ps.first ? a : ws.data();
        uint32_t *fold_dst = ps.last ? out : ws.data();
        bn_for_parts(ps.lanes, step, [&](size_t lo, size_t cnt) -> int {
            ++*launches;
            switch (ps.levels) {
            case 1: quot_lanes<1>(src, z, vars, fold_dst, out, lo, cnt); break;
            case 2: quot_lanes<2>(src, z, vars, fold_dst, out, lo, cnt); break;
            case 3: quot_lanes<3>(src, z, vars, fold_dst, out, lo, cnt); break;
            default: quot_lanes<4>(src, z, vars, fold_dst, out, lo, cnt); break;
            }
            return 0;
        });
        vars -= ps.levels;
    }
    return vars == 0 ? 0 : -1;
}
