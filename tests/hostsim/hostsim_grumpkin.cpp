// TEST INFRASTRUCTURE - host simulation of bn254_grumpkin_{validate,add,mul,msm}_batch: the bodies of bn_amd/csrc/grumpkin_ops.hpp compiled with g++
// for the CPU - the very code the kernels run, one loop over lanes per launch, over host arrays - and the segmented sum replayed over the work
// list of host_plan.hpp's bn_dot_plan exactly as bn254_grumpkin.hip launches it.  Built with -DBN_BOUNDS (fe.hpp: a violated bound aborts).  Never
// loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // host_plan.hpp reaches the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/grumpkin_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hsg_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
EXPORT int hsg_window() { return GRK_MUL_WINDOW; }
EXPORT unsigned hsg_fan() { return GRK_MSM_FAN; }

// the device forms: sub-launches of at most `step` lanes, each lane through the body; `launches` counts them
template <class Lane>
static int parts(size_t n, size_t step, size_t *launches, Lane lane) {
    *launches = 0;
    if (n == 0) return 0;
    return bn_for_parts(n, step, [&](size_t lo, size_t cnt) -> int { ++*launches; for (size_t i = 0; i < cnt; ++i) lane(lo + i); return 0; });
}
EXPORT int hsg_validate(const uint32_t *p, int32_t *status, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { grk_validate_body(p, status, i); });
}
EXPORT int hsg_add(const uint32_t *p, const uint32_t *q, uint32_t *out, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { grk_add_body(p, q, out, i); });
}
EXPORT int hsg_mul(const uint32_t *p, const uint32_t *k, uint32_t *out, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { grk_mul_body(p, k, out, i); });
}
// ok[i] = the dedicated doubling of p[i] and add(p[i], p[i]) are the same point projectively, at Z = 1 and again one doubling later (Z != 1);
// out[i] = the affine doubling
EXPORT int hsg_double_vs_add(const uint32_t *p, uint32_t *out, int32_t *ok, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const GrkPt a = grk_load_affine(p, i);
        const GrkPt d = grk_double(a), s = grk_add(a, a);
        const GrkPt d2 = grk_double(s), s2 = grk_add(s, s);
        ok[i] = (grk_eq(d, s) ? 1 : 0) | (grk_eq(d2, s2) ? 2 : 0);
        grk_store_affine(d, out, i);
    }
    return 0;
}
// bn254_grumpkin_msm_batch_dev as bn254_grumpkin.hip runs it: the checks, the plan, level 0 and the fold levels as sub-launches of at most `step`
// pieces over a scratch array of plan.slots slots filled with a pattern first.  slots / levels / launches report the plan.
EXPORT int hsg_msm(const uint32_t *p, const uint32_t *k, const size_t *off, size_t m, uint32_t *out, size_t step, size_t *slots, size_t *levels, size_t *launches) {
    *slots = *levels = *launches = 0;
    if (m == 0) return 0;
    const int rc = bn_seg_check(p, k, off, m, out); if (rc) return rc;
    const BnDotPlan plan = bn_dot_plan(off, m, 1, GRK_MSM_FAN);
    std::vector<uint32_t> part(plan.slots * 24 + 8, 0x5a5a5a5au);
    std::vector<uint8_t> written(plan.slots + 1, 0);
    *slots = plan.slots; *levels = plan.levels.size();
    for (size_t l = 0; l < plan.levels.size(); ++l) {
        const BnDotLevel &lv = plan.levels[l];
        const int r = bn_for_parts(lv.count, step, [&](size_t lo, size_t cnt) -> int {
            ++*launches;
            const BnDotPiece *at = plan.pieces.data() + lv.first + lo;
            for (size_t i = 0; i < cnt; ++i) {
                if (!dot_piece_to_out(at[i])) { if (at[i].dst >= plan.slots || written[at[i].dst]++) return BN254_E_INTERNAL; }       // no slot is written twice
                else if (at[i].dst >= m) return BN254_E_INTERNAL;
                if (l) grk_msm_fold_body(at, part.data(), out, i); else grk_msm_piece_body(p, k, at, part.data(), out, i);
            }
            return 0;
        });
        if (r) return r;
    }
    return 0;
}
