// TEST INFRASTRUCTURE - raw limbs as operands of the leaves of bn_amd/csrc/fe.hpp, with the bounds the caller CLAIMS (-DBN_BOUNDS enforces
// them: a claim the limbs do not meet aborts), and the two double-width leaves on such operands.  Shared by hostsim_wide.cpp (hsw_wmul2 /
// hsw_wred) and hostsim_leaf.cpp (every leaf).  Include after fe.hpp, with BN_HOSTSIM defined.
#pragma once
namespace {
using namespace bn254;
inline Fe fe_raw(const uint32_t *l, unsigned lb, unsigned vb, int sg) {
    Fe r;
    for (int i = 0; i < 9; ++i) r.l[i] = l[i];
    BN_SETB(r, lb, vb);
    BN_IFB(r.sg = sg != 0;)
    (void)lb; (void)vb; (void)sg;
    BN_VERIFY(r, "raw operand");
    return r;
}
inline FeW few_raw(const uint32_t *l, unsigned lb, unsigned wb) {
    FeW r;
    for (int i = 0; i < 18; ++i) r.l[i] = l[i];
    BN_IFB(r.lb = lb; r.wb = wb;)
    (void)lb; (void)wb;
    BN_VERIFYW(r, "raw operand");
    return r;
}

// a*u + c*v on raw limbs -> 18 limbs.  bounds: (lb, vb) of a, u, c, v in this order
static inline void raw_wmul2(int is_signed, const uint32_t *a, const uint32_t *u, const uint32_t *c, const uint32_t *v, const uint32_t *bounds, uint32_t *o) {
    const Fe A = fe_raw(a, bounds[0], bounds[1], is_signed), U = fe_raw(u, bounds[2], bounds[3], is_signed);
    const Fe Cc = fe_raw(c, bounds[4], bounds[5], is_signed), V = fe_raw(v, bounds[6], bounds[7], is_signed);
    const FeW r = is_signed ? fe_wmul2s(A, U, Cc, V) : fe_wmul2(A, U, Cc, V);
    for (int i = 0; i < 18; ++i) o[i] = r.l[i];
}
// reduce(n + [xi] (9 x + s px)) - [sub] d on raw limbs -> 9 limbs.  bounds: (lb, wb) of n, x, px, then (lb, vb) of d
static inline void raw_wred(int xi, int sub, const uint32_t *n, const uint32_t *x, const uint32_t *px, int neg, const uint32_t *d, const uint32_t *bounds, uint32_t *o) {
    const FeW N = few_raw(n, bounds[0], bounds[1]), X = few_raw(x, bounds[2], bounds[3]), PX = few_raw(px, bounds[4], bounds[5]);
    const Fe D = fe_raw(d, bounds[6], bounds[7], 0);
    const Fe r = xi ? (sub ? fe_wred<true, true>(N, X, PX, neg != 0, D) : fe_wred<true, false>(N, X, PX, neg != 0, D))
                    : (sub ? fe_wred<false, true>(N, X, PX, neg != 0, D) : fe_wred<false, false>(N, X, PX, neg != 0, D));
    for (int i = 0; i < 9; ++i) o[i] = r.l[i];
}
}  // namespace
