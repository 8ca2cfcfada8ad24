// TEST INFRASTRUCTURE - host simulation of the lazily reduced tower products: the two double-width leaves of bn_amd/csrc/fe.hpp (fe_wmul2 /
// fe_wmul2s, fe_wred) on raw limbs with the bounds the caller CLAIMS (-DBN_BOUNDS enforces them: a claim the limbs do not meet aborts), and
// f6_mul_lazy / f12_mul / f12_sqr of tower.hpp on a simulated lane pair, next to their generic (WIDE = false) forms, and on TWO lane pairs
// side by side (lanequad.hpp's four-lane value type: lanes 0-1 are the even slot of a batch, lanes 2-3 the odd one, each with its own element).
// Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"
#include "lanequad.hpp"                    // two lane pairs side by side: the even and the odd SLOT of a batch
#include "../../bn_amd/csrc/io.hpp"
#include "rawleaf.hpp"                     // fe_raw / few_raw and the two wide leaves on raw limbs

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))
typedef Fq2B<FeP> F2B;

EXPORT int hsw_bounds_enabled() {
#ifdef BN_BOUNDS
    return 1;
#else
    return 0;
#endif
}
// a*u + c*v on raw limbs -> 18 limbs.  bounds: (lb, vb) of a, u, c, v in this order  (rawleaf.hpp, shared with hostsim_leaf.cpp)
EXPORT void hsw_wmul2(int is_signed, const uint32_t *a, const uint32_t *u, const uint32_t *c, const uint32_t *v, const uint32_t *bounds, uint32_t *o) { raw_wmul2(is_signed, a, u, c, v, bounds, o); }
// reduce(n + [xi] (9 x + s px)) - [sub] d on raw limbs -> 9 limbs.  bounds: (lb, wb) of n, x, px, then (lb, vb) of d
EXPORT void hsw_wred(int xi, int sub, const uint32_t *n, const uint32_t *x, const uint32_t *px, int neg, const uint32_t *d, const uint32_t *bounds, uint32_t *o) { raw_wred(xi, sub, n, x, px, neg, d, bounds, o); }
// wide values of the limb-wise sums the tower forms: o = x + y
EXPORT void hsw_wadd(const uint32_t *x, const uint32_t *y, const uint32_t *bounds, uint32_t *o) {
    const FeW r = fe_wadd(few_raw(x, bounds[0], bounds[1]), few_raw(y, bounds[2], bounds[3]));
    for (int i = 0; i < 18; ++i) o[i] = r.l[i];
}

// the tower on a simulated lane pair.  An Fq6 travels as the c0 half of an Fq12 record (the c1 half is ignored / written as zero).
EXPORT void hsw_fq6_mul(int wide, const uint32_t *a, const uint32_t *b, uint32_t *o) {
    const Fq12<F2B> x = f12_load<F2B>(a), y = f12_load<F2B>(b);
    Fq12<F2B> r = {wide ? f6_mul_lazy(x.c0, y.c0) : f6_mul(x.c0, y.c0), f6_zero<F2B>()};
    f12_store(r, o);
}
// a*b - d, the subtrahend inside the reductions (the cross term of f12_mul and f12_sqr)
EXPORT void hsw_fq6_mul_sub(const uint32_t *a, const uint32_t *b, const uint32_t *d, uint32_t *o) {
    const Fq12<F2B> x = f12_load<F2B>(a), y = f12_load<F2B>(b), z = f12_load<F2B>(d);
    Fq12<F2B> r = {f6_mul_lazy<true>(x.c0, y.c0, z.c0), f6_zero<F2B>()};
    f12_store(r, o);
}
EXPORT void hsw_fq12_mul(int wide, int conj, const uint32_t *a, const uint32_t *b, uint32_t *o) {
    const Fq12<F2B> x = f12_load<F2B>(a), y = f12_load<F2B>(b);
    f12_store(wide ? f12_mul_src<true>(x, Fq12Ref<F2B>{y}, conj != 0) : f12_mul_src<false>(x, Fq12Ref<F2B>{y}, conj != 0), o);
}
EXPORT void hsw_fq12_sqr(int wide, int reduced_c1, const uint32_t *a, uint32_t *o) {
    const Fq12<F2B> x = f12_load<F2B>(a);
    Fq12<F2B> r;
    if (wide) r = reduced_c1 ? f12_sqr<true, true>(x) : f12_sqr<false, true>(x);
    else r = reduced_c1 ? f12_sqr<true, false>(x) : f12_sqr<false, false>(x);
    f12_store(r, o);
}
// chains: every output feeds the next operation in the form it was returned in (the bounds of one step meet the requirements of the next)
EXPORT void hsw_fq12_sqr_chain(int reduced_c1, int n, const uint32_t *a, uint32_t *o) {
    Fq12<F2B> x = f12_load<F2B>(a);
    for (int i = 0; i < n; ++i) x = reduced_c1 ? f12_sqr<true>(x) : f12_mul(f12_sqr<false>(x), x);
    f12_store(x, o);
}
EXPORT void hsw_counts(int what, const uint32_t *a, const uint32_t *b, unsigned long *macs) {
    const Fq12<F2B> x = f12_load<F2B>(a), y = f12_load<F2B>(b);
#if defined(BN_BOUNDS)
    op_counts() = OpCounts{};
    Fq12<F2B> r;
    switch (what) {
    case 0: r.c0 = f6_mul_lazy(x.c0, y.c0); break;
    case 1: r.c0 = f6_mul(x.c0, y.c0); break;
    case 2: r = f12_mul_src<true>(x, Fq12Ref<F2B>{y}, false); break;
    case 3: r = f12_mul_src<false>(x, Fq12Ref<F2B>{y}, false); break;
    case 4: r = f12_sqr<false, true>(x); break;
    default: r = f12_sqr<false, false>(x); break;
    }
    *macs = op_counts().macs / 2;          // per lane
    (void)r;
#else
    (void)x; (void)y; *macs = 0;
#endif
}

// ---- two lane pairs side by side: slot 0 (lanes 0, 1) and slot 1 (lanes 2, 3) each hold their own element, as adjacent pairings of a batch do
typedef Fq2B<FeQ> F2S;
static F2S slots2(const F2B &even, const F2B &odd) { return {{{even.v, odd.v}}}; }
static Fq6<F2S> slots6(const Fq6<F2B> &e, const Fq6<F2B> &o) { return {slots2(e.c0, o.c0), slots2(e.c1, o.c1), slots2(e.c2, o.c2)}; }
static Fq12<F2S> slots12(const Fq12<F2B> &e, const Fq12<F2B> &o) { return {slots6(e.c0, o.c0), slots6(e.c1, o.c1)}; }
static Fq6<F2B> slot6(const Fq6<F2S> &x, int i) { return {{x.c0.v.p[i]}, {x.c1.v.p[i]}, {x.c2.v.p[i]}}; }
static Fq12<F2B> slot12(const Fq12<F2S> &x, int i) { return {slot6(x.c0, i), slot6(x.c1, i)}; }
// (a_even * b_even, a_odd * b_odd) computed in ONE call
EXPORT void hsw_fq12_mul_slots(const uint32_t *ae, const uint32_t *be, const uint32_t *ao, const uint32_t *bo, uint32_t *oe, uint32_t *oo) {
    const Fq12<F2S> a = slots12(f12_load<F2B>(ae), f12_load<F2B>(ao)), b = slots12(f12_load<F2B>(be), f12_load<F2B>(bo));
    const Fq12<F2S> r = f12_mul_src<true>(a, Fq12Ref<F2S>{b}, false);
    f12_store(slot12(r, 0), oe); f12_store(slot12(r, 1), oo);
}
EXPORT void hsw_fq12_sqr_slots(int reduced_c1, const uint32_t *ae, const uint32_t *ao, uint32_t *oe, uint32_t *oo) {
    const Fq12<F2S> a = slots12(f12_load<F2B>(ae), f12_load<F2B>(ao));
    const Fq12<F2S> r = reduced_c1 ? f12_sqr<true, true>(a) : f12_sqr<false, true>(a);
    f12_store(slot12(r, 0), oe); f12_store(slot12(r, 1), oo);
}
EXPORT void hsw_fq6_mul_slots(const uint32_t *ae, const uint32_t *be, const uint32_t *ao, const uint32_t *bo, uint32_t *oe, uint32_t *oo) {
    const Fq12<F2S> a = slots12(f12_load<F2B>(ae), f12_load<F2B>(ao)), b = slots12(f12_load<F2B>(be), f12_load<F2B>(bo));
    const Fq6<F2S> r = f6_mul_lazy(a.c0, b.c0);
    f12_store(Fq12<F2B>{slot6(r, 0), f6_zero<F2B>()}, oe); f12_store(Fq12<F2B>{slot6(r, 1), f6_zero<F2B>()}, oo);
}
