// TEST INFRASTRUCTURE - host simulation of bn254_fr_sqrt_batch, bn254_bjj_{pack,unpack}_batch and bn254_eddsa_poseidon_verify_packed_batch: the
// bodies of bn_amd/csrc/fr_sqrt_ops.hpp and babyjub_ops.hpp compiled with g++ for the CPU - the very code the kernels run, one loop over lanes
// per launch, over host arrays.  Built with -DBN_BOUNDS (fe.hpp: a violated bound aborts).  Both forms of the square root are in the library
// whichever one ships.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // host_plan.hpp reaches the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/babyjub_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hsp_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
EXPORT int hsp_shipped_form() { return BN254_FR_SQRT_FORM; }

// the device forms: sub-launches of at most `step` lanes, each lane through the body; `launches` counts them
template <class Lane>
static int parts(size_t n, size_t step, size_t *launches, Lane lane) {
    *launches = 0;
    if (n == 0) return 0;
    return bn_for_parts(n, step, [&](size_t lo, size_t cnt) -> int { ++*launches; for (size_t i = 0; i < cnt; ++i) lane(lo + i); return 0; });
}
// ok may be NULL, out may be a
EXPORT int hsp_sqrt(int form, const uint32_t *a, uint32_t *out, int32_t *ok, size_t n, size_t step, size_t *launches) {
    if (form != 0 && form != 1) return BN254_E_BAD_ARG;
    return parts(n, step, launches, [&](size_t i) { if (form == 0) fr_sqrt_body<0>(a, out, ok, i); else fr_sqrt_body<1>(a, out, ok, i); });
}
// root and flag of u / v
EXPORT int hsp_sqrt_ratio(int form, const uint32_t *u, const uint32_t *v, uint32_t *out, int32_t *ok, size_t n) {
    if (form != 0 && form != 1) return BN254_E_BAD_ARG;
    for (size_t i = 0; i < n; ++i) {
        FrSqrt r;
        if (form == 0) fr_sqrt_ratio<0>(fr_load(u, i), fr_load(v, i), r); else fr_sqrt_ratio<1>(fr_load(u, i), fr_load(v, i), r);
        fr_store(r.root, out, i);
        ok[i] = r.is_square ? 1 : 0;
    }
    return 0;
}
EXPORT int hsp_pack(const uint32_t *p, uint32_t *out32, size_t n, size_t step, size_t *launches) {
    return parts(n, step, launches, [&](size_t i) { bjj_pack_body(p, out32, i); });
}
EXPORT int hsp_unpack(int form, const uint32_t *in32, uint32_t *out, int32_t *status, size_t n, size_t step, size_t *launches) {
    if (form != 0 && form != 1) return BN254_E_BAD_ARG;
    return parts(n, step, launches, [&](size_t i) { if (form == 0) bjj_unpack_body<0>(in32, out, status, i); else bjj_unpack_body<1>(in32, out, status, i); });
}
EXPORT int hsp_verify_packed(int form, const uint32_t *a32, const uint32_t *sig64, const uint32_t *msg, int32_t *status, size_t n, size_t step, size_t *launches) {
    if (form != 0 && form != 1) return BN254_E_BAD_ARG;
    return parts(n, step, launches, [&](size_t i) {
        if (form == 0) eddsa_verify_packed_body<BN254_EDDSA_WINDOW, 0>(a32, sig64, msg, status, i);
        else eddsa_verify_packed_body<BN254_EDDSA_WINDOW, 1>(a32, sig64, msg, status, i);
    });
}
