// TEST INFRASTRUCTURE - the CPU twins of the GPU's inline-asm leaves: every leaf of tests/leafprobe/leaf_list.hpp (the multiplier leaves, the
// double-width leaves and the fused reductions of bn_amd/csrc/fe.hpp) on RAW limbs in, raw limbs out - no conversion to canonical form on either
// side - with the bounds the caller CLAIMS for every operand.  Compiled with -DBN_BOUNDS, so a claim the limbs do not meet, an operand outside a
// leaf's BN_REQUIRE contract, or a result outside the bounds the leaf states aborts the process.  tests/leafprobe/bn254_leafprobe.hip runs the same
// list on the GPU, where the same names are the asm paths.  Never loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "../../bn_amd/csrc/fe.hpp"
#include "rawleaf.hpp"                     // fe_raw / few_raw, raw_wmul2 / raw_wred (shared with hostsim_wide.cpp)

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

// operand offsets (in limbs) of a kinds string: 'f' = 9 limbs, 'w' = 18
struct Kinds {
    int n = 0, stride = 0, off[12] = {};
    constexpr Kinds(const char *s) {
        for (; s[n]; ++n) { off[n] = stride; stride += s[n] == 'w' ? 18 : 9; }
    }
};
static void st(uint32_t *o, const Fe &r) { for (int i = 0; i < 9; ++i) o[i] = r.l[i]; }
static void st(uint32_t *o, const FeW &r) { for (int i = 0; i < 18; ++i) o[i] = r.l[i]; }

EXPORT int hsl_bounds_enabled() {
#ifdef BN_BOUNDS
    return 1;
#else
    return 0;
#endif
}
EXPORT int hsl_leaf_count() {
#define LEAF(...)
#define LEAF_HOST(...)
#include "../leafprobe/leaf_list.hpp"
#undef LEAF
#undef LEAF_HOST
    return LEAF_COUNT;
}
// "name:kinds:output limbs" of a leaf, for the check against tests/leaf_cases.py
EXPORT const char *hsl_leaf_info(int leaf) {
    switch (leaf) {
#define LEAF(ID, NAME, OUTW, KINDS, ...) case ID: return #NAME ":" KINDS ":" #OUTW;
#define LEAF_HOST(ID, NAME, OUTW, KINDS, STMT, ...) case ID: return #NAME ":" KINDS ":" #OUTW;
#include "../leafprobe/leaf_list.hpp"
#undef LEAF
#undef LEAF_HOST
    default: return "";
    }
}
// n cases of one leaf.  ops: the operands' limbs, case after case (operands in order, 9 or 18 limbs each);  bounds: per case and operand three
// words - (lb, vb, signed) of an Fe, (lb, wb, 0) of an FeW;  flags: the per-case boolean;  out: 9 or 18 limbs per case.  Returns 0, or -1 for an unknown leaf.
EXPORT int hsl_run(int leaf, int n, const uint32_t *ops, const uint32_t *bounds, const int32_t *flags, uint32_t *out) {
#define P(i) (p + K.off[i])
#define F(i) fe_raw(P(i), b[3 * (i)], b[3 * (i) + 1], (int)b[3 * (i) + 2])
#define W(i) few_raw(P(i), b[3 * (i)], b[3 * (i) + 1])
#define FLAG (flags[t] != 0)
#define B2 b2
#define O o
#define LEAF(ID, NAME, OUTW, KINDS, ...)                                                                  \
    case ID: {                                                                                            \
        constexpr Kinds K(KINDS);                                                                         \
        for (int t = 0; t < n; ++t) {                                                                     \
            const uint32_t *p = ops + (size_t)t * K.stride, *b = bounds + (size_t)t * 3 * K.n;            \
            st(out + (size_t)t * OUTW, __VA_ARGS__);                                                      \
        }                                                                                                 \
        return 0;                                                                                         \
    }
    // the double-width leaves go through the raw-limb calls hostsim_wide.cpp exports, which take (lb, vb) pairs
#define LEAF_HOST(ID, NAME, OUTW, KINDS, STMT, ...)                                                       \
    case ID: {                                                                                            \
        constexpr Kinds K(KINDS);                                                                         \
        for (int t = 0; t < n; ++t) {                                                                     \
            const uint32_t *p = ops + (size_t)t * K.stride, *b = bounds + (size_t)t * 3 * K.n;            \
            uint32_t b2[8], *o = out + (size_t)t * OUTW;                                                  \
            for (int j = 0; j < 4; ++j) { b2[2 * j] = b[3 * j]; b2[2 * j + 1] = b[3 * j + 1]; }           \
            STMT;                                                                                         \
        }                                                                                                 \
        return 0;                                                                                         \
    }
    switch (leaf) {
#include "../leafprobe/leaf_list.hpp"
    default: return -1;
    }
}
