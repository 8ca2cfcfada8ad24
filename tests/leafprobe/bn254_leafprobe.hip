// TEST INFRASTRUCTURE - the GPU probe of the field leaves: one kernel per entry of leaf_list.hpp, one CASE per lane.  A lane loads the raw limbs
// of its operands from global memory, calls the leaf by its public name - on the GPU the inline-asm path of fe_asm.hpp / BN_LC_CHAIN - and writes
// the raw limbs of the result.  No conversion on either side, no asm of its own, nothing beyond fe.hpp.  tests/test_gpu_leaf.py compares the
// output with the bounds-checked CPU twins (tests/hostsim/hostsim_leaf.cpp) limb for limb.
// This source is compiled TWICE into one library (tests/leafprobe.py): with BN_INLINE_ALL, the forced-inline form of the pairing kernels
// (prefix lpi_ / bnlp_inl_), and without it, where the leaves are real functions whose operands travel by the calling convention (lpf_ / bnlp_fn_).
// Never loaded by the product (bn_amd/) and adds no symbol to it.
#include "fe.hpp"

using namespace bn254;

#ifdef BN_INLINE_ALL
#define LP_K(NAME) lpi_##NAME
#define LP_SYM(NAME) bnlp_inl_##NAME
#else
#define LP_K(NAME) lpf_##NAME
#define LP_SYM(NAME) bnlp_fn_##NAME
#endif

namespace {
// operand offsets (in limbs) of a kinds string: 'f' = 9 limbs, 'w' = 18
struct Kinds {
    int n = 0, stride = 0, off[12] = {};
    constexpr Kinds(const char *s) {
        for (; s[n]; ++n) { off[n] = stride; stride += s[n] == 'w' ? 18 : 9; }
    }
};
BN_FN Fe ld_fe(const uint32_t *p) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = p[i];
    return r;
}
BN_FN FeW ld_few(const uint32_t *p) {
    FeW r;
#pragma unroll
    for (int i = 0; i < 18; ++i) r.l[i] = p[i];
    return r;
}
BN_FN void st(uint32_t *o, const Fe &r) {
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = r.l[i];
}
BN_FN void st(uint32_t *o, const FeW &r) {
#pragma unroll
    for (int i = 0; i < 18; ++i) o[i] = r.l[i];
}
}  // namespace

#define F(i) ld_fe(p + K.off[i])
#define W(i) ld_few(p + K.off[i])
#define FLAG flag
// lanes at or beyond n return before they touch memory; every index is the lane's own case
#define LEAF(ID, NAME, OUTW, KINDS, ...)                                                                              \
    __global__ void __launch_bounds__(64) LP_K(NAME)(const uint32_t *ops, const int32_t *flags, uint32_t *out, uint32_t n) { \
        const uint32_t t = blockIdx.x * 64u + threadIdx.x;                                                           \
        if (t >= n) return;                                                                                           \
        constexpr Kinds K(KINDS);                                                                                     \
        const uint32_t *p = ops + (size_t)t * K.stride;                                                               \
        const bool flag = flags[t] != 0;                                                                              \
        (void)flag;                                                                                                   \
        st(out + (size_t)t * OUTW, __VA_ARGS__);                                                                      \
    }
#define LEAF_HOST(ID, NAME, OUTW, KINDS, STMT, ...) LEAF(ID, NAME, OUTW, KINDS, __VA_ARGS__)
#include "leaf_list.hpp"
#undef LEAF
#undef LEAF_HOST

extern "C" {
__attribute__((visibility("default"))) int LP_SYM(leaf_count)() { return LEAF_COUNT; }
// "name:kinds:output limbs" of a leaf
__attribute__((visibility("default"))) const char *LP_SYM(leaf_info)(int leaf) {
    switch (leaf) {
#define LEAF(ID, NAME, OUTW, KINDS, ...) case ID: return #NAME ":" KINDS ":" #OUTW;
#define LEAF_HOST(ID, NAME, OUTW, KINDS, STMT, ...) case ID: return #NAME ":" KINDS ":" #OUTW;
#include "leaf_list.hpp"
#undef LEAF
#undef LEAF_HOST
    default: return "";
    }
}
// one launch over n cases of one leaf, 64 threads per block, on `stream`.  Returns a hipError_t (0 = launched), or -1 for an unknown leaf.
__attribute__((visibility("default"))) int LP_SYM(run)(int leaf, const void *ops, const void *flags, void *out, size_t n, void *stream) {
    if (n == 0) return 0;
    if (n > 0x7fffffffull) return -2;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    switch (leaf) {
#define LEAF(ID, NAME, OUTW, KINDS, ...)                                                                                              \
    case ID: hipLaunchKernelGGL(LP_K(NAME), grid, block, 0, (hipStream_t)stream, (const uint32_t *)ops, (const int32_t *)flags, (uint32_t *)out, (uint32_t)n); break;
#define LEAF_HOST(ID, NAME, OUTW, KINDS, STMT, ...) LEAF(ID, NAME, OUTW, KINDS, __VA_ARGS__)
#include "leaf_list.hpp"
#undef LEAF
#undef LEAF_HOST
    default: return -1;
    }
    return (int)hipGetLastError();
}
}
