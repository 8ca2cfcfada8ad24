// TEST INFRASTRUCTURE - host simulation of bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch and bn254_fr_merkle_tree: the bodies of
// bn_amd/csrc/poseidon_ops.hpp and the checks and level arithmetic of host_plan.hpp (bn_poseidon_check, bn_merkle_check, bn_merkle_plan)
// compiled with g++ for the CPU - the very code the kernels and the entry points run, one loop over lanes per launch, over host arrays.
// Built with -DBN_BOUNDS (fe.hpp: a violated bound aborts), once with -DBN254_POSEIDON_FUSED_ROW=0 and once with =1, so that the product-sum
// of fr.hpp (fr_dot) is run under its bound checks by the whole permutation whichever variant the library ships.  Never loaded by the
// product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // host_plan.hpp reaches the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/poseidon_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int hsp_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
EXPORT int hsp_fused_row() {
#if BN254_POSEIDON_FUSED_ROW
    return 1;
#else
    return 0;
#endif
}
EXPORT int hsp_poseidon_check(const void *in, int t, const void *out, size_t n) { return bn_poseidon_check(in, t, out, n); }
EXPORT int hsp_merkle_check(const void *leaves, int log_n, const void *nodes) { return bn_merkle_check(leaves, log_n, nodes); }
// the plan as plain words: levels as (cnt, src, dst, parts, from_leaves) rows.  Returns the number of levels; nothing is written beyond the capacity.
EXPORT size_t hsp_merkle_plan(int log_n, size_t step, uint64_t *levels, size_t level_cap) {
    const std::vector<BnMerkleLevel> plan = bn_merkle_plan(log_n, step);
    for (size_t l = 0; l < plan.size() && l < level_cap; ++l) {
        const BnMerkleLevel &lv = plan[l];
        levels[5 * l] = lv.cnt; levels[5 * l + 1] = lv.src; levels[5 * l + 2] = lv.dst; levels[5 * l + 3] = lv.parts; levels[5 * l + 4] = lv.from_leaves;
    }
    return plan.size();
}
template <template <int> class Body>
static void lanes_t(int t, const uint32_t *in, uint32_t *out, size_t lo, size_t cnt) {
    for (size_t i = 0; i < cnt; ++i) switch (t) {
        case 2: Body<2>::run(in, out, lo + i); break;
        case 3: Body<3>::run(in, out, lo + i); break;
        case 4: Body<4>::run(in, out, lo + i); break;
        default: Body<5>::run(in, out, lo + i); break;
    }
}
template <int T> struct HashBody { static void run(const uint32_t *in, uint32_t *out, size_t i) { fr_poseidon_hash_body<T>(in, out, i); } };
template <int T> struct PermuteBody { static void run(const uint32_t *in, uint32_t *out, size_t i) { fr_poseidon_permute_body<T>(in, out, i); } };
// the device forms: sub-launches of at most `step` lanes, each lane through the body; `launches` counts them
EXPORT int hsp_hash(const uint32_t *in, int arity, uint32_t *out, size_t n, size_t step, size_t *launches) {
    *launches = 0;
    if (arity < 1 || arity > BN254_POSEIDON_ARITY_MAX) return BN254_E_BAD_ARG;
    if (n == 0) return 0;
    const int rc = bn_poseidon_check(in, arity + 1, out, n); if (rc) return rc;
    return bn_for_parts(n, step, [&](size_t lo, size_t cnt) -> int { ++*launches; lanes_t<HashBody>(arity + 1, in, out, lo, cnt); return 0; });
}
// out may be in
EXPORT int hsp_permute(const uint32_t *in, int t, uint32_t *out, size_t n, size_t step, size_t *launches) {
    *launches = 0;
    if (t < 2 || t > BN254_POSEIDON_ARITY_MAX + 1) return BN254_E_BAD_ARG;
    if (n == 0) return 0;
    const int rc = bn_poseidon_check(in, t, out, n); if (rc) return rc;
    return bn_for_parts(n, step, [&](size_t lo, size_t cnt) -> int { ++*launches; lanes_t<PermuteBody>(t, in, out, lo, cnt); return 0; });
}
// The levels of the plan in its order.  Every level is checked against `nodes` before its lanes run (-1: a level reads or writes outside
// the n - 1 nodes, -2: it reads a node no earlier level wrote, -3: a node is written twice, -4: a node nothing wrote).  A positive return is
// the argument check's answer negated.
EXPORT int hsp_merkle(const uint32_t *leaves, int log_n, uint32_t *nodes, size_t step, size_t *launches) {
    *launches = 0;
    const int rc = bn_merkle_check(leaves, log_n, nodes); if (rc) return -rc;
    if (log_n == 0) return 0;
    const size_t n = (size_t)1 << log_n;
    std::vector<char> done(n - 1, 0);
    size_t expect = n / 2;
    for (const BnMerkleLevel &lv : bn_merkle_plan(log_n, step)) {
        if (lv.cnt != expect || lv.dst + lv.cnt > n - 1 || lv.parts != (lv.cnt + step - 1) / step) return -1;
        if (!lv.from_leaves) {
            if (lv.src + 2 * lv.cnt > n - 1) return -1;
            for (size_t i = 0; i < 2 * lv.cnt; ++i)
                if (!done[lv.src + i]) return -2;
        }
        for (size_t i = 0; i < lv.cnt; ++i) { if (done[lv.dst + i]) return -3; done[lv.dst + i] = 1; }
        const uint32_t *src = lv.from_leaves ? leaves : nodes + 8 * lv.src;
        bn_for_parts(lv.cnt, step, [&](size_t lo, size_t cnt) -> int { ++*launches; lanes_t<HashBody>(3, src, nodes + 8 * lv.dst, lo, cnt); return 0; });
        expect /= 2;
    }
    for (size_t i = 0; i < n - 1; ++i)
        if (!done[i]) return -4;
    return expect == 0 ? 0 : -1;
}
// fr_dot<T> of fr.hpp alone: sum_k a[k] * b[k] over T pairs of canonical Montgomery images (its bound checks abort the process)
EXPORT int hsp_dot(int T, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    Fr r;
    switch (T) {
    case 1: { Fr x[1]; x[0] = fr_load(a, 0); r = fr_dot<1>(x, (const uint32_t (*)[8])b); break; }
    case 2: { Fr x[2]; for (int i = 0; i < 2; ++i) x[i] = fr_load(a, i); r = fr_dot<2>(x, (const uint32_t (*)[8])b); break; }
    case 3: { Fr x[3]; for (int i = 0; i < 3; ++i) x[i] = fr_load(a, i); r = fr_dot<3>(x, (const uint32_t (*)[8])b); break; }
    case 4: { Fr x[4]; for (int i = 0; i < 4; ++i) x[i] = fr_load(a, i); r = fr_dot<4>(x, (const uint32_t (*)[8])b); break; }
    case 5: { Fr x[5]; for (int i = 0; i < 5; ++i) x[i] = fr_load(a, i); r = fr_dot<5>(x, (const uint32_t (*)[8])b); break; }
    default: return BN254_E_BAD_ARG;
    }
    fr_store(r, out, 0);
    return 0;
}
