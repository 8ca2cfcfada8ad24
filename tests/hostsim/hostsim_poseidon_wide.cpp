// TEST INFRASTRUCTURE - host simulation of bn254_fr_poseidon_ex_batch and bn254_fr_poseidon_chain_batch: the bodies of
// bn_amd/csrc/poseidon_wide_ops.hpp, the table derivation of poseidon_wide_table.hpp and the checks of host_plan.hpp compiled with g++ for the
// CPU - the very code the kernels and the entry points run.  A group of G lanes is a loop over its lanes per phase (HostLanes::phase); the
// exchange buffer is a host array laid out like the workgroup's LDS (three groups interleaved, the middle one used, the others must stay
// untouched).  Built with -DBN_BOUNDS (fe.hpp: a violated bound aborts), so fr_dot runs under its bound checks at every width and cut.  Never
// loaded by the product (bn_amd/); not a CPU fallback.
#define BN_HOSTSIM 1
#include "lanepair.hpp"                    // host_plan.hpp reaches the pairing headers through io.hpp: they need the lane-pair shim
#include "../../bn_amd/csrc/poseidon_wide_ops.hpp"
#include "../../bn_amd/csrc/host_plan.hpp"
#include <vector>

using namespace bn254;
#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {
constexpr uint32_t STRIDE = 3, MINE = 1, PATTERN = 0xffffffffu;      // the pattern is no canonical word string: a read of it trips fr_dot's check
template <int G_>
struct HostLanes {
    static constexpr int G = G_;
    template <class F>
    void phase(F f) const { for (int g = 0; g < G; ++g) f(g); }
};
struct Buffer {
    std::vector<uint32_t> w = std::vector<uint32_t>((size_t)PSDW_GROUP_WORDS * STRIDE, PATTERN);
    PsdwExchange ex() { return PsdwExchange{w.data() + MINE, STRIDE}; }
    bool neighbours_untouched() const {
        for (size_t i = 0; i < w.size(); ++i)
            if (i % STRIDE != MINE && w[i] != PATTERN) return false;
        return true;
    }
};
template <int G>
int ex_lanes(const uint32_t *in, int n_inputs, const uint32_t *init, int n_outs, uint32_t *out, size_t lo, size_t cnt, const uint32_t *tbl) {
    for (size_t i = 0; i < cnt; ++i) {
        Buffer b;
        psdw_ex_body(b.ex(), in, n_inputs, init, n_outs, out, lo + i, psdw::R_P[n_inputs + 1], tbl, HostLanes<G>{});
        if (!b.neighbours_untouched()) return -100;
    }
    return 0;
}
template <int G>
int chain_lanes(const uint32_t *in, const size_t *off, int rate, uint32_t *out, size_t lo, size_t cnt, const uint32_t *tbl) {
    for (size_t i = 0; i < cnt; ++i) {
        Buffer b;
        const size_t j = lo + i;
        psdw_chain_body(b.ex(), in, off[j], off[j + 1] - off[j], rate, out, j, psdw::R_P[rate + 1], tbl, HostLanes<G>{});
        if (!b.neighbours_untouched()) return -100;
    }
    return 0;
}
size_t groups_per_launch(size_t step_lanes, int G) { const size_t g = step_lanes / (size_t)G; return g ? g : 1; }
}  // namespace

EXPORT int hspw_bounds_enabled() {
#if defined(BN_BOUNDS)
    return 1;
#else
    return 0;
#endif
}
EXPORT int hspw_default_lanes() { return BN254_POSEIDON_WIDE_LANES; }
EXPORT size_t hspw_table_elems(int t) { return (t < psdw::T_MIN || t > psdw::T_MAX) ? 0 : psdw::table_elems(t); }
EXPORT int hspw_rounds_partial(int t) { return (t < psdw::T_MIN || t > psdw::T_MAX) ? -1 : psdw::R_P[t]; }
// the table of width t as the kernels read it: table_elems(t) records of eight words, C then M
EXPORT int hspw_table(int t, uint32_t *out) {
    std::vector<uint32_t> host;
    if (!psdw::derive(t, host)) return BN254_E_BAD_ARG;
    for (size_t i = 0; i < host.size(); ++i) out[i] = host[i];
    return 0;
}
EXPORT int hspw_ex_check(const void *in, int n_inputs, const void *init, int n_outs, const void *out, size_t n, int host_buffers) {
    const int rc = bn_poseidon_ex_range(n_inputs, n_outs); if (rc || n == 0) return rc;
    return bn_poseidon_ex_check(in, n_inputs, init, n_outs, out, n, host_buffers != 0);
}
EXPORT int hspw_chain_check(const void *in, const size_t *offsets, size_t m, int rate, const void *out, int host_buffers) {
    if (rate < 1 || rate > BN254_POSEIDON_EX_INPUTS_MAX) return BN254_E_BAD_ARG;
    if (m == 0) return 0;
    return bn_poseidon_chain_check(in, offsets, m, rate, out, host_buffers != 0);
}
// the device forms: sub-launches of at most `step` LANES (step / G groups, at least one), each group through the body; `launches` counts them
EXPORT int hspw_ex(int G, const uint32_t *in, int n_inputs, const uint32_t *init, int n_outs, uint32_t *out, size_t n, size_t step, size_t *launches) {
    *launches = 0;
    int rc = hspw_ex_check(in, n_inputs, init, n_outs, out, n, 1); if (rc || n == 0) return rc;
    std::vector<uint32_t> tbl;
    if (!psdw::derive(n_inputs + 1, tbl)) return BN254_E_INTERNAL;
    return bn_for_parts(n, groups_per_launch(step, G), [&](size_t lo, size_t cnt) -> int {
        ++*launches;
        switch (G) {
        case 4: return ex_lanes<4>(in, n_inputs, init, n_outs, out, lo, cnt, tbl.data());
        case 8: return ex_lanes<8>(in, n_inputs, init, n_outs, out, lo, cnt, tbl.data());
        case 16: return ex_lanes<16>(in, n_inputs, init, n_outs, out, lo, cnt, tbl.data());
        default: return BN254_E_BAD_ARG;
        }
    });
}
EXPORT int hspw_chain(int G, const uint32_t *in, const size_t *offsets, size_t m, int rate, uint32_t *out, size_t step, size_t *launches) {
    *launches = 0;
    int rc = hspw_chain_check(in, offsets, m, rate, out, 1); if (rc || m == 0) return rc;
    std::vector<uint32_t> tbl;
    if (!psdw::derive(rate + 1, tbl)) return BN254_E_INTERNAL;
    return bn_for_parts(m, groups_per_launch(step, G), [&](size_t lo, size_t cnt) -> int {
        ++*launches;
        switch (G) {
        case 4: return chain_lanes<4>(in, offsets, rate, out, lo, cnt, tbl.data());
        case 8: return chain_lanes<8>(in, offsets, rate, out, lo, cnt, tbl.data());
        case 16: return chain_lanes<16>(in, offsets, rate, out, lo, cnt, tbl.data());
        default: return BN254_E_BAD_ARG;
        }
    });
}
