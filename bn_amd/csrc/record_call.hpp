// The host side of a RECORD FAMILY: entry points that take n fixed-size records in, run one lane per record and write n records out, with an
// optional second output (a status word per record).  A family keeps its Ops, a table of BnRecordKind rows, its BnLaunchMax and a launch
// functor (args, lo, cnt, stream) -> int - the `switch` over its Ops for lanes [lo, lo + cnt) -; the check, the sub-launches, the _dev form and
// the host-buffer form are the ones below.  Included by .hip host units only; everything here is a template or inline and hidden, so the
// library's list of dynamic symbols does not see it.  Not part of the ABI.
#pragma once
#include <cstring>

#include "host_ctx.hpp"
#include "lane_launch.hpp"

constexpr size_t BN_RECORD_N_MAX = (size_t)1 << 40;       // records of one call

// one kind of call: the name of its scope (bn254_kernel_stats), its inputs and the bytes of one record of each, of the output and of the second output (0: none)
struct BnRecordKind { const char *scope; int n_in; size_t in_bytes[BN_STAGE_INS]; size_t out_bytes, out2_bytes; };
// the arguments of a call: device or host pointers, depending on the entry point
struct BnRecordArgs { const void *in[BN_STAGE_INS]; void *out, *out2; };

// arguments only: nothing here touches a device.  1 = nothing to do.  An input whose record has no bytes in this call may be NULL.
__attribute__((visibility("hidden"))) inline int bn_record_check(const BnRecordKind &k, const BnRecordArgs &a, size_t n, size_t n_max) {
    if (n == 0) return 1;
    if (!a.out || (k.out2_bytes && !a.out2) || n > n_max) return BN254_E_BAD_ARG;
    for (int j = 0; j < k.n_in; ++j)
        if (!a.in[j] && k.in_bytes[j]) return BN254_E_BAD_ARG;
    return BN254_OK;
}
// sub-launches of at most launch_max.step() records, each under the kind's scope
template <class Launch>
int bn_record_run(bn254_ctx *ctx, const BnRecordKind &k, const BnLaunchMax &launch_max, const BnRecordArgs &a, size_t n, hipStream_t s, const Launch &launch) {
    return bn_for_parts(n, launch_max.step(), [&](size_t lo, size_t cnt) -> int {
        BnScope sc(ctx, s, k.scope);
        return launch(a, lo, cnt, s);
    });
}
// order of the checks: arguments, then context and device; no scratch, nothing waits, nothing is read back
template <class Launch>
int bn_record_dev(bn254_ctx *ctx, const BnRecordKind &k, const BnLaunchMax &launch_max, const BnRecordArgs &a, size_t n, void *stream, const Launch &launch,
                  size_t n_max = BN_RECORD_N_MAX) {
    int rc = bn_record_check(k, a, n, n_max); if (rc) return rc == 1 ? BN254_OK : rc;
    return bn_dev_entry(ctx, stream, false, [&](hipStream_t s) { return bn_record_run(ctx, k, launch_max, a, n, s, launch); });
}
// the host-buffer form: the same checks, then the context's mutex for the whole call and bn_staged_n's sequence on the context's stream
template <class Launch>
int bn_record_host(bn254_ctx *ctx, const BnRecordKind &k, const BnLaunchMax &launch_max, const BnRecordArgs &a, size_t n, const Launch &launch,
                   size_t n_max = BN_RECORD_N_MAX) {
    int rc = bn_record_check(k, a, n, n_max); if (rc) return rc == 1 ? BN254_OK : rc;
    BnHost h(ctx); if (h.rc) return h.rc;
    return bn_no_throw([&] {
        BnStageIn in[BN_STAGE_INS] = {};
        for (int j = 0; j < k.n_in; ++j) in[j] = {k.in_bytes[j] ? a.in[j] : nullptr, n * k.in_bytes[j]};
        return bn_staged_n(ctx, in, k.n_in, a.out, n * k.out_bytes, k.out2_bytes ? a.out2 : nullptr, n * k.out2_bytes, [&](const BnStaged &d) {
            return bn_record_run(ctx, k, launch_max, {{d.in[0], d.in[1], d.in[2], d.in[3]}, d.out, d.out2}, n, ctx->stream, launch);
        });
    });
}

// ---- what the two hash-to-curve families (bn254_hash.hip, bn254_hash_g2.hip) share beyond that: their message kind, whose record size
// (msg_len) and tag are per-call values.  Its own rules run first, before the empty call's answer, and touch no device; the tag travels in
// the Op's argument record (launch.m): DST || len(DST), the same for every lane.  Then go(kind, launch) takes the shared path in the form -
// host buffers, or device pointers on a stream - the entry point chooses.  The other kinds (msg_kind == false) go straight there.
constexpr size_t BN_H2C_MSG_MAX = (size_t)1 << 20;
template <class Launch, class Go>
int bn_h2c_call(BnRecordKind kind, Launch launch, bool msg_kind, size_t msg_len, const uint8_t *dst, size_t dst_len, size_t n, Go go) {
    if (msg_kind) {
        if (dst_len == 0 || dst_len > BN254_H2C_DST_MAX || msg_len > BN_H2C_MSG_MAX) return BN254_E_BAD_ARG;
        if (n && (!dst || n > BN_RECORD_N_MAX || n * msg_len > BN_RECORD_N_MAX)) return BN254_E_BAD_ARG;       // (no overflow: both factors were bounded above)
        kind.in_bytes[0] = msg_len;
        if (n) {
            launch.m.msg_len = msg_len; launch.m.dst_prime_len = (uint32_t)dst_len + 1;
            memcpy(launch.m.dst_prime, dst, dst_len);
            launch.m.dst_prime[dst_len] = (uint8_t)dst_len;
        }
    }
    return go(kind, launch);
}
