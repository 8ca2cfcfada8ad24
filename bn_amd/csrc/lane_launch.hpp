// What the units of the integer ("lane") kernels share: the ONE kernel shell bn254_fr_decode_k<B, Op> every family's Ops are instances of, its
// two launchers, the cap of one launch, and the process-wide overrides behind the internal setters of tests and tools (sub-launch size,
// measurement variants).  Included by .hip units only; needs nothing of host_ctx.hpp, so the kernel units include it too.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>

#include "../../include/bn254_hip.h"

constexpr size_t BN_LAUNCH_MAX = (size_t)1 << 22;       // units per launch (32-bit word offsets inside a kernel); also the cap of the size options

// The kernel: a workgroup of B lanes runs op().  The Op (a struct of the unit's anonymous namespace, passed by value) owns the lane index, the
// bounds check and the body; B is the __launch_bounds__ the unit's Ops are written for (they index with the same constant).
template <unsigned B, class Op>
__global__ void __launch_bounds__(B) bn254_fr_decode_k(Op op) { op(); }

// one lane per unit of work: ceil(lanes / B) workgroups
template <unsigned B, class Op>
int bn_lane_launch(const Op &op, size_t lanes, hipStream_t s) {
    hipLaunchKernelGGL((bn254_fr_decode_k<B, Op>), dim3((unsigned)((lanes + B - 1) / B)), dim3(B), 0, s, op);
    return (int)hipGetLastError();
}
// the kernels that index by workgroup: `blocks` workgroups with `lds_bytes` of dynamic LDS each
template <unsigned B, class Op>
int bn_block_launch(const Op &op, size_t blocks, size_t lds_bytes, hipStream_t s) {
    if (lds_bytes > 64 * 1024) {                                                   // only a variant library with a larger tile gets here
        const hipError_t e = hipFuncSetAttribute((const void *)bn254_fr_decode_k<B, Op>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((bn254_fr_decode_k<B, Op>), dim3((unsigned)blocks), dim3(B), lds_bytes, s, op);
    return (int)hipGetLastError();
}

// A process-wide override for tests and measurement tools: 0 (the initial state) = the shipped value.  Host side; a relaxed atomic because
// every launch path reads it, possibly from several host threads.  The exported setters check their range and forward to set().
template <class T>
struct BnOverride {
    std::atomic<T> v{};
    T get(T shipped) const { const T set = v.load(std::memory_order_relaxed); return set ? set : shipped; }
    int set(T value) { v.store(value, std::memory_order_relaxed); return BN254_OK; }
};
// the sub-launch size of a family (0 = BN_LAUNCH_MAX), so that a test reaches the seam between two sub-launches with a handful of elements
struct BnLaunchMax {
    BnOverride<size_t> v;
    size_t step() const { return v.get(BN_LAUNCH_MAX); }
    int set(size_t units) { return units > BN_LAUNCH_MAX ? BN254_E_BAD_ARG : v.set(units); }
};
