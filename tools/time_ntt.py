#!/usr/bin/env python3
"""Number-theoretic transforms over Fr (bn254_fr_ntt_batch) on one GPU, one process; every figure is the median [min max] of --repeats runs
after --warmup.
  kernel    kernel ms (bn254_kernel_stats "ntt") of the _dev call for one transform of 2^12, 2^16, 2^20, 2^24 and for 2^8 transforms of 2^12:
            forward, inverse and coset inverse (shift 5), each beside
              - the bandwidth floor: a device-to-device hipMemcpyAsync of the same bytes, times the number of passes, timed in the same run
              - the compute floor: the Montgomery products per element the passes issue (counted from the plan), 136 multiply-adds each,
                at the rate bn254_ubench_mac32_ex measures on 32-bit operands in the same run
  tiles     tile logs 8 .. the shipped one through the library's process-wide override (internal: bn254_ntt_set_tile_log; the bytes do not
            depend on it, which is checked) at 2^20 and 2^24
  table     the build of the twiddle tables ("ntt_table"): launches, kernel ms, bytes held
  wall      the host-buffer call of one 2^20 transform (staging and copies included) against an O(n log n) transform over Python integers
Everything printed is also written to --out (default profiles/r14_ntt.txt).
usage: tools/time_ntt.py [--repeats 5] [--warmup 1] [--lg 12,16,20,24] [--no-python-model]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
OUT = None
MACS_PER_PRODUCT = 136              # fr.hpp fr_mul: 128 multiply-adds and 8 low products
TBL_LOG = 12                        # ntt_ops.hpp NTT_TBL_LOG


def say(line):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def fmt(v):
    return "%9.4f [%9.4f %9.4f]" % (statistics.median(v), min(v), max(v))


def repeat(fn, repeats, warmup):
    out = []
    for rep in range(warmup + repeats):
        r = fn()
        if rep >= warmup:
            out.append(r)
    return out


def plan(log_n, T):
    """host_plan.hpp bn_ntt_plan: [(t, log_m, log_s)]"""
    P = -(-log_n // T) if log_n else 1
    base, rem = divmod(log_n, P)
    out, done = [], 0
    for i in range(P):
        t = base + (1 if i < rem else 0)
        out.append((t, log_n - done - t, done))
        done += t
    return out


def products_per_element(log_n, T, inverse, shift):
    """Montgomery products per element over all passes (ntt_ops.hpp): half a product per stage but the last of a pass, two for the twiddle
    between passes (its two table halves, then the element), one or two for the coset power, one for n^-1"""
    total = 0.0
    for t, log_m, _ in plan(log_n, T):
        total += max(t - 1, 0) / 2 + (2 if log_m else 0)
    if shift:
        total += 2 if log_n > TBL_LOG else 1
    elif inverse:
        total += 1
    return total


def python_ntt(x, w, r):
    n = len(x)
    bits = n.bit_length() - 1
    a = [0] * n
    for i in range(n):
        a[int(format(i, "0%db" % bits)[::-1], 2) if bits else 0] = x[i]
    size = 2
    while size <= n:
        wm = pow(w, n // size, r)
        half = size // 2
        tw = [1] * half
        for j in range(1, half):
            tw[j] = tw[j - 1] * wm % r
        for start in range(0, n, size):
            for j in range(half):
                u, v = a[start + j], a[start + j + half] * tw[j] % r
                a[start + j], a[start + j + half] = (u + v) % r, (u - v) % r
        size *= 2
    return a


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lg", default="12,16,20,24")
    ap.add_argument("--no-python-model", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r14_ntt.txt"))
    ap.add_argument("--sweep-only", action="store_true", help="only the tile-log sweep, APPENDED to --out: for a variant library (BN254_LIB_PATH) built with a larger tile")
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import Fr, _native
    OUT = open(a.out, "a" if a.sweep_only else "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_ntt_tile_log.argtypes = []; lib.bn254_ntt_tile_log.restype = C.c_uint
    lib.bn254_ntt_set_tile_log.argtypes = [C.c_uint]
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    T = lib.bn254_ntt_tile_log()
    say("%s: tile log T = %d (2^%d elements: %d KiB of LDS per workgroup, and up to %d KiB for the stage twiddles of a pass); median [min max] over %d runs after %d warm-up, one process"
        % ("== variant library " + str(_native.LIB_PATH.name) if a.sweep_only else "shipped library", T, T, 32 << T >> 10, 16 << T >> 10, a.repeats, a.warmup))
    lgs = [int(x) for x in a.lg.split(",")]
    nmax = 1 << max(lgs + [20])
    s0 = torch.cuda.current_stream().cuda_stream
    A = torch.empty(nmax * 4, dtype=torch.int64, device=dev); O = torch.empty_like(A); O2 = torch.empty_like(A)
    eng.synthetic_scalars_dev(7, 0, nmax, 0, A.data_ptr(), s0)
    torch.cuda.synchronize()
    five = Fr(5).limbs

    def kernel_ms(scope, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        ms, launches = eng.kernel_stats(scope)
        eng.profile(False)
        return ms, launches

    if not a.sweep_only:
        measure(a, eng, lib, hip, torch, A, O, O2, s0, five, T, lgs, kernel_ms)
    sweep(a, eng, lib, torch, A, O, O2, s0, five, T, nmax, kernel_ms)
    if not a.sweep_only:
        wall(a, eng, A, Fr, bn_amd)


def measure(a, eng, lib, hip, torch, A, O, O2, s0, five, T, lgs, kernel_ms):
    say("-- the twiddle tables: built on the device on first use, kept by the context")
    first = kernel_ms("ntt_table", lambda: eng.fr_ntt_batch_dev(A.data_ptr(), O.data_ptr(), 12, 1, False, None, s0))
    again = kernel_ms("ntt_table", lambda: eng.fr_ntt_batch_dev(A.data_ptr(), O.data_ptr(), 16, 1, True, None, s0))
    coset = kernel_ms("ntt_table", lambda: eng.fr_ntt_batch_dev(A.data_ptr(), O.data_ptr(), 12, 1, False, five, s0))
    say("root pair (w_24^i, w_24^(2^12 i), i < 2^12: 256 KiB), first call of the context | %d launch, kernel ms %.4f" % (first[1], first[0]))
    say("a later call of another size and direction                                     | %d launches" % again[1])
    say("shift pair (the powers of one coset shift for one size and direction: 256 KiB)  | %d launch, kernel ms %.4f" % (coset[1], coset[0]))
    say("held per context: 512 KiB of tables; between the passes of a transform above 2^T one array of the group's size (two for an odd number of passes in place)")

    g32, _ = eng.ubench_mac32(8, 1 << 15, 32)
    say("-- bn254_ubench_mac32_ex at 32-bit operands, 8 waves per SIMD: %.1f G multiply-adds/s" % g32)

    def copy_ms(nbytes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert hip.hipMemcpyAsync(O2.data_ptr(), A.data_ptr(), nbytes, 3, s0) == 0
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def transform_ms(lg, count, inverse, shift):
        return kernel_ms("ntt", lambda: eng.fr_ntt_batch_dev(A.data_ptr(), O.data_ptr(), lg, count, inverse, shift, s0))[0]

    say("-- kernel ms of the _dev call, out of place")
    shapes = [(lg, 1) for lg in lgs] + [(12, 1 << 8)]
    for lg, count in shapes:
        n = count << lg
        label = "%3d x 2^%-2d" % (count, lg)
        passes = len(plan(lg, T))
        cp = repeat(lambda: copy_ms(32 * n), a.repeats, a.warmup)
        floor_bw = statistics.median(cp) * passes
        say("%s d2d memcpy of 32 n bytes | event ms %s | x %d passes = %.4f ms (bandwidth floor), %.1f GB/s of traffic"
            % (label, fmt(cp), passes, floor_bw, 64 * n / statistics.median(cp) / 1e6))
        for name, inverse, shift in (("forward", False, None), ("inverse", True, None), ("coset inverse", True, five)):
            v = repeat(lambda: transform_ms(lg, count, inverse, shift), a.repeats, a.warmup)
            med = statistics.median(v)
            prods = products_per_element(lg, T, inverse, shift is not None)
            floor_mac = n * prods * MACS_PER_PRODUCT / (g32 * 1e9) * 1e3
            say("%s %-13s | kernel ms %s | %7.1f M elements/s | %.2f x the bandwidth floor | %.2f products per element: compute floor %.4f ms, %.2f x"
                % (label, name, fmt(v), n / med / 1e3, med / floor_bw, prods, floor_mac, med / floor_mac))



def sweep(a, eng, lib, torch, A, O, O2, s0, five, T, nmax, kernel_ms):
    def transform_ms(lg, count, inverse, shift):
        return kernel_ms("ntt", lambda: eng.fr_ntt_batch_dev(A.data_ptr(), O.data_ptr(), lg, count, inverse, shift, s0))[0]

    say("-- tile logs 8 .. %d through the override (it only goes down from the library's own), forward, kernel ms" % T)
    best = {}
    try:
        for lg in (20, 24):
            if (1 << lg) > nmax:
                continue
            eng.fr_ntt_batch_dev(A.data_ptr(), O2.data_ptr(), lg, 1, False, five, s0); torch.cuda.synchronize()
            ref = O2[:4 << lg].clone()
            for t in range(8, T + 1):
                assert lib.bn254_ntt_set_tile_log(t) == 0
                eng.fr_ntt_batch_dev(A.data_ptr(), O.data_ptr(), lg, 1, False, five, s0); torch.cuda.synchronize()
                assert torch.equal(O[:4 << lg], ref), (lg, t)
                v = repeat(lambda: transform_ms(lg, 1, False, None), a.repeats, a.warmup)
                best[lg, t] = statistics.median(v)
                say("2^%d tile log %-2d (%d passes: %s stages) | kernel ms %s%s" % (lg, t, len(plan(lg, t)), "+".join(str(p[0]) for p in plan(lg, t)), fmt(v), "   (this library's own)" if t == T else ""))
    finally:
        lib.bn254_ntt_set_tile_log(0)
    for lg in (20, 24):
        mine = [(v, t) for (l, t), v in best.items() if l == lg]
        if mine:
            say("fastest tile log at 2^%d: %d" % (lg, min(mine)[1]))
    say("twiddle schemes: only the factored one (two tables of 2^12 entries, a pass's stage twiddles copied to LDS) was built; a full half-table of 16 n bytes was not, so it was not measured")



def wall(a, eng, A, Fr, bn_amd):
    say("-- wall ms of one 2^20 transform: the host-buffer call (staging, copies) against an O(n log n) transform over Python integers")
    n = 1 << 20
    ha = A[:n * 4].cpu().numpy().view(np.uint64).reshape(n, 4)

    def once():
        t0 = time.perf_counter()
        eng.fr_ntt_batch(ha, 20)
        return (time.perf_counter() - t0) * 1e3
    vg = repeat(once, a.repeats, a.warmup)
    if a.no_python_model:
        say("2^20 forward | host-buffer call %s | Python model not run" % fmt(vg))
    else:
        r = bn_amd.api.R_MOD
        minv = pow(1 << 256, -1, r)
        ints = [(int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192) * minv % r for x in ha]
        t0 = time.perf_counter()
        want = python_ntt(ints, Fr.root_of_unity(20).v, r)
        py = (time.perf_counter() - t0) * 1e3
        got = eng.fr_ntt_batch(ha, 20)
        for k in (0, 1, n // 2, n - 1, 123457):
            assert Fr.from_limbs(got[k]).v == want[k], k
        say("2^20 forward | host-buffer call %s | Python model %.0f ms (one run) | %.0f x" % (fmt(vg), py, py / statistics.median(vg)))


if __name__ == "__main__":
    main()
