#!/usr/bin/env python3
"""Segmented scans over Fr (bn254_fr_scan_batch) on one GPU, one process; every figure is the median [min max] of --repeats runs after
--warmup.  Kernel ms come from bn254_kernel_stats ("fr_scan_reduce" + "fr_scan_up" + "fr_scan_down" + "fr_scan") around the _dev call.
Three shapes, general recurrence (a, b and init given):
  (a)  one segment of 2^22 terms                     - the powers, Horner and grand-product workload
  (b)  2^10 segments of 2^12 terms
  (c)  2^18 segments of 1..24 terms
and for each of them piece lengths 8 / 16 / 32 / 64 through the library's process-wide override (internal: bn254_fr_scan_set_piece; the
bytes do not depend on it, which is checked).  The rule for the shipped piece length was fixed before measuring: the fastest on (a) ships;
how far it is behind the best on (b) and (c) is recorded next to the choice.  The fan (16) is not swept.
Then, for the shipped setting on 2^22 terms in one segment: the general scan, prefix products (b == NULL), prefix sums (a == NULL) and
A_PER_SEGMENT against
  - bn254_fr_mul_batch_dev on the same 2^22 elements (one product per element, 96 bytes moved; the general scan executes three products per
    term and moves about five records per term - a, b read twice, out written once)
  - a device-to-device hipMemcpyAsync of the bytes the variant must move (half read, half written)
  - the host loop groth16.setup used for 2^16 powers (Python integers), as wall time, beside poly.powers(x, 2^16) end to end
Reported, not gated.  Everything printed is also written to --out (default profiles/r16_scan.txt).
usage: tools/time_scan.py [--repeats 5] [--warmup 1] [--small]"""
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
PIECES = (8, 16, 32, 64)
SCOPES = ("fr_scan_reduce", "fr_scan_up", "fr_scan_down", "fr_scan")


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


def shapes(small):
    """[(name, description, offsets)]"""
    rng = np.random.default_rng(16)
    k = 4 if small else 0                                       # --small: every size divided by 2^4, for a dry run
    n_a = 1 << (22 - k)
    r_b, c_b = 1 << (10 - k // 2), 1 << (12 - k // 2)
    lens = rng.integers(1, 25, 1 << (18 - k))
    return [("a", "one segment of %d terms" % n_a, np.array([0, n_a], np.uint64)),
            ("b", "%d segments of %d terms" % (r_b, c_b), np.arange(r_b + 1, dtype=np.uint64) * c_b),
            ("c", "%d segments of 1..24 terms" % lens.size, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))]


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="sizes divided by 16: a dry run of the tool, not a measurement")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r16_scan.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import _native, poly
    from bn_amd.api import R_MOD
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_fr_scan_piece.argtypes = []; lib.bn254_fr_scan_piece.restype = C.c_uint
    lib.bn254_fr_scan_fan.argtypes = []; lib.bn254_fr_scan_fan.restype = C.c_uint
    lib.bn254_fr_scan_set_piece.argtypes = [C.c_uint]
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    P0, F = lib.bn254_fr_scan_piece(), lib.bn254_fr_scan_fan()
    say("shipped library: piece length P = %d, fan F = %d; kernel ms = %s; median [min max] over %d runs after %d warm-up, one process%s"
        % (P0, F, " + ".join('"%s"' % s for s in SCOPES), a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    sh = shapes(a.small)
    nmax = max(int(o[-1]) for _, _, o in sh)
    mmax = max(o.size - 1 for _, _, o in sh)
    s0 = torch.cuda.current_stream().cuda_stream
    A = torch.empty(nmax * 4, dtype=torch.int64, device=dev); B = torch.empty_like(A); O = torch.empty_like(A)
    I = torch.empty(max(mmax, 1) * 4, dtype=torch.int64, device=dev)
    src = torch.zeros(nmax * 4 * 3, dtype=torch.int64, device=dev); dst = torch.empty_like(src)
    eng.synthetic_scalars_dev(16, 0, nmax, 0, A.data_ptr(), s0)
    eng.synthetic_scalars_dev(16, 0, nmax, 1, B.data_ptr(), s0)
    eng.synthetic_scalars_dev(17, 0, mmax, 0, I.data_ptr(), s0)
    torch.cuda.synchronize()

    def kernel_ms(scopes, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        got = [eng.kernel_stats(s) for s in scopes]
        eng.profile(False)
        return sum(ms for ms, _ in got), [l for _, l in got]

    def copy_ms(nbytes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, s0) == 0
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    best = {}
    try:
        for name, what, off in sh:
            n, m = int(off[-1]), off.size - 1
            say("-- (%s)  %s: n = %d terms, m = %d, general recurrence" % (name, what, n, m))
            call = lambda: eng.fr_scan_batch_dev(A.data_ptr(), B.data_ptr(), I.data_ptr(), off, m, O.data_ptr(), stream=s0)
            lib.bn254_fr_scan_set_piece(0)
            call(); torch.cuda.synchronize()
            ref = O[:n * 4].clone()
            for P in PIECES:
                assert lib.bn254_fr_scan_set_piece(P) == 0
                call(); torch.cuda.synchronize()
                assert torch.equal(O[:n * 4], ref), (name, P)
                launches = kernel_ms(SCOPES, call)[1]
                v = repeat(lambda: kernel_ms(SCOPES, call)[0], a.repeats, a.warmup)
                best[name, P] = statistics.median(v)
                say("(%s) P = %-2d | kernel ms %s | %8.1f M terms/s | launches: %d reduce, %d up, %d down, %d apply%s"
                    % (name, P, fmt(v), n / best[name, P] / 1e3, launches[0], launches[1], launches[2], launches[3], "   (shipped)" if P == P0 else ""))
            lib.bn254_fr_scan_set_piece(0)
    finally:
        lib.bn254_fr_scan_set_piece(0)
    win = min((best["a", P], P) for P in PIECES)[1]
    say("-- the rule (fixed before measuring): the fastest P on (a) ships: P = %d (the library carries %d)" % (win, P0))
    for name in ("b", "c"):
        t, p = min((best[name, P], P) for P in PIECES)
        say("   on (%s) P = %d takes %.4f ms against the best there, %.4f ms (P = %d): %+.1f %%" % (name, win, best[name, win], t, p, 100 * (best[name, win] / t - 1)))
    say("   the fan F = %d was not swept" % F)

    n = int(sh[0][2][-1])
    off = sh[0][2]
    say("-- the shipped setting (P = %d) on one segment of %d terms against its floors" % (P0, n))
    mul = repeat(lambda: kernel_ms(("fr_mul",), lambda: eng.fr_mul_batch_dev(A.data_ptr(), B.data_ptr(), O.data_ptr(), n, s0))[0], a.repeats, a.warmup)
    say("fr_mul_batch_dev on %d elements (one product each, 96 n bytes) | kernel ms %s" % (n, fmt(mul)))
    mul_ms = statistics.median(mul)
    variants = [("general (a, b, init)", (A, B, I), {}, 5),                           # records per term: a and b read twice, out written
                ("prefix products (b == NULL)", (A, None, None), {}, 3),              # a read twice, out written
                ("prefix sums (a == NULL)", (None, B, None), {}, 3),
                ("A_PER_SEGMENT (Horner: a[0], b)", (A, B, None), {"a_per_segment": True}, 3)]
    for what, (xa, xb, xi), flags, recs in variants:
        ptr = lambda t: None if t is None else t.data_ptr()
        call = lambda: eng.fr_scan_batch_dev(ptr(xa), ptr(xb), ptr(xi), off, 1, O.data_ptr(), stream=s0, **flags)
        v = repeat(lambda: kernel_ms(SCOPES, call)[0], a.repeats, a.warmup)
        must = recs * 32 * n
        c = repeat(lambda: copy_ms(must // 2), a.repeats, a.warmup)                   # a copy of k bytes moves 2 k
        ms = statistics.median(v)
        say("%-34s | kernel ms %s | %8.1f M terms/s | %.2f x fr_mul_batch_dev | %d n bytes to move: d2d copy %.4f ms, the scan takes %.2f x"
            % (what, fmt(v), n / ms / 1e3, ms / mul_ms, recs * 32, statistics.median(c), ms / statistics.median(c)))
    k = 1 << (12 if a.small else 16)
    tau = int.from_bytes(np.random.default_rng(1).bytes(64), "little") % R_MOD

    def host_loop():
        t0 = time.perf_counter()
        powers = [1]
        for _ in range(k - 1):
            powers.append(powers[-1] * tau % R_MOD)
        return (time.perf_counter() - t0) * 1e3

    def device_powers():
        t0 = time.perf_counter()
        poly.powers(bn_amd.Fr(tau), k, limbs=True)
        return (time.perf_counter() - t0) * 1e3
    h = repeat(host_loop, a.repeats, a.warmup)
    d = repeat(device_powers, a.repeats, a.warmup)
    say("%d powers: the host loop groth16.setup used (Python integers; their %d conversions to limbs not counted) | wall ms %s" % (k, k, fmt(h)))
    say("%d powers: poly.powers(x, n, limbs=True) end to end (plan, upload, four kernels, copy back) | wall ms %s | %.1f x faster" % (k, fmt(d), statistics.median(h) / statistics.median(d)))
    say("   not built: a single-pass look-back scan (by decision: no workgroup waits on another), a lazily reduced reduce level, a sweep of the fan")


if __name__ == "__main__":
    main()
