#!/usr/bin/env python3
"""Sparse linear maps over Fr (bn254_fr_dot_batch) on one GPU, one process; every figure is the median [min max] of --repeats runs after
--warmup.  Kernel ms come from bn254_kernel_stats ("fr_dot" + "fr_dot_fold") around the _dev call.  Three shapes:
  S1  R1CS-like: 3 * 2^18 rows, lengths uniform in 1..6, every 1024th row given 4096 terms, random indices over nx = 2^18
  S2  one segment of 2^22 terms, index == NULL
  S3  2^10 rows of 2^12 terms, every row over all of x (nx = 2^12)
and for each of them
  - piece lengths 4 / 8 / 16 / 32 through the library's process-wide override (internal: bn254_fr_dot_set_piece; the bytes do not depend
    on it, which is checked)
  - for scale, bn254_fr_mul_batch_dev on the same number of pre-gathered terms (it does less - no sum - and moves more: 32 n bytes written)
  - a device-to-device hipMemcpyAsync of the (32 + 8 + 32) n + 32 m bytes the call must move (index == NULL: (32 + 32) n + 32 m)
The rule for the shipped piece length was fixed before measuring: the fastest on S1 ships; if it loses more than 10 % on S2 against the
best there, that is recorded next to the choice.  The lazily reduced variant was not built, so it is not timed.
Everything printed is also written to --out (default profiles/r15_dot.txt).
usage: tools/time_dot.py [--repeats 5] [--warmup 1] [--small]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
OUT = None
PIECES = (4, 8, 16, 32)


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
    """[(name, description, offsets, nx, index as a host array or None)]"""
    rng = np.random.default_rng(15)
    k = 4 if small else 0                                       # --small: every size divided by 2^4, for a dry run
    rows = 3 << (18 - k)
    lens = rng.integers(1, 7, rows)
    lens[::1024] = 4096
    off1 = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nx1 = 1 << (18 - k)
    n2 = 1 << (22 - k)
    r3, c3 = 1 << (10 - k // 2), 1 << (12 - k // 2)
    return [("S1", "R1CS-like: %d rows of 1..6 terms, every 1024th of 4096, nx = %d" % (rows, nx1), off1, nx1, rng.integers(0, nx1, int(off1[-1])).astype(np.uint64)),
            ("S2", "one segment of %d terms, index == NULL" % n2, np.array([0, n2], np.uint64), n2, None),
            ("S3", "%d rows of %d terms over nx = %d" % (r3, c3, c3), (np.arange(r3 + 1, dtype=np.uint64) * c3), c3, np.tile(np.arange(c3, dtype=np.uint64), r3))]


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="sizes divided by 16: a dry run of the tool, not a measurement")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r15_dot.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import _native
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_fr_dot_piece.argtypes = []; lib.bn254_fr_dot_piece.restype = C.c_uint
    lib.bn254_fr_dot_fan.argtypes = []; lib.bn254_fr_dot_fan.restype = C.c_uint
    lib.bn254_fr_dot_set_piece.argtypes = [C.c_uint]
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    P0, F = lib.bn254_fr_dot_piece(), lib.bn254_fr_dot_fan()
    say("shipped library: piece length P = %d, fan F = %d; kernel ms = \"fr_dot\" + \"fr_dot_fold\"; median [min max] over %d runs after %d warm-up, one process%s"
        % (P0, F, a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    sh = shapes(a.small)
    nmax = max(int(o[-1]) for _, _, o, _, _ in sh)
    xmax = max(nx for _, _, _, nx, _ in sh)
    s0 = torch.cuda.current_stream().cuda_stream
    assert xmax <= nmax
    Cf = torch.empty(nmax * 4, dtype=torch.int64, device=dev); G = torch.empty_like(Cf); X = G          # x: the first nx records of the second operand
    copy_words = (72 * nmax + 32 * max(o.size for _, _, o, _, _ in sh)) // 8 + 1
    src = torch.zeros(copy_words, dtype=torch.int64, device=dev); dst = torch.empty_like(src)
    eng.synthetic_scalars_dev(15, 0, nmax, 0, Cf.data_ptr(), s0)
    eng.synthetic_scalars_dev(15, 0, nmax, 1, G.data_ptr(), s0)
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
        for name, what, off, nx, index in sh:
            n, m = int(off[-1]), off.size - 1
            I = None if index is None else torch.from_numpy(index.view(np.int64)).to(dev)
            O = torch.empty(m * 4, dtype=torch.int64, device=dev)
            must = (72 if index is not None else 64) * n + 32 * m
            say("-- %s  %s: n = %d terms, m = %d, %d bytes to move" % (name, what, n, m, must))
            call = lambda: eng.fr_dot_batch_dev(Cf.data_ptr(), None if I is None else I.data_ptr(), X.data_ptr(), nx, off, m, O.data_ptr(), s0)
            lib.bn254_fr_dot_set_piece(0)
            call(); torch.cuda.synchronize()
            ref = O.clone()
            for P in PIECES:
                assert lib.bn254_fr_dot_set_piece(P) == 0
                call(); torch.cuda.synchronize()
                assert torch.equal(O, ref), (name, P)
                launches = kernel_ms(("fr_dot", "fr_dot_fold"), call)[1]
                v = repeat(lambda: kernel_ms(("fr_dot", "fr_dot_fold"), call)[0], a.repeats, a.warmup)
                best[name, P] = statistics.median(v)
                say("%s P = %-2d | kernel ms %s | %8.1f M terms/s | %7.1f GB/s of the bytes to move | launches: %d product, %d fold%s"
                    % (name, P, fmt(v), n / best[name, P] / 1e3, must / best[name, P] / 1e6, launches[0], launches[1], "   (shipped)" if P == P0 else ""))
            lib.bn254_fr_dot_set_piece(0)
            v = repeat(lambda: kernel_ms(("fr_mul",), lambda: eng.fr_mul_batch_dev(Cf.data_ptr(), G.data_ptr(), dst.data_ptr(), n, s0))[0], a.repeats, a.warmup)
            say("%s fr_mul_batch_dev on %d pre-gathered terms (no sum; 96 n bytes) | kernel ms %s | %.2f x the shipped P" % (name, n, fmt(v), statistics.median(v) / best[name, P0]))
            v = repeat(lambda: copy_ms(must), a.repeats, a.warmup)
            say("%s d2d memcpy of the %d bytes to move | event ms %s | %.1f GB/s copied | the shipped P takes %.2f x" % (name, must, fmt(v), must / statistics.median(v) / 1e6, best[name, P0] / statistics.median(v)))
    finally:
        lib.bn254_fr_dot_set_piece(0)
    win = min((best["S1", P], P) for P in PIECES)[1]
    s2 = min(best["S2", P] for P in PIECES)
    loss = best["S2", win] / s2 - 1
    say("-- the rule (fixed before measuring): the fastest P on S1 ships: P = %d (the library carries %d)" % (win, P0))
    say("   on S2 P = %d takes %.4f ms against the best there, %.4f ms (P = %d): %+.1f %%%s"
        % (win, best["S2", win], s2, min((best["S2", P], P) for P in PIECES)[1], 100 * loss, " - MORE than 10 % behind" if loss > 0.10 else ""))
    say("   lazily reduced accumulation (one Montgomery reduction per four products): not built, not timed")


if __name__ == "__main__":
    main()
