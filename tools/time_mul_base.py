#!/usr/bin/env python3
"""Fixed-base scalar multiplication: bn254_g{1,2}_mul_base_batch against bn254_g{1,2}_mul_batch on the tiled base with the same scalars,
on one GPU, one process (distinct full-width scalars generated on the device; the base is a random point with z != 1).  Per group:
  sizes   device-resident, the two calls alternating inside one repetition loop, the table cached: the median, minimum and maximum over
          --repeats runs (after --warmup) of the KERNEL ms (bn254_kernel_stats: scope g*_mul_base against g*_mul) and of the wall ms
          (enqueue to synchronize), the ratio, and whether the [min max] ranges overlap; the results are compared on the device
  build   the table build alone (scope g*_base_table) and a miss at n = 1 (build + chain, kernel and wall ms: a new base every run) against
          bn254_g{1,2}_mul_batch at n = 1
  sweep   the window widths of --widths at the largest size (the library's process-wide override, for this tool only)
  host    host-buffer wall ms of both calls at the largest size
usage: tools/time_mul_base.py [--groups 1,2] [--repeats 5] [--warmup 1] [--widths 8,10,12]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SIZES = {1: (12, 16, 20), 2: (12, 15, 18)}


def fmt(v):
    return "%8.3f [%7.3f %7.3f]" % (statistics.median(v), min(v), max(v))


def timed(eng, scopes, call):
    import torch
    eng.profile(True); eng.profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    per = [eng.kernel_stats(s)[0] for s in scopes]
    eng.profile(False)
    return per, wall


def bases(te, g, count):
    """`count` random points with z != 1 (host rows), by the reference's chain on the device"""
    import torch
    from bn_amd import distributed as D
    g1, g2 = D.generator_limbs()
    gen = torch.from_numpy(np.ascontiguousarray(g1 if g == 1 else g2).view(np.int64)).to(te.device)
    tiled = te.empty(count, 12 if g == 1 else 24)
    te.e.tile_dev(gen.data_ptr(), 96 if g == 1 else 192, count, tiled.data_ptr(), te._stream())
    P = (te.g1_mul if g == 1 else te.g2_mul)(tiled, D.synthetic_scalars_device(te, 1 << 25, (1 << 25) + count, g - 1), normalize=False)
    torch.cuda.synchronize()
    return P.cpu().numpy().view(np.uint64)


def sizes(eng, te, g, base, logs, repeats, warmup, tag=""):
    import torch
    from bn_amd import distributed as D
    fixed = te.g1_mul_base if g == 1 else te.g2_mul_base
    general = te.g1_mul if g == 1 else te.g2_mul
    dbase = torch.from_numpy(base.view(np.int64)).to(te.device)
    res = {}
    for lg in logs:
        n = 1 << lg
        k = D.synthetic_scalars_device(te, 0, n, g - 1)
        tiled = te.empty(n, base.size)
        te.e.tile_dev(dbase.data_ptr(), 8 * base.size, n, tiled.data_ptr(), te._stream())
        out = {}
        calls = {"fixed": lambda: out.__setitem__("fixed", fixed(base, k)), "general": lambda: out.__setitem__("general", general(tiled, k))}
        runs = {nm: [] for nm in calls}
        for rep in range(warmup + repeats):
            for nm, call in calls.items():
                (ms, built), wall = timed(eng, (f"g{g}_mul_base" if nm == "fixed" else f"g{g}_mul", f"g{g}_base_table"), call)
                if rep >= warmup:
                    assert nm == "general" or built == 0.0, "the table was not cached"
                    runs[nm].append((ms, wall))
        assert torch.equal(out["fixed"], out["general"]), (g, lg)
        kf, kg = [r[0] for r in runs["fixed"]], [r[0] for r in runs["general"]]
        for nm in calls:
            print("G%d n=2^%-2d %s%-8s | kernel ms %s | wall ms %s" % (g, lg, tag, nm, fmt([r[0] for r in runs[nm]]), fmt([r[1] for r in runs[nm]])), flush=True)
        print("G%d n=2^%-2d %sgeneral / fixed = %.2f (kernel medians); ranges %s" % (
            g, lg, tag, statistics.median(kg) / statistics.median(kf), "do not overlap" if max(kf) < min(kg) else "OVERLAP"), flush=True)
        res[lg] = statistics.median(kf)
    return res


def build(eng, te, g, pts, repeats, warmup):
    import torch
    from bn_amd import distributed as D
    fixed = te.g1_mul_base if g == 1 else te.g2_mul_base
    general = te.g1_mul if g == 1 else te.g2_mul
    k1 = D.synthetic_scalars_device(te, 7, 8, g - 1)
    runs, ref = [], []
    for rep in range(warmup + repeats):
        base = pts[rep]                                                   # a base this context has not seen: every run is a miss
        one = torch.from_numpy(base.view(np.int64)).to(te.device).reshape(1, -1)
        (tb, ch), wall = timed(eng, (f"g{g}_base_table", f"g{g}_mul_base"), lambda: fixed(base, k1))
        (gm,), gwall = timed(eng, (f"g{g}_mul",), lambda: general(one, k1))
        if rep >= warmup:
            runs.append((tb, tb + ch, wall)); ref.append((gm, gwall))
    print("G%d table build          | kernel ms %s" % (g, fmt([r[0] for r in runs])), flush=True)
    print("G%d miss at n=1 (fixed)  | kernel ms %s | wall ms %s" % (g, fmt([r[1] for r in runs]), fmt([r[2] for r in runs])), flush=True)
    print("G%d n=1 (general)        | kernel ms %s | wall ms %s" % (g, fmt([r[0] for r in ref]), fmt([r[1] for r in ref])), flush=True)


def host(eng, g, base, lg, repeats, warmup):
    from bn_amd import distributed as D
    n = 1 << lg
    K = D.synthetic_scalars(0, 1 << 10, g - 1)
    K = np.ascontiguousarray(np.tile(K, (n >> 10, 1)))                  # host scalars: 2^10 distinct ones repeated (the kernels do not care)
    tiled = np.ascontiguousarray(np.tile(base, (n, 1)))
    calls = {"fixed": lambda: (eng.g1_mul_base_batch if g == 1 else eng.g2_mul_base_batch)(base, K),
             "general": lambda: (eng.g1_mul_batch if g == 1 else eng.g2_mul_batch)(tiled, K)}
    runs = {nm: [] for nm in calls}
    got = {}
    for rep in range(warmup + repeats):
        for nm, call in calls.items():
            t0 = time.perf_counter()
            got[nm] = call()
            if rep >= warmup:
                runs[nm].append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(got["fixed"], got["general"])
    for nm in calls:
        print("G%d n=2^%-2d host buffers %-8s | wall ms %s" % (g, lg, nm, fmt(runs[nm])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--widths", default="8,10,12")
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import _native
    from bn_amd import distributed as D
    lib = _native.lib()
    lib.bn254_mul_base_window.argtypes = [C.c_int]; lib.bn254_mul_base_window.restype = C.c_uint
    lib.bn254_mul_base_table_bytes.argtypes = [C.c_int]; lib.bn254_mul_base_table_bytes.restype = C.c_size_t
    lib.bn254_mul_base_set_window.argtypes = [C.c_int, C.c_uint]
    eng = bn_amd.Engine(0)
    te = D.TorchEngine(eng, torch.device("cuda", 0))
    print("kernel / wall ms: median [min max] over %d runs after %d warm-up" % (a.repeats, a.warmup))
    for g in (int(x) for x in a.groups.split(",")):
        print("G%d shipped window c = %d, %d table bytes per base" % (g, lib.bn254_mul_base_window(g), lib.bn254_mul_base_table_bytes(g)))
        pts = bases(te, g, a.repeats + a.warmup + 1)
        sizes(eng, te, g, pts[-1], SIZES[g], a.repeats, a.warmup)
        build(eng, te, g, pts, a.repeats, a.warmup)
        best = {}
        for c in (int(x) for x in a.widths.split(",") if x):
            _native.check(lib.bn254_mul_base_set_window(g, c))
            try:
                best[c] = sizes(eng, te, g, pts[-1], SIZES[g][-1:], a.repeats, a.warmup, tag="c=%-2d " % c)[SIZES[g][-1]]
            finally:
                _native.check(lib.bn254_mul_base_set_window(g, 0))
        if best:
            print("G%d sweep at 2^%d: fastest c = %d (%s)" % (g, SIZES[g][-1], min(best, key=best.get), ", ".join("c=%d %.3f ms" % cv for cv in sorted(best.items()))), flush=True)
        host(eng, g, pts[-1], SIZES[g][-1], a.repeats, a.warmup)


if __name__ == "__main__":
    main()
