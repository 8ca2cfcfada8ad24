#!/usr/bin/env python3
"""Batched normalize and projective equality: bn254_g{1,2}_normalize_batch_dev against bn254_g{1,2}_mul_batch_dev with every scalar
Fr::one() on the same points - how a point was normalized before -, and bn254_g{1,2}_eq_batch_dev against the two such multiplications a
comparison took, on one GPU, one process.  The points are random subgroup points with z != 1 (the reference's chain on the device).
  sizes    device-resident, the two calls alternating inside one repetition loop: the median, minimum and maximum over --repeats runs
           (after --warmup) of the KERNEL ms (bn254_kernel_stats: scope g*_normalize against g*_mul) and of the wall ms (enqueue to
           synchronize), the ratio, and whether the [min max] ranges overlap; the results are compared on the device
  eq       the same for scope g*_eq against TWO multiplications by one (both operands), at every size
  variant  --variant NAME: only the normalize kernel at the largest size, for a library built with another run length
           (NORM_RUN of bn_amd/csrc/group_ops.hpp edited, UNITS=bn254_kernels_mul tools/build_variant.sh NAME, BN254_LIB_PATH=...)
Everything printed is also appended to --out (default profiles/r12_normalize.txt; --fresh truncates it first).
usage: tools/time_normalize.py [--groups 1,2] [--repeats 5] [--warmup 1] [--variant NAME] [--fresh]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SIZES = {1: (0, 16, 20), 2: (0, 15, 18)}
FR_ONE = (0xac96341c4ffffffb, 0x36fc76959f60cd29, 0x666ea36f7879462e, 0x0e0a77c19a07df2f)      # the Montgomery image of 1 mod r
OUT = None


def say(line):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def fmt(v):
    return "%8.3f [%7.3f %7.3f]" % (statistics.median(v), min(v), max(v))


def timed(eng, scope, call):
    import torch
    eng.profile(True); eng.profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    ms = eng.kernel_stats(scope)[0]
    eng.profile(False)
    return ms, wall


def points(te, g, n):
    """n random points with z != 1 on the device, by the reference's chain"""
    import torch
    from bn_amd import distributed as D
    g1, g2 = D.generator_limbs()
    gen = torch.from_numpy(np.ascontiguousarray(g1 if g == 1 else g2).view(np.int64)).to(te.device)
    tiled = te.empty(n, 12 if g == 1 else 24)
    te.e.tile_dev(gen.data_ptr(), 96 if g == 1 else 192, n, tiled.data_ptr(), te._stream())
    P = (te.g1_mul if g == 1 else te.g2_mul)(tiled, D.synthetic_scalars_device(te, 1 << 26, (1 << 26) + n, g - 1), normalize=False)
    torch.cuda.synchronize()
    return P


def ones(te, n):
    import torch
    one = torch.from_numpy(np.array(FR_ONE, np.uint64).view(np.int64)).to(te.device)
    k = te.empty(n, 4)
    te.e.tile_dev(one.data_ptr(), 32, n, k.data_ptr(), te._stream())
    torch.cuda.synchronize()
    return k


def compare(label, runs, new, old):
    kn, ko = [r[0] for r in runs[new]], [r[0] for r in runs[old]]
    for nm in (new, old):
        say("%s %-10s | kernel ms %s | wall ms %s" % (label, nm, fmt([r[0] for r in runs[nm]]), fmt([r[1] for r in runs[nm]])))
    say("%s %s / %s = %.1f (kernel medians), %.1f (wall medians); kernel ranges %s" % (
        label, old, new, statistics.median(ko) / statistics.median(kn),
        statistics.median([r[1] for r in runs[old]]) / statistics.median([r[1] for r in runs[new]]), "do not overlap" if max(kn) < min(ko) else "OVERLAP"))


def sizes(eng, te, g, P, lg, repeats, warmup, only_normalize=False, tag=""):
    import torch
    n = 1 if lg == 0 else 1 << lg
    label = "G%d n=%-5s %s" % (g, "1" if lg == 0 else "2^%d" % lg, tag)
    p = P[:n]
    k = ones(te, n)
    mul = te.g1_mul if g == 1 else te.g2_mul
    norm_dev = eng.g1_normalize_dev if g == 1 else eng.g2_normalize_dev
    eq_dev = eng.g1_eq_dev if g == 1 else eng.g2_eq_dev
    out = {"normalize": torch.empty_like(p), "eq": torch.empty(n, dtype=torch.int32, device=te.device)}
    calls = {"normalize": (f"g{g}_normalize", lambda: norm_dev(p.data_ptr(), out["normalize"].data_ptr(), n, te._stream()))}
    if not only_normalize:
        calls["mul_by_one"] = (f"g{g}_mul", lambda: out.__setitem__("mul_by_one", mul(p, k)))
    runs = {nm: [] for nm in calls}
    for rep in range(warmup + repeats):
        for nm, (scope, call) in calls.items():
            r = timed(eng, scope, call)
            if rep >= warmup:
                runs[nm].append(r)
    if only_normalize:
        say("%s normalize  | kernel ms %s" % (label, fmt([r[0] for r in runs["normalize"]])))
        return statistics.median([r[0] for r in runs["normalize"]])
    assert torch.equal(out["normalize"], out["mul_by_one"]), (g, lg)
    compare(label, runs, "normalize", "mul_by_one")
    # eq(p, normalize(p)) against the two multiplications by one that a comparison took
    q = out["normalize"]
    calls = {"eq": (f"g{g}_eq", lambda: eq_dev(p.data_ptr(), q.data_ptr(), out["eq"].data_ptr(), n, te._stream())),
             "2 x mul_by_one": (f"g{g}_mul", lambda: (mul(p, k), mul(q, k)))}
    runs = {nm: [] for nm in calls}
    for rep in range(warmup + repeats):
        for nm, (scope, call) in calls.items():
            r = timed(eng, scope, call)
            if rep >= warmup:
                runs[nm].append(r)
    assert bool((out["eq"] == 1).all()), (g, lg)
    compare(label, runs, "eq", "2 x mul_by_one")


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variant", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12_normalize.txt"))
    ap.add_argument("--fresh", action="store_true")
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import _native
    from bn_amd import distributed as D
    OUT = open(a.out, "w" if a.fresh else "a")
    lib = _native.lib()
    lib.bn254_normalize_run.argtypes = []; lib.bn254_normalize_run.restype = C.c_uint
    eng = bn_amd.Engine(0)
    te = D.TorchEngine(eng, torch.device("cuda", 0))
    K = lib.bn254_normalize_run()
    if a.variant:
        say("variant %s (%s): run length K = %d; kernel ms: median [min max] over %d runs after %d warm-up" % (a.variant, _native.LIB_PATH.name, K, a.repeats, a.warmup))
    else:
        say("shipped library: run length K = %d; kernel / wall ms: median [min max] over %d runs after %d warm-up, one process" % (K, a.repeats, a.warmup))
    for g in (int(x) for x in a.groups.split(",")):
        P = points(te, g, 1 << SIZES[g][-1])
        if a.variant:
            sizes(eng, te, g, P, SIZES[g][-1], a.repeats, a.warmup, only_normalize=True, tag="K=%-2d " % K)
            continue
        for lg in SIZES[g]:
            sizes(eng, te, g, P, lg, a.repeats, a.warmup)
        sizes(eng, te, g, P, SIZES[g][-1], a.repeats, a.warmup, only_normalize=True, tag="K=%-2d " % K)


if __name__ == "__main__":
    main()
