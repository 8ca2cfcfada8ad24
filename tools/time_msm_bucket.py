#!/usr/bin/env python3
"""One large multi-scalar multiplication: the bucket route of bn254_g{1,2}_msm against the parent's route - bn254_g{1,2}_msm_batch with the
one segment {0, n} - on one GPU, one process, device-resident inputs (distinct points with z != 1 made by the reference chain, distinct
full-width scalars).  For every n the candidates alternate inside one repetition loop: the new call with msm_bucket_min = 0 at every
candidate window width c, the new call with DEFAULT options, and the parent's route.  Per candidate: the median, minimum and maximum over
--repeats runs (after --warmup) of the KERNEL ms (bn254_kernel_stats, summed over the scopes of the call) and of the wall ms
(enqueue to synchronize), and the kernel ms per scope of the median run.  --equal adds the all-equal-scalars input (every term in one
bucket per window) at the given sizes, default options against the parent's route.
usage: tools/time_msm_bucket.py [--groups 1,2] [--log2 12-20] [--widths auto] [--repeats 5] [--warmup 1] [--equal 16,20]"""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SCOPES = ("digits", "bucket", "reduce", "mul", "fold")


def inputs(te, g, n, equal):
    import torch
    from bn_amd import distributed as D
    g1, g2 = D.generator_limbs()
    gen = torch.from_numpy(np.ascontiguousarray(g1 if g == 1 else g2).view(np.int64)).to(te.device)
    kb = D.synthetic_scalars_device(te, 0, n, g - 1)
    base = te.empty(n, 12 if g == 1 else 24)
    te.e.tile_dev(gen.data_ptr(), 96 if g == 1 else 192, n, base.data_ptr(), te._stream())
    P = (te.g1_mul if g == 1 else te.g2_mul)(base, kb, normalize=False)
    k = D.synthetic_scalars_device(te, 1 << 24, (1 << 24) + n, 1)
    if equal:
        k = k[:1].repeat(n, 1).contiguous()
    torch.cuda.synchronize()
    return P, k


def timed(eng, g, call):
    import torch
    eng.profile(True); eng.profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    per = {s: eng.kernel_stats(f"g{g}_msm_{s}")[0] for s in SCOPES}
    eng.profile(False)
    return sum(per.values()), wall, per


def fmt(v):
    return "%8.3f [%7.3f %7.3f]" % (statistics.median(v), min(v), max(v))


def measure(eng, te, g, n, widths, repeats, warmup, equal):
    import torch
    P, k = inputs(te, g, n, equal)
    out = {}
    new = eng.g1_msm_dev if g == 1 else eng.g2_msm_dev
    old = eng.g1_msm_batch_dev if g == 1 else eng.g2_msm_batch_dev

    def cand(name):
        o = out.setdefault(name, te.empty(1, P.shape[1]))
        if name == "parent":
            return lambda: old(P.data_ptr(), k.data_ptr(), [0, n], o.data_ptr(), te._stream())
        return lambda: new(P.data_ptr(), k.data_ptr(), n, o.data_ptr(), te._stream())

    names = [f"c={c}" for c in widths] + ["default", "parent"]
    runs = {nm: [] for nm in names}
    for rep in range(warmup + repeats):
        for nm in names:
            opts = {} if nm in ("default", "parent") else {"msm_bucket_min": 0, "msm_window_bits": int(nm[2:])}
            with eng.options(**opts):
                r = timed(eng, g, cand(nm))
            if rep >= warmup:
                runs[nm].append(r)
    torch.cuda.synchronize()
    for nm in names:
        assert torch.equal(out[nm], out["parent"]), (g, n, nm)
    route = "buckets" if any(runs["default"][0][2][s] for s in ("digits", "bucket", "reduce")) else "segmented"
    for nm in names:
        rs = sorted(runs[nm], key=lambda r: r[0])
        med = rs[len(rs) // 2][2]
        print("G%d n=2^%-2d %-5s %-8s | kernel ms %s | wall ms %s | %s%s" % (
            g, n.bit_length() - 1, "equal" if equal else "rand", nm, fmt([r[0] for r in rs]), fmt([r[1] for r in rs]),
            "  ".join("%s %.3f" % (s, med[s]) for s in SCOPES if med[s]), "  (route: %s)" % route if nm == "default" else ""), flush=True)
    km = {nm: statistics.median(r[0] for r in runs[nm]) for nm in names}
    best = min((nm for nm in names if nm.startswith("c=")), key=lambda nm: km[nm], default=None)
    print("G%d n=2^%-2d %-5s best %s: parent / best = %.2f, parent / default = %.2f" % (
        g, n.bit_length() - 1, "equal" if equal else "rand", best, km["parent"] / km[best] if best else float("nan"), km["parent"] / km["default"]), flush=True)


def auto_widths(lg):
    return sorted({max(4, min(16, lg - d)) for d in (8, 6, 5, 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--log2", default="12-20")
    ap.add_argument("--widths", default="auto")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--equal", default="16,19,20")
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import distributed as D
    eng = bn_amd.Engine(0)
    te = D.TorchEngine(eng, torch.device("cuda", 0))
    lo, hi = (int(x) for x in a.log2.split("-"))
    print("kernel / wall ms: median [min max] over %d runs after %d warm-up; default bucket_min = %d (G1; G2: see the route of its default rows)" % (a.repeats, a.warmup, eng.get_option("msm_bucket_min")))
    for g in (int(x) for x in a.groups.split(",")):
        top = hi if g == 1 else min(hi, 19)
        for lg in range(lo, top + 1):
            widths = auto_widths(lg) if a.widths == "auto" else [int(x) for x in a.widths.split(",")]
            measure(eng, te, g, 1 << lg, widths, a.repeats, a.warmup, False)
        for lg in (int(x) for x in a.equal.split(",") if x):
            if lg <= top:
                measure(eng, te, g, 1 << lg, [], a.repeats, a.warmup, True)


if __name__ == "__main__":
    main()
