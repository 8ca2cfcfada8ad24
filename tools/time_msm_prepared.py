#!/usr/bin/env python3
"""Multi-scalar multiplication against prepared bases (bn254_g{1,2}_msm_prepare / _prepared) against bn254_g{1,2}_msm_dev - the parent's
route - on one GPU, one process, device-resident inputs (distinct points with z != 1 made by the reference chain, distinct full-width
scalars).  Every row is KERNEL ms between the events of the call's scopes (bn254_kernel_stats, summed): the median, minimum and maximum
over --repeats runs after --warmup, the candidates of a size alternating inside one repetition loop, and the bytes of every candidate are
asserted equal to those of bn254_g{1,2}_msm_dev on the same raw points and scalars.
  --widths      the prepared bucket route at c = 10 .. 16 for G1 2^16 / 2^18 / 2^20 / 2^22 and G2 2^15 / 2^18 / 2^20: per width the time,
                the shares of digits / bucket / reduce / tail, the build time and the bytes of the handle; the best width per size
  --crossover   every power of two from 2^10 to 2^20 at the handle's DEFAULT width: the prepared bucket route, the small route on the
                handle's points and the parent's call; the smallest size from which the bucket route's [min, max] lies wholly below the
                small route's at that size and at every larger one
  --equal       all-equal scalars at 2^20 (every term in one bucket per window)
  --wall        wall ms of groth16.prove (4096 constraints, domain 4096) and kzg.commit (2^16 coefficients) with the plain and with the
                prepared key, host buffers as their callers pass them
usage: tools/time_msm_prepared.py [--widths] [--crossover] [--equal] [--wall] [--groups 1,2] [--repeats 5] [--warmup 1]"""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
NEW = ("digits", "bucket", "reduce")
WIDTH_SIZES = {1: (16, 18, 20, 22), 2: (15, 18, 20)}


def inputs(te, g, n, equal=False):
    import torch
    from bn_amd import distributed as D
    g1, g2 = D.generator_limbs()
    gen = torch.from_numpy(np.ascontiguousarray(g1 if g == 1 else g2).view(np.int64)).to(te.device)
    P = te.empty(n, 12 if g == 1 else 24)
    step = 1 << 20                                                    # the term kernels' scratch is sized per call: make the points in parts
    for lo in range(0, n, step):
        cnt = min(step, n - lo)
        kb = D.synthetic_scalars_device(te, lo, lo + cnt, g - 1)
        base = te.empty(cnt, P.shape[1])
        te.e.tile_dev(gen.data_ptr(), 96 if g == 1 else 192, cnt, base.data_ptr(), te._stream())
        P[lo:lo + cnt] = (te.g1_mul if g == 1 else te.g2_mul)(base, kb, normalize=False)
    k = D.synthetic_scalars_device(te, 1 << 24, (1 << 24) + n, 1)
    if equal:
        k = k[:1].repeat(n, 1).contiguous()
    torch.cuda.synchronize()
    return P, k


def scopes(eng, g):
    per = {"p_" + s: eng.kernel_stats(f"g{g}_msmp_{s}")[0] for s in NEW}
    per.update({s: eng.kernel_stats(f"g{g}_msm_{s}")[0] for s in NEW + ("mul", "fold")})
    return per


def timed(eng, g, call):
    import torch
    eng.profile(True); eng.profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    per = scopes(eng, g)
    eng.profile(False)
    return sum(per.values()), wall, per


def build(eng, te, g, P, n, c):
    """(handle, kernel ms of the build: the table scopes and the normalisations, wall ms)"""
    import torch
    eng.profile(True); eng.profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = (eng.g1_msm_prepare_dev if g == 1 else eng.g2_msm_prepare_dev)(P.data_ptr(), n, c, te._stream())
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    ms = eng.kernel_stats(f"g{g}_msmp_table")[0] + eng.kernel_stats(f"g{g}_normalize")[0]
    eng.profile(False)
    return h, ms, wall


def fmt(v):
    return "%8.3f [%7.3f %7.3f]" % (statistics.median(v), min(v), max(v))


def shares(per):
    tail = per["mul"] + per["fold"]
    total = per["p_digits"] + per["p_bucket"] + per["p_reduce"] + tail
    if not per["p_reduce"]:
        return "mul %.3f  fold %.3f" % (per["mul"], per["fold"]) + ("  digits %.3f  bucket %.3f  reduce %.3f" % (per["digits"], per["bucket"], per["reduce"]) if per["reduce"] else "")
    return "digits %.3f (%2.0f%%)  bucket %.3f (%2.0f%%)  reduce %.3f (%2.0f%%)  tail %.3f (%2.0f%%)" % (
        per["p_digits"], 100 * per["p_digits"] / total, per["p_bucket"], 100 * per["p_bucket"] / total, per["p_reduce"], 100 * per["p_reduce"] / total, tail, 100 * tail / total)


def measure(eng, te, g, n, handles, repeats, warmup, tag, small=False, equal=False, PK=None):
    """handles: {name: PreparedMSM}; candidates: every handle on the bucket route (msm_bucket_min = 0), with small=True every handle on the
    small route as well (msm_bucket_min above n), and the parent's call with default options -> {name: [(kernel ms, wall ms, per scope)]}"""
    import torch
    P, k = PK
    out = {}
    call_p = eng.g1_msm_prepared_dev if g == 1 else eng.g2_msm_prepared_dev
    parent = eng.g1_msm_dev if g == 1 else eng.g2_msm_dev
    names = list(handles) + (["small"] if small else []) + ["parent"]
    runs = {nm: [] for nm in names}
    first = next(iter(handles.values()))
    for rep in range(warmup + repeats):
        for nm in names:
            o = out.setdefault(nm, te.empty(1, P.shape[1]))
            if nm == "parent":
                opts, fn = {}, (lambda: parent(P.data_ptr(), k.data_ptr(), n, o.data_ptr(), te._stream()))
            elif nm == "small":
                opts, fn = {"msm_bucket_min": n + 1}, (lambda: call_p(first, 0, k.data_ptr(), n, o.data_ptr(), te._stream()))
            else:
                opts, fn = {"msm_bucket_min": 0}, (lambda h=handles[nm]: call_p(h, 0, k.data_ptr(), n, o.data_ptr(), te._stream()))
            with eng.options(**opts):
                r = timed(eng, g, fn)
            if rep >= warmup:
                runs[nm].append(r)
    torch.cuda.synchronize()
    for nm in names:
        assert torch.equal(out[nm], out["parent"]), (g, n, nm)              # equal bytes in every row
    for nm in names:
        rs = sorted(runs[nm], key=lambda r: r[0])
        print("G%d n=2^%-2d %-5s %-8s | kernel ms %s | wall ms %s | %s" % (g, n.bit_length() - 1, tag, nm, fmt([r[0] for r in rs]), fmt([r[1] for r in rs]), shares(rs[len(rs) // 2][2])),
              flush=True)
    return runs


def widths(eng, te, groups, repeats, warmup):
    best = {}
    for g in groups:
        for lg in WIDTH_SIZES[g]:
            n = 1 << lg
            PK = inputs(te, g, n)
            handles = {}
            for c in range(10, 17):
                h, ms, wall = build(eng, te, g, PK[0], n, c)
                handles[f"c={c}"] = h
                print("G%d n=2^%-2d build c=%-2d | kernel ms %9.3f | wall ms %9.3f (allocation included) | %6.1f MB in %d windows" % (g, lg, c, ms, wall, h.device_bytes / 1e6, h.windows), flush=True)
            runs = measure(eng, te, g, n, handles, repeats, warmup, "rand", PK=PK)
            km = {nm: statistics.median(r[0] for r in rs) for nm, rs in runs.items()}
            b = min((nm for nm in km if nm.startswith("c=")), key=lambda nm: km[nm])
            best[(g, lg)] = int(b[2:])
            print("G%d n=2^%-2d best %s: parent / best = %.2f  (parent %.3f ms, best %.3f ms)" % (g, lg, b, km["parent"] / km[b], km["parent"], km[b]), flush=True)
            for h in handles.values():
                h.close()
            del PK
    print("# width table (the width with the smallest median per size): " + ", ".join("G%d 2^%d: %d" % (g, lg, c) for (g, lg), c in best.items()))


def crossover(eng, te, groups, repeats, warmup):
    for g in groups:
        rows = {}
        for lg in range(10, 21):
            n = 1 << lg
            PK = inputs(te, g, n)
            h, ms, wall = build(eng, te, g, PK[0], n, None)
            print("G%d n=2^%-2d build c=%-2d (default) | kernel ms %9.3f | wall ms %9.3f | %6.1f MB" % (g, lg, h.window_bits, ms, wall, h.device_bytes / 1e6), flush=True)
            runs = measure(eng, te, g, n, {"buckets": h}, repeats, warmup, "rand", small=True, PK=PK)
            rows[lg] = {nm: (min(r[0] for r in rs), statistics.median(r[0] for r in rs), max(r[0] for r in rs)) for nm, rs in runs.items()}
            h.close()
            del PK
        below = [rows[lg]["buckets"][2] < rows[lg]["small"][0] for lg in range(10, 21)]
        cross = next((10 + i for i in range(len(below)) if all(below[i:])), None)
        print("# G%d crossover: %s" % (g, "never (at no measured size does the bucket route's [min, max] stay wholly below the small route's from there on)" if cross is None else
                                       "2^%d (from there on the bucket route's [min, max] lies wholly below the small route's at every measured size)" % cross))
        for lg in range(10, 21):
            r = rows[lg]
            print("# G%d 2^%-2d  buckets / small = %.2f   parent / buckets = %.2f   parent / small = %.2f" % (g, lg, r["buckets"][1] / r["small"][1], r["parent"][1] / r["buckets"][1],
                                                                                                          r["parent"][1] / r["small"][1]))


def equal(eng, te, groups, repeats, warmup):
    for g in groups:
        n = 1 << 20
        PK = inputs(te, g, n, equal=True)
        h, ms, wall = build(eng, te, g, PK[0], n, None)
        measure(eng, te, g, n, {f"c={h.window_bits}": h}, repeats, warmup, "equal", PK=PK)
        h.close()


def wall(eng, repeats):
    import dot_cases as DC
    import fr_cases as FC
    from bn_amd import groth16, kzg

    def med(fn):
        fn()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return r, ts

    rows, l = 4096, 2
    _, nv, a, b, c, z = DC.r1cs(rows, l, [1, 2, 3], seed=29)
    mat = lambda m: (np.array(m[0], np.uint64), np.array(m[1], np.uint64), FC.rows(m[2]))
    system = groth16.R1CS(l, nv, mat(a), mat(b), mat(c))
    Z = FC.rows(z)
    pk, vk = groth16.setup(system, np.random.default_rng(1), engine=eng)
    t0 = time.perf_counter(); ppk = groth16.prepare_proving_key(pk, engine=eng); prep_ms = (time.perf_counter() - t0) * 1e3
    p1, t1 = med(lambda: groth16.prove(pk, system, Z, np.random.default_rng(2), engine=eng))
    p2, t2 = med(lambda: groth16.prove(ppk, system, Z, np.random.default_rng(2), engine=eng))
    assert all(np.array_equal(x.limbs, y.limbs) for x, y in zip(p1, p2))
    print("groth16.prove, %d constraints, %d variables, domain %d | wall ms plain key %s | prepared key %s | prepare_proving_key once %.1f ms, %.1f MB" % (
        rows, nv, 1 << 12, fmt(t1), fmt(t2), prep_ms, sum(h.device_bytes for h in ppk.prepared.values()) / 1e6), flush=True)
    n = 1 << 16
    srs = kzg.setup(n, np.random.default_rng(3), engine=eng)
    t0 = time.perf_counter(); psrs = kzg.prepare(srs, engine=eng); prep_ms = (time.perf_counter() - t0) * 1e3
    coeffs = np.frombuffer(np.random.default_rng(4).bytes(n * 32), np.uint64).reshape(n, 4).copy()
    coeffs[:, 3] &= (1 << 59) - 1
    c1, t1 = med(lambda: kzg.commit(srs, coeffs, engine=eng))
    c2, t2 = med(lambda: kzg.commit(psrs, coeffs, engine=eng))
    assert np.array_equal(c1.limbs, c2.limbs)
    print("kzg.commit, 2^16 coefficients | wall ms plain string %s | prepared string %s | kzg.prepare once %.1f ms, %.1f MB (c = %d)" % (
        fmt(t1), fmt(t2), prep_ms, psrs.prepared.device_bytes / 1e6, psrs.prepared.window_bits), flush=True)
    with eng.options(msm_bucket_min=0):
        c3, t3 = med(lambda: kzg.commit(psrs, coeffs, engine=eng))
    assert np.array_equal(c1.limbs, c3.limbs)
    print("kzg.commit, 2^16 coefficients | wall ms prepared string, bucket route forced %s" % fmt(t3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    for m in ("widths", "crossover", "equal", "wall"):
        ap.add_argument("--" + m, action="store_true")
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import _native
    from bn_amd import distributed as D
    eng = bn_amd.Engine(0)
    te = D.TorchEngine(eng, torch.device("cuda", 0))
    groups = [int(x) for x in a.groups.split(",")]
    lib = _native.lib()
    print("kernel / wall ms: median [min max] over %d runs after %d warm-up, candidates interleaved; bytes equal to bn254_g*_msm_dev asserted in every row" % (a.repeats, a.warmup))
    print("shipped defaults: crossover G1 %d, G2 %d; width by size " % (lib.bn254_msm_prepared_default_min(1), lib.bn254_msm_prepared_default_min(2)) +
          ", ".join("2^%d: %d" % (lg, lib.bn254_msm_prepared_default_window_bits(1 << lg)) for lg in range(10, 23, 2)))
    if a.widths:
        widths(eng, te, groups, a.repeats, a.warmup)
    if a.crossover:
        crossover(eng, te, groups, a.repeats, a.warmup)
    if a.equal:
        equal(eng, te, groups, a.repeats, a.warmup)
    if a.wall:
        wall(eng, a.repeats)


if __name__ == "__main__":
    main()
