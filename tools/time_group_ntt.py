#!/usr/bin/env python3
"""Transforms over G1 and G2 (bn254_g{1,2}_ntt_batch) on one GPU, one process; every figure is the median [min max] of --repeats runs after
--warmup.
  kernel    kernel ms (bn254_kernel_stats "g*_ntt" + "g*_ntt_scale" + "g*_ntt_normalize") of the _dev call for one forward transform without
            a shift: G1 at 2^10, 2^16, 2^20 and G2 at 2^10, 2^15, 2^18, each beside
              - the chain floor: n / 2 (log_n - 1) multiplications through bn254_g*_mul_batch_dev (log_n - 1 calls of n / 2), kernel ms
              - the same transform composed per stage from the calls the engine had before: one g*_mul_batch and two g*_add_batch on views
                gathered on the host, one g*_normalize at the end - kernel ms of their scopes and wall ms; equal bytes asserted
  passes    the inverse and the coset forms at the middle size
  fk20      bn_amd.kzg.open_all at n = 2^10 against n calls of kzg.open, wall ms
Everything printed is also written to --out (default profiles/r28_group_ntt.txt).
usage: tools/time_group_ntt.py [--repeats 5] [--warmup 1] [--g1 10,16,20] [--g2 10,15,18] [--compose-max 20]"""
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


def say(line):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def fmt(v):
    return "%10.3f [%10.3f %10.3f]" % (statistics.median(v), min(v), max(v))


def repeat(fn, repeats, warmup):
    out = []
    for rep in range(warmup + repeats):
        r = fn()
        if rep >= warmup:
            out.append(r)
    return out


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--g1", default="10,16,20")
    ap.add_argument("--g2", default="10,15,18")
    ap.add_argument("--compose-max", type=int, default=20, help="largest log_n the per-stage composition is run at")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r28_group_ntt.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import Fr, G1, G2, _native, kzg, poly
    OUT = open(a.out, "w")
    lib = _native.lib()
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    s0 = torch.cuda.current_stream().cuda_stream
    say("shipped library; median [min max] over %d runs after %d warm-up, one process; forward, no shift unless said" % (a.repeats, a.warmup))

    def kernel_ms(scopes, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        ms = sum(eng.kernel_stats(s)[0] for s in scopes)
        eng.profile(False)
        return ms

    for g, lgs in ((1, [int(x) for x in a.g1.split(",")]), (2, [int(x) for x in a.g2.split(",")])):
        words = 12 if g == 1 else 24
        gen = (G1 if g == 1 else G2).one().limbs
        nmax = 1 << max(lgs)
        K = torch.empty(nmax * 4, dtype=torch.int64, device=dev)
        P = torch.empty(nmax * words, dtype=torch.int64, device=dev); O = torch.empty_like(P)
        eng.synthetic_scalars_dev(7 + g, 0, nmax, 0, K.data_ptr(), s0)
        (eng.g1_mul_base_batch_dev if g == 1 else eng.g2_mul_base_batch_dev)(gen, K.data_ptr(), P.data_ptr(), nmax, s0)      # points: random multiples of the generator
        torch.cuda.synchronize()
        ntt_dev = eng.g1_ntt_batch_dev if g == 1 else eng.g2_ntt_batch_dev
        mul_dev = lib.bn254_g1_mul_batch_dev if g == 1 else lib.bn254_g2_mul_batch_dev
        scopes = ["g%d_ntt" % g, "g%d_ntt_scale" % g, "g%d_ntt_normalize" % g]
        old_scopes = ["g%d_mul" % g, "g%d_add" % g, "g%d_normalize" % g]
        mul_h = eng.g1_mul_batch if g == 1 else eng.g2_mul_batch
        add_h = eng.g1_add_batch if g == 1 else eng.g2_add_batch
        norm_h = eng.g1_normalize if g == 1 else eng.g2_normalize
        say("-- G%d: kernel ms of the _dev call, out of place" % g)

        def composed(hp, lg):
            """the route there was before: per stage the twiddle products in one call, sum and difference in two, gathers on the host"""
            n = 1 << lg
            cur = hp
            bf = np.arange(n // 2)
            for i in range(lg):
                lr = lg - 1 - i
                rho, k = bf & ((1 << lr) - 1), bf >> lr
                ia = rho + (k << (lr + 1))
                t = cur[ia + (1 << lr)]
                if i:
                    tw = np.repeat(poly.powers(Fr.root_of_unity(i + 1), 1 << i, engine=eng, limbs=True), 1 << lr, axis=0)
                    t = mul_h(t, tw)
                x = cur[ia]
                cur = np.concatenate([add_h(x, t), add_h(x, t, negate_b=True)])
            return norm_h(cur)

        for lg in lgs:
            n = 1 << lg
            label = "G%d 2^%-2d" % (g, lg)
            v = repeat(lambda: kernel_ms(scopes, lambda: ntt_dev(P.data_ptr(), O.data_ptr(), lg, 1, False, None, s0)), a.repeats, a.warmup)
            med = statistics.median(v)
            chains = n // 2 * (lg - 1)

            def floor():
                def calls():
                    for _ in range(lg - 1):
                        assert mul_dev(eng._h, P.data_ptr(), K.data_ptr(), O.data_ptr(), n // 2, s0) == 0
                return kernel_ms(old_scopes[:1], calls)
            f = repeat(floor, a.repeats, a.warmup)
            fmed = statistics.median(f)
            say("%s transform            | kernel ms %s | %8.2f M butterflies/s" % (label, fmt(v), n // 2 * lg / med / 1e3))
            say("%s chain floor          | kernel ms %s | %d multiplications in %d calls of n / 2 (normalising kernel), %.1f M/s | transform = %.2f x the floor"
                % (label, fmt(f), chains, lg - 1, chains / fmed / 1e3, med / fmed))
            if lg > a.compose_max:
                say("%s composed per stage   | not run above 2^%d" % (label, a.compose_max))
                continue
            hp = P[:n * words].cpu().numpy().view(np.uint64).reshape(n, words)
            ntt_dev(P.data_ptr(), O.data_ptr(), lg, 1, False, None, s0); torch.cuda.synchronize()
            mine = O[:n * words].cpu().numpy().view(np.uint64).reshape(n, words)
            assert composed(hp, lg).tobytes() == mine.tobytes(), ("the composition and the transform differ", g, lg)
            reps = a.repeats if lg <= 16 else 1
            walls = []

            def comp():
                t0 = time.perf_counter()
                ms = kernel_ms(old_scopes, lambda: composed(hp, lg))
                walls.append((time.perf_counter() - t0) * 1e3)
                return ms
            c = repeat(comp, reps, a.warmup if lg <= 16 else 0)
            walls = walls[-reps:]

            def mine_wall():
                t0 = time.perf_counter()
                (eng.g1_ntt_batch if g == 1 else eng.g2_ntt_batch)(hp, lg)
                return (time.perf_counter() - t0) * 1e3
            w = repeat(mine_wall, reps, a.warmup if lg <= 16 else 0)
            say("%s composed per stage   | kernel ms %s | wall ms %s | equal bytes | transform = %.2f x its kernel time (%d run%s)"
                % (label, fmt(c), fmt(walls), med / statistics.median(c), reps, "" if reps == 1 else "s"))
            say("%s host-buffer call     | wall ms %s | %.2f x the wall time of the composition" % (label, fmt(w), statistics.median(w) / statistics.median(walls)))
        lg = lgs[len(lgs) // 2]
        five = Fr(5).limbs
        for name, inverse, shift in (("inverse", True, None), ("coset forward", False, five), ("coset inverse", True, five)):
            v = repeat(lambda: kernel_ms(scopes, lambda: ntt_dev(P.data_ptr(), O.data_ptr(), lg, 1, inverse, shift, s0)), a.repeats, a.warmup)
            say("G%d 2^%-2d %-20s | kernel ms %s | one pass of n chains more than forward" % (g, lg, name, fmt(v)))
        del K, P, O

    say("-- kzg.open_all at n = 2^10 against n calls of kzg.open, wall ms")
    n, lg = 1 << 10, 10
    srs = kzg.setup(n, np.random.default_rng(28))
    rng = np.random.default_rng(29)
    p = [Fr(int.from_bytes(rng.bytes(64), "little") % bn_amd.api.R_MOD) for _ in range(n)]
    w = Fr.root_of_unity(lg).v
    zs = [Fr(pow(w, m, bn_amd.api.R_MOD)) for m in range(n)]

    def all_once():
        t0 = time.perf_counter()
        out = kzg.open_all(srs, p, lg)
        return (time.perf_counter() - t0) * 1e3, out
    runs = repeat(all_once, a.repeats, a.warmup)
    t0 = time.perf_counter()
    singles = [kzg.open(srs, p, z) for z in zs]
    one_by_one = (time.perf_counter() - t0) * 1e3
    ys, proofs = runs[-1][1]
    assert all(ys[m] == singles[m][0] for m in range(n))
    assert np.stack([x.limbs for x in proofs]).tobytes() == eng.g1_normalize(np.stack([s[1].limbs for s in singles])).tobytes()
    va = [r[0] for r in runs]
    say("open_all (3 transforms over G1 of 2^11, 2^11, 2^10; 2 over Fr; one g1_mul_batch; Python objects out) | wall ms %s" % fmt(va))
    say("%d x open (a scan and a multi-scalar multiplication each), one run                                  | wall ms %10.3f | %.1f x open_all | equal bytes"
        % (n, one_by_one, one_by_one / statistics.median(va)))


if __name__ == "__main__":
    main()
