#!/usr/bin/env python3
"""Batched multi-pairing over prepared points (bn254_pairing_product_batch_prepared_native_dev) against bn254_pairing_product_batch_dev on the
SAME pairs, in the same process, alternating - blocks of m Groth16-shaped checks (four pairs, G2 indices [3 + j, 0, 1, 2] over a handle
[K0, K1, K2, B_0 .. B_{m-1}]), device-resident inputs.
Three sides per alternation: `general` (pairing_product_batch_dev on the gathered G2 points - the baseline), `prepared` (the new call over a
handle made beforehand) and `prepare+prepared` (bn254_g2_prepare_dev of the m + 3 points, the new call, the handle destroyed: what
groth16.verify_batch(prepared=True) pays per block).  Kernel ms = the sum of bn254_kernel_stats over every scope of the side, wall ms =
host time around the call(s) including the stream synchronisation.  Every alternation is printed (the acceptance rule asks for every one of
at least three), then the medians and the new call's kernel ms per scope.
usage: tools/time_product_batch_prepared.py [--repeats 5] [--checks 8,1024,65536]"""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SCOPES = ["miller", "miller_shared", "miller_wave", "miller_quad", "pairing_wave", "final_exp", "final_exp_wave", "final_exp_quad", "gt_product", "gt_tail",
          "gt_segment", "gt_tail_seg", "g2_prepare_native", "miller_native", "miller_native_shared", "miller_native_seg", "g2_gather"]


def pool(eng, n, rng):
    from bn_amd.api import G1, G2, Fr
    k1 = np.stack([Fr.random(rng).limbs for _ in range(n)]); k2 = np.stack([Fr.random(rng).limbs for _ in range(n)])
    return eng.g1_mul_batch(np.tile(G1.one().limbs, (n, 1)), k1), eng.g2_mul_batch(np.tile(G2.one().limbs, (n, 1)), k2)


def measure(eng, fn):
    """(kernel ms, wall ms, kernel ms per scope) of one call"""
    eng.profile_reset()
    t = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t) * 1e3
    per = {s: eng.kernel_stats(s)[0] for s in SCOPES}
    return sum(per.values()), wall, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--checks", default="8,1024,65536")
    a = ap.parse_args()
    import torch
    import bn_amd
    eng = bn_amd.Engine(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    P0, Q0 = pool(eng, 4096, rng)
    eng.profile(True)
    for m in (int(x) for x in a.checks.split(",")):
        n = 4 * m
        P = P0[rng.integers(0, P0.shape[0], n)]
        H = np.concatenate([Q0[:3], Q0[rng.integers(0, Q0.shape[0], m)]])                 # the handle's points: key, then one B per check
        qi = np.empty((m, 4), np.uint64)
        qi[:, 0] = 3 + np.arange(m); qi[:, 1:] = np.arange(3)
        qi = qi.reshape(-1)
        offs = np.arange(m + 1, dtype=np.uint64) * 4
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
        dp, dq, dh, dqi = t(P), t(H[qi.astype(np.int64)]), t(H), t(qi)
        out_g = torch.empty((m, 48), dtype=torch.int64, device=dev); out_p = torch.empty_like(out_g); out_pp = torch.empty_like(out_g)
        stream = torch.cuda.current_stream(dev)
        handle = eng.g2_prepare_dev(dh.data_ptr(), m + 3, stream.cuda_stream)
        stream.synchronize()

        def general():
            eng.pairing_product_batch_dev(dp.data_ptr(), dq.data_ptr(), offs, out_g.data_ptr(), stream.cuda_stream)
            stream.synchronize()

        def prepared():
            eng.pairing_product_batch_prepared_native_dev(dp.data_ptr(), handle, offs, out_p.data_ptr(), dqi.data_ptr(), stream.cuda_stream)
            stream.synchronize()

        def prepare_and_prepared():
            h = eng.g2_prepare_dev(dh.data_ptr(), m + 3, stream.cuda_stream)
            eng.pairing_product_batch_prepared_native_dev(dp.data_ptr(), h, offs, out_pp.data_ptr(), dqi.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            h.close()
        sides = {"general": general, "prepared": prepared, "prepare+prepared": prepare_and_prepared}
        for fn in sides.values():                      # warm-up: buffers, code, tables
            fn()
        assert torch.equal(out_g, out_p) and torch.equal(out_g, out_pp), "the sides disagree"
        res = {s: [] for s in sides}
        print(f"--- {m} checks x 4 pairs = {n} pairs (handle of {m + 3} points)")
        for r in range(a.repeats):
            for s, fn in sides.items():
                res[s].append(measure(eng, fn))
            g, p, pp = (res[s][-1] for s in sides)
            print(f"alternation {r}: kernel ms  general {g[0]:8.3f}  prepared {p[0]:8.3f} ({p[0] / g[0]:5.3f} x)  prepare+prepared {pp[0]:8.3f} ({pp[0] / g[0]:5.3f} x)"
                  f" | wall ms  general {g[1]:8.3f}  prepared {p[1]:8.3f}  prepare+prepared {pp[1]:8.3f}", flush=True)
        for s in sides:
            k = statistics.median(x[0] for x in res[s]); w = statistics.median(x[1] for x in res[s])
            scopes = {sc: statistics.median(x[2][sc] for x in res[s]) for sc in SCOPES}
            print(f"median {s:17s}: kernel {k:8.3f} ms  wall {w:8.3f} ms | " + ", ".join(f"{sc} {ms:.3f}" for sc, ms in scopes.items() if ms > 0), flush=True)
        handle.close()
    eng.profile(False)


if __name__ == "__main__":
    main()
