#!/usr/bin/env python3
"""Batched multi-pairing (bn254_pairing_product_batch) against what a caller does without it, on one GPU.
For every shape (segments x pairs per segment): kernel ms (the sum of bn254_kernel_stats over every scope of the call) of
bn254_pairing_product_batch_dev against bn254_pairing_batch_dev on the same device-resident pairs (one final exponentiation per PAIR; one
stream each - the host entry point of pairing_batch overlaps two streams, so its summed kernel ms would overstate the device time), and
wall ms of the host entry points: pairing_product_batch (with its kernel ms), pairing_batch and - for small shapes - one
bn254_pairing_product call per segment.  Every shape is warmed up first; then the sides alternate inside the same process and the median
of --repeats runs is printed, with the kernel ms per scope of pairing_product_batch_dev.  --dev-only alternates the two device-resident
sides alone, without the host-buffer calls in between.
usage: tools/time_product_batch.py [--repeats 5] [--shapes 8x4,65536x4,...] [--dev-only]"""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SCOPES = ["miller", "miller_shared", "miller_wave", "miller_quad", "pairing_wave", "final_exp", "final_exp_wave", "final_exp_quad",
          "gt_product", "gt_tail", "gt_segment", "gt_tail_seg"]
SHAPES = "8x4,64x4,1024x4,16384x4,65536x4,3584x1,65536x1,16x300,1x5000"


def pool(eng, n, rng):
    from bn_amd.api import G1, G2, Fr
    k1 = np.stack([Fr.random(rng).limbs for _ in range(n)]); k2 = np.stack([Fr.random(rng).limbs for _ in range(n)])
    return eng.g1_mul_batch(np.tile(G1.one().limbs, (n, 1)), k1), eng.g2_mul_batch(np.tile(G2.one().limbs, (n, 1)), k2)


def measure(eng, fn):
    """(kernel ms, wall ms) of one call"""
    eng.profile_reset()
    t = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t) * 1e3
    per = {s: eng.kernel_stats(s)[0] for s in SCOPES}
    return sum(per.values()), wall, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--dev-only", action="store_true", help="time only pairing_product_batch_dev and pairing_batch_dev")
    a = ap.parse_args()
    import torch
    import bn_amd
    eng = bn_amd.Engine(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    P0, Q0 = pool(eng, 4096, rng)
    eng.profile(True)
    print("shape (segments x pairs)       | kernel ms: product_batch_dev  pairing_batch_dev  ratio | product_batch kernel / wall ms | "
          "pairing_batch wall ms | per-product calls wall ms | product_batch_dev scopes (kernel ms)")
    for shape in a.shapes.split(","):
        m, k = (int(x) for x in shape.split("x"))
        n = m * k
        idx = rng.integers(0, P0.shape[0], n)
        P, Q = P0[idx], Q0[idx]
        offs = np.arange(m + 1, dtype=np.uint64) * k
        dp = torch.from_numpy(np.ascontiguousarray(P).view(np.int64)).to(dev)
        dq = torch.from_numpy(np.ascontiguousarray(Q).view(np.int64)).to(dev)
        dout = torch.empty((n, 48), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)

        def batch_dev():
            eng.pairing_product_batch_dev(dp.data_ptr(), dq.data_ptr(), offs, dout.data_ptr(), stream.cuda_stream)
            stream.synchronize()

        def pairs_dev():
            eng.pairing_batch_dev(dp.data_ptr(), dq.data_ptr(), dout.data_ptr(), n, stream.cuda_stream)
            stream.synchronize()
        sides = {"batch_dev": batch_dev, "pairs_dev": pairs_dev}
        if not a.dev_only:
            sides.update(batch=lambda: eng.pairing_product_batch(P, Q, offs), pairs=lambda: eng.pairing_batch(P, Q))
        if m <= 64 and not a.dev_only:
            sides["calls"] = lambda: [eng.pairing_product(P[j * k:(j + 1) * k], Q[j * k:(j + 1) * k]) for j in range(m)]
        for fn in sides.values():                      # warm-up: buffers, code, tables
            fn()
        res = {s: [] for s in sides}
        for _ in range(a.repeats):
            for s, fn in sides.items():
                res[s].append(measure(eng, fn))
        med = {s: (statistics.median(r[0] for r in v), statistics.median(r[1] for r in v)) for s, v in res.items()}
        scopes = {sc: statistics.median(r[2][sc] for r in res["batch_dev"]) for sc in SCOPES}
        scopes = ", ".join(f"{sc} {ms:.3f}" for sc, ms in scopes.items() if ms > 0)
        calls = f"{med['calls'][1]:9.3f}" if "calls" in med else "        -"
        host = (f"{med['batch'][0]:9.3f} / {med['batch'][1]:9.3f} | {med['pairs'][1]:9.3f}" if "batch" in med else "        - /         - |         -")
        print(f"{m:7d} x {k:4d} = {n:7d} pairs | {med['batch_dev'][0]:9.3f} {med['pairs_dev'][0]:9.3f} {med['batch_dev'][0] / med['pairs_dev'][0]:6.3f} "
              f"| {host} | {calls} | {scopes}", flush=True)
    eng.profile(False)


if __name__ == "__main__":
    main()
