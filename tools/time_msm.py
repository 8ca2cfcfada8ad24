#!/usr/bin/env python3
"""Segmented multi-scalar multiplication (bn254_g{1,2}_msm_batch) against the composition a caller writes without it, on one GPU, host
buffers on both sides:
    composition = g*_mul_batch of every term (normalises every term)  ->  level-wise g*_add_batch over the terms of each segment
                  (ceil(log2 L) calls)  ->  g*_mul_batch of the sums by Fr::one() (normalises them)
For every shape (segments x terms per segment) both sides are warmed up, then alternate inside the same process; the median wall ms of
--repeats runs of each, their ratio (the condition is new / composition < 0.97), and the kernel-time split of the new call
(g*_msm_mul / g*_msm_fold from bn254_kernel_stats) beside g*_mul of bn254_g*_mul_batch_dev on the same terms.
--build-sweep W1,W2,...  (no GPU needed) builds build_variants/lib_msmfold_W.so: the library with BN_MSM_FOLD = W (only bn254_seg.hip is
                         recompiled, from a copy with the constant replaced; the other objects come from the last regular build)
--sweep W1,W2,...        runs the shapes once per such library, each in a child process of its own, and prints one table per width
usage: tools/time_msm.py [--repeats 7] [--shapes 64x9,16384x16] [--groups 1,2] [--sweep 4,8,16,32]"""
import argparse
import os
import pathlib
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SHAPES = "64x9,16384x16"
VARIANTS = ROOT / "build_variants"


def build_sweep(widths):
    from bn_amd import _native
    _native.build()
    VARIANTS.mkdir(exist_ok=True)
    src = (_native.HERE / "csrc" / "bn254_seg.hip").read_text()
    pat = r"constexpr size_t BN_MSM_FOLD = \d+;"
    assert len(re.findall(pat, src)) == 1
    flags = (_native.OBJ_DIR / "flags.txt").read_text().split()
    for w in widths:
        unit = _native.HERE / "csrc" / f"_msmfold_{w}.hip"            # beside the original: it includes its headers by relative path
        obj = VARIANTS / f"bn254_seg_msmfold_{w}.o"
        try:
            unit.write_text(re.sub(pat, f"constexpr size_t BN_MSM_FOLD = {w};", src))
            subprocess.check_call(flags + ["-c", str(unit), "-o", str(obj)])
        finally:
            unit.unlink(missing_ok=True)
        objs = [str(obj if s.stem == "bn254_seg" else _native.OBJ_DIR / (s.stem + ".o")) for s in _native.SOURCES]
        so = VARIANTS / f"lib_msmfold_{w}.so"
        subprocess.check_call([_native.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-lpthread", "-o", str(so)])
        obj.unlink()
        print("built", so.relative_to(ROOT))


def composition(eng, g, P, K, m, L, one):
    mul, add = (eng.g1_mul_batch, eng.g1_add_batch) if g == 1 else (eng.g2_mul_batch, eng.g2_add_batch)
    zero = np.zeros(P.shape[1], np.uint64); zero[P.shape[1] // 3:P.shape[1] // 3 + 4] = one_fq()
    t = mul(P, K).reshape(m, L, -1)
    while t.shape[1] > 1:
        if t.shape[1] % 2:
            t = np.concatenate([t, np.broadcast_to(zero, (m, 1, t.shape[2]))], axis=1)
        a = np.ascontiguousarray(t[:, 0::2]).reshape(-1, t.shape[2]); b = np.ascontiguousarray(t[:, 1::2]).reshape(-1, t.shape[2])
        t = add(a, b).reshape(m, -1, t.shape[2])
    return mul(t.reshape(m, -1), one)


def one_fq():
    from bn_amd.api import _one_fq
    return _one_fq()


def run(a):
    import torch
    import bn_amd
    from bn_amd.api import G1, G2, Fr
    eng = bn_amd.Engine(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    print("group shape (segments x terms)   | wall ms: msm_batch  composition  ratio | kernel ms: msm_mul  msm_fold  | mul_batch_dev on the same terms (g*_mul) "
          "| fold share of msm  saved vs g*_mul")
    worst = 0.0
    for g in (int(x) for x in a.groups.split(",")):
        G, words = (G1, 12) if g == 1 else (G2, 24)
        pool_k = np.stack([Fr.random(rng).limbs for _ in range(4096)])
        pool = (eng.g1_mul_batch if g == 1 else eng.g2_mul_batch)(np.tile(G.one().limbs, (4096, 1)), pool_k)
        msm = eng.g1_msm_batch if g == 1 else eng.g2_msm_batch
        mul_dev = eng.g1_mul_dev if g == 1 else eng.g2_mul_dev
        for shape in a.shapes.split(","):
            m, L = (int(x) for x in shape.split("x"))
            n = m * L
            P = pool[rng.integers(0, 4096, n)]
            K = np.frombuffer(rng.bytes(n * 32), np.uint64).reshape(n, 4).copy()
            K[:, 3] &= (1 << 59) - 1                         # below r: canonical Montgomery images of some scalars
            offs = np.arange(m + 1, dtype=np.uint64) * L
            one = np.tile(Fr.one().limbs, (m, 1))
            dp = torch.from_numpy(P.view(np.int64)).to(dev); dk = torch.from_numpy(K.view(np.int64)).to(dev); dout = torch.empty_like(dp)
            stream = torch.cuda.current_stream(dev)

            def new(): return msm(P, K, offs)
            def old(): return composition(eng, g, P, K, m, L, one)
            def plain():
                mul_dev(dp.data_ptr(), dk.data_ptr(), dout.data_ptr(), n, stream.cuda_stream); stream.synchronize()
            assert np.array_equal(new(), old())              # warm-up of both sides, and they agree
            plain()
            eng.profile(True)
            res = {"new": [], "old": [], "mul": [], "fold": [], "plain": []}
            for _ in range(a.repeats):
                eng.profile_reset()
                t = time.perf_counter(); new(); res["new"].append((time.perf_counter() - t) * 1e3)
                res["mul"].append(eng.kernel_stats(f"g{g}_msm_mul")[0]); res["fold"].append(eng.kernel_stats(f"g{g}_msm_fold")[0])
                t = time.perf_counter(); old(); res["old"].append((time.perf_counter() - t) * 1e3)
                eng.profile_reset()
                plain(); res["plain"].append(eng.kernel_stats(f"g{g}_mul")[0])
            eng.profile(False)
            md = {k: statistics.median(v) for k, v in res.items()}
            ratio = md["new"] / md["old"]
            worst = max(worst, ratio)
            print(f"G{g} {m:7d} x {L:3d} = {n:7d} terms | {md['new']:9.3f} {md['old']:9.3f} {ratio:6.3f} | {md['mul']:9.3f} {md['fold']:9.3f} | {md['plain']:9.3f} "
                  f"| {md['fold'] / (md['mul'] + md['fold']):6.1%} {(md['plain'] - md['mul']) / md['plain']:6.1%}", flush=True)
    print(f"# worst new / composition = {worst:.3f} ({'below' if worst < 0.97 else 'NOT below'} 0.97)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--build-sweep", default="")
    ap.add_argument("--sweep", default="")
    a = ap.parse_args()
    if a.build_sweep:
        return build_sweep([int(w) for w in a.build_sweep.split(",")])
    if a.sweep:
        for w in a.sweep.split(","):
            so = VARIANTS / f"lib_msmfold_{w}.so"
            print(f"# BN_MSM_FOLD = {w} ({so.relative_to(ROOT)})", flush=True)
            # a fresh child per library (the library is chosen when bn_amd is first imported); stop at the first failure
            subprocess.run([sys.executable, __file__, "--repeats", str(a.repeats), "--shapes", a.shapes, "--groups", a.groups],
                           env=dict(os.environ, BN254_LIB_PATH=str(so)), check=True, timeout=300)
        return
    run(a)


if __name__ == "__main__":
    main()
