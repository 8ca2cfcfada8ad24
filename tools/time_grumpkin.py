#!/usr/bin/env python3
"""Grumpkin (bn254_grumpkin_{validate,add,mul,msm}_batch_dev) on one GPU, one process; every figure is the median [min max] of --repeats runs after
--warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - validate, add and mul at n = 1, 2^16 and 2^20 on points of the curve and random 256-bit scalars, beside two comparisons: (a)
    bn254_bjj_mul_batch_dev on as many records (same field, same window, a cheaper group law) and (b) bn254_fr_mul_batch_dev scaled to the number
    of field products the formulas execute - the count is printed; measured at 2^22 products and scaled linearly
  - bn254_grumpkin_msm_batch_dev on 2^12 segments of 256 terms and on 2^16 segments of 4 terms against the composition bn254_grumpkin_mul_batch_dev
    plus levels of bn254_grumpkin_add_batch_dev (halves of every segment added pairwise; the copies that line the halves up are not timed), in
    the same process, equal bytes asserted; ratio and ranges
  - VGPRs, spill count and private bytes of every new kernel instance (tools/kernel_meta.py)
  - with --variants W4.so W5.so (two libraries from tools/build_variant.sh, UNITS=bn254_grumpkin, with -DBN254_GRUMPKIN_MUL_WINDOW=4 and =5): the rule
    for the window of [k]P, fixed before measuring - 4 stays unless the [min, max] of five bn254_grumpkin_mul_batch_dev runs at 2^20 with a window
    of 5 lies wholly below, at zero spilled VGPRs (interleaved, events on the stream, equal bytes asserted)
Reported, not gated.  Everything printed is also written to --out (default profiles/r30_grumpkin.txt).
usage: tools/time_grumpkin.py [--repeats 5] [--warmup 1] [--small] [--variants W4.so W5.so] [--note TEXT]"""
import argparse
import ctypes as C
import pathlib
import re
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
OUT = None

# field products per record, from the formulas of grumpkin_ops.hpp (a product by the constant b3 counts as one)
ADD, DBL, INV = 14, 9, 2 + 127 * 3                     # complete addition (12 + 2 by b3); doubling (6 + 2 squarings + 1 by b3); Fermat inversion with 2-bit windows
MUL_CHAIN = 14 * ADD + 252 * DBL + 63 * ADD             # the table [2 .. 15]P, 63 windows of 4 doublings and one addition
PRODUCTS = {"validate": 3, "add": ADD + INV + 2, "mul": MUL_CHAIN + INV + 2}


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


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="sizes divided by 2^6: a dry run of the tool, not a measurement")
    ap.add_argument("--variants", nargs=2, metavar=("W4.so", "W5.so"))
    ap.add_argument("--note", action="append", default=[], help="a line to append to the report (the build times, for instance)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r30_grumpkin.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, babyjub as BJ, grumpkin as GK
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    lib.bn254_grumpkin_window.argtypes = []
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    say("shipped library: the window of [k]P is %d bits (a table of %d points); kernel ms; median [min max] over %d runs after %d warm-up, one process%s"
        % (lib.bn254_grumpkin_window(), 1 << lib.bn254_grumpkin_window(), a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    s0 = torch.cuda.current_stream().cuda_stream
    n_big, n_seed = 1 << (20 - sh), 1 << (14 - sh)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1)).to(dev)
    i64 = lambda words: torch.empty(words, dtype=torch.int64, device=dev)

    # ---- inputs: n_big random 256-bit scalars (two 512-bit draws mod r would be below r: the words of synthetic scalars are taken as plain
    # integers, and the top word is filled from a second draw so that all 256 bits are live); n_seed points [k]G, tiled to n_big
    K = i64(n_big * 4); K2 = i64(n_big * 4)
    eng.synthetic_scalars_dev(30, 0, n_big, 0, K.data_ptr(), s0); eng.synthetic_scalars_dev(31, 0, n_big, 0, K2.data_ptr(), s0)
    K.view(-1, 4)[:, 3] ^= K2.view(-1, 4)[:, 0]
    Gt = up(np.tile(GK.point_limbs(GK.G), (n_seed, 1, 1)))
    P0 = i64(n_seed * 8)
    eng.grumpkin_mul_batch_dev(Gt.data_ptr(), K.data_ptr(), P0.data_ptr(), n_seed, s0)
    torch.cuda.synchronize()
    P = P0.repeat(n_big // n_seed)
    Q = torch.roll(P.view(-1, 8), 1, 0).contiguous().view(-1)
    O8 = i64(n_big * 8)
    ST = torch.full((n_big,), -1, dtype=torch.int32, device=dev)
    BJP = up(np.tile(BJ.point_limbs(BJ.B8), (n_big, 1, 1)))
    KB = i64(n_big * 4)
    eng.synthetic_scalars_dev(32, 0, n_big, 0, KB.data_ptr(), s0)
    torch.cuda.synchronize()

    def kernel_ms(scopes, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        got = [eng.kernel_stats(s) for s in scopes]
        eng.profile(False)
        return sum(ms for ms, _ in got)

    say("-- kernel instances (tools/kernel_meta.py): VGPRs, the waves per SIMD they allow (512 registers, allocated in eights), spill, private bytes")
    for name, m in sorted(kernel_meta.instances(_native.LIB_PATH).items()):
        mm = re.search(r"\d+(GrkValidateOp|GrkAddOp|GrkMulOp|GrkMsmOp|GrkMsmFoldOp|BjjMulOp)E", name)
        if mm:
            say("%s<%s> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (kernel_meta.short_name(name), mm.group(1), m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    n_ref = 1 << (22 - sh)
    X = i64(n_ref * 4); Y = i64(n_ref * 4); Z = i64(n_ref * 4)
    eng.synthetic_scalars_dev(33, 0, n_ref, 0, X.data_ptr(), s0); eng.synthetic_scalars_dev(34, 0, n_ref, 0, Y.data_ptr(), s0)
    ref = repeat(lambda: kernel_ms(("fr_mul",), lambda: eng.fr_mul_batch_dev(X.data_ptr(), Y.data_ptr(), Z.data_ptr(), n_ref, s0)), a.repeats, a.warmup)
    per_product = statistics.median(ref) / n_ref
    say("-- reference (b): bn254_fr_mul_batch_dev on 2^%d products: kernel ms %s = %.3f ps per product (it moves 96 bytes per product; the chains keep theirs in registers)" % (22 - sh, fmt(ref), per_product * 1e9))

    calls = {
        "validate": (("grumpkin_validate",), lambda n: eng.grumpkin_validate_batch_dev(P.data_ptr(), ST.data_ptr(), n, s0)),
        "add": (("grumpkin_add",), lambda n: eng.grumpkin_add_batch_dev(P.data_ptr(), Q.data_ptr(), O8.data_ptr(), n, s0)),
        "mul": (("grumpkin_mul",), lambda n: eng.grumpkin_mul_batch_dev(P.data_ptr(), K.data_ptr(), O8.data_ptr(), n, s0)),
    }
    for what, (scopes, call) in calls.items():
        count = PRODUCTS[what]
        say("-- bn254_grumpkin_%s_batch_dev: %d field products per record" % (what, count))
        for n in (1, 1 << (16 - sh), n_big):
            ST.fill_(-1)
            v = repeat(lambda: kernel_ms(scopes, lambda: call(n)), a.repeats, a.warmup)
            if what == "validate":
                assert not ST[:n].any().item(), "a point of the curve was rejected"
            ms = statistics.median(v)
            line = "n = %-7d | kernel ms %s | %9.3f M/s | (b) fr_mul_batch_dev on %d x n products, scaled: %9.4f ms, the call takes %.2f x" % (n, fmt(v), n / ms / 1e3, count, per_product * count * n, ms / (per_product * count * n))
            if what == "mul":
                vb = repeat(lambda: kernel_ms(("bjj_mul",), lambda: eng.bjj_mul_batch_dev(BJP.data_ptr(), KB.data_ptr(), O8.data_ptr(), n, s0)), a.repeats, a.warmup)
                line += " | (a) bjj_mul_batch_dev on n records: %s, the call takes %.2f x" % (fmt(vb), ms / statistics.median(vb))
            say(line)

    # ---- the segmented sum against mul + levels of add
    any_faster = False
    for log_m, L in ((12 - sh, 256), (16 - sh, 4)):
        m = 1 << log_m; n = m * L
        offs = np.arange(0, n + 1, L, dtype=np.uint64)
        OUTM = i64(m * 8)
        say("-- bn254_grumpkin_msm_batch_dev on 2^%d segments of %d terms (%d terms) against bn254_grumpkin_mul_batch_dev + %d levels of bn254_grumpkin_add_batch_dev" % (log_m, L, n, L.bit_length() - 1))
        fused = repeat(lambda: kernel_ms(("grumpkin_msm", "grumpkin_msm_fold"), lambda: eng.grumpkin_msm_batch_dev(P.data_ptr(), K.data_ptr(), offs, m, OUTM.data_ptr(), s0)), a.repeats, a.warmup)
        PR = i64(n * 8)
        holder = {}

        def composed():
            eng.profile(True); eng.profile_reset()
            torch.cuda.synchronize()
            eng.grumpkin_mul_batch_dev(P.data_ptr(), K.data_ptr(), PR.data_ptr(), n, s0)
            cur = PR.view(m, L, 8)
            while cur.shape[1] > 1:
                h = cur.shape[1] // 2
                lo, hi = cur[:, :h].contiguous(), cur[:, h:].contiguous()
                eng.grumpkin_add_batch_dev(lo.data_ptr(), hi.data_ptr(), lo.data_ptr(), m * h, s0)
                cur = lo
            torch.cuda.synchronize()
            ms = eng.kernel_stats("grumpkin_mul")[0] + eng.kernel_stats("grumpkin_add")[0]
            eng.profile(False)
            holder["out"] = cur.reshape(-1)
            return ms
        comp = repeat(composed, a.repeats, a.warmup)
        assert torch.equal(holder["out"], OUTM), "the segmented sum and the composition differ"
        fm, cm = statistics.median(fused), statistics.median(comp)
        below = max(fused) < min(comp)
        any_faster |= below
        say("fused      | kernel ms %s | %9.3f M terms/s" % (fmt(fused), n / fm / 1e3))
        say("mul + adds | kernel ms %s | the fused call takes %.3f x; its [min, max] lies %s the composition's; equal bytes" % (fmt(comp), fm / cm, "wholly below" if below else "NOT wholly below"))
    if not any_faster:
        say("the fused call is not faster than the composition anywhere measured")

    if a.variants:
        say("-- the window of [k]P, 4 bits against 5: bn254_grumpkin_mul_batch_dev at 2^%d through each library (tools/build_variant.sh, UNITS=bn254_grumpkin), interleaved, events on the stream" % (20 - sh))
        libs = []
        for path in a.variants:
            l = C.CDLL(str(pathlib.Path(path).resolve()))
            l.bn254_grumpkin_mul_batch_dev.argtypes = _native.SIGNATURES["bn254_grumpkin_mul_batch_dev"]
            l.bn254_grumpkin_window.argtypes = []
            libs.append(l)
            for name, mt in sorted(kernel_meta.instances(pathlib.Path(path).resolve()).items()):
                if re.search(r"\d+(GrkMulOp|GrkMsmOp)E", name):
                    say("W = %d: %s | %3d VGPRs | spill %d | private %d" % (l.bn254_grumpkin_window(), re.search(r"Grk\w+?Op", name).group(0), mt["vgpr"], mt["spill"], mt["private"]))
        assert [l.bn254_grumpkin_window() for l in libs] == [4, 5], "--variants takes the 4-bit library first, the 5-bit one second"
        outs = [i64(n_big * 8) for _ in libs]

        def one_run(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert libs[k].bn254_grumpkin_mul_batch_dev(None, P.data_ptr(), K.data_ptr(), outs[k].data_ptr(), n_big, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        times = ([], [])
        for r in range(a.warmup + a.repeats):
            for k in (0, 1):
                ms = one_run(k)
                if r >= a.warmup:
                    times[k].append(ms)
        assert torch.equal(outs[0], outs[1]), "the two windows differ in their bytes"
        for k, w in enumerate((4, 5)):
            say("W = %d | ms %s | %9.3f M/s" % (w, fmt(times[k]), n_big / statistics.median(times[k]) / 1e3))
        say("the rule (fixed before measuring): 4 stays unless the [min, max] of W = 5 lies wholly below W = 4's at zero spilled VGPRs -> %s; equal bytes"
            % ("W = 5 qualifies by time (check its spill count above)" if max(times[1]) < min(times[0]) else "W = 4 stays"))
    for note in a.note:
        say(note)
    say("   not built: GLV, signed digits and mixed additions, a bucket-method MSM, prepared or fixed-base generator tables, compressed points, an Fq type in the ABI, Barretenberg-compatible generators, multi-GPU forms")


if __name__ == "__main__":
    main()
