#!/usr/bin/env python3
"""Hash-to-curve for G1 (bn254_g1_map_to_curve_batch, bn254_g1_hash_to_curve_uniform_batch, bn254_g1_hash_to_curve_batch) on one GPU, one
process; every figure is the median [min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - the three calls at n = 1, 2^16, 2^20 (32-byte messages), and beside each bn254_g1_decompress_batch_dev on as many records: that is one
    exponentiation chain per record, so the ratio shows what each of the map's chains costs (the map runs four, a hash eight and an inversion)
  - the VGPRs, spills and private bytes of the three kernel instances (tools/kernel_meta.py)
  - bls.verify_batch on 2^12 signatures as wall time, split into hashing and the rest (negation and pairing check)
  - with --variants FERMAT.so CAND.so (two libraries from tools/build_variant.sh, UNITS=bn254_hash, with -DBN254_H2C_INV0=0 and =1):
    map_to_curve of 2^20 elements through each library, interleaved, timed by events on the stream, the same bytes asserted, and the
    decision by the rule fixed before measuring - the form with the smaller median ships
Reported, not gated.  Everything printed is also written to --out (default profiles/r22_hash.txt).
usage: tools/time_hash.py [--repeats 5] [--warmup 1] [--small] [--variants FERMAT.so CAND.so]"""
import argparse
import ctypes as C
import pathlib
import re
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
OUT = None


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
    ap.add_argument("--variants", nargs=2, metavar=("FERMAT.so", "CAND.so"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r22_hash.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, bls
    from bn_amd.api import Fr, G1
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    lib.bn254_hash_inv0_form.argtypes = []
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    shipped = lib.bn254_hash_inv0_form()
    forms = ("fe_inverse_fermat (a^(q-2) bit by bit)", "the candidate chain (a^-1 = chi t^2)")
    say("shipped library: one launch per call; inv0 by %s; kernel ms; median [min max] over %d runs after %d warm-up, one process%s"
        % (forms[shipped], a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    s0 = torch.cuda.current_stream().cuda_stream
    n1 = 1 << (20 - sh)
    gen = torch.Generator(device=dev); gen.manual_seed(22)
    U = torch.randint(0, 256, (n1 * 96,), dtype=torch.uint8, device=dev, generator=gen)          # 48-byte elements, 96-byte records or 32-byte messages
    O = torch.empty(n1 * 12, dtype=torch.int64, device=dev)
    K = torch.empty(n1 * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(22, 0, n1, 0, K.data_ptr(), s0)
    P1 = torch.empty(n1 * 12, dtype=torch.int64, device=dev)
    eng.g1_mul_base_batch_dev(G1.one().limbs, K.data_ptr(), P1.data_ptr(), n1, s0)
    B1 = torch.empty(n1 * 32, dtype=torch.uint8, device=dev)
    ST = torch.empty(n1, dtype=torch.int32, device=dev)
    eng.g1_compress_batch_dev(P1.data_ptr(), B1.data_ptr(), n1, "ark", s0)
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
        mm = re.search(r"\d+(G1(?:MapToCurve|HashUniform|HashMsg)Op)E", name)
        if mm:
            say("%s<%s> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (kernel_meta.short_name(name), mm.group(1), m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    calls = (("map_to_curve (48-byte elements)", "g1_map_to_curve", lambda n: eng.g1_map_to_curve_batch_dev(U.data_ptr(), O.data_ptr(), n, s0)),
             ("hash_to_curve from 96 uniform bytes", "g1_hash_to_curve", lambda n: eng.g1_hash_to_curve_uniform_batch_dev(U.data_ptr(), O.data_ptr(), n, s0)),
             ("hash_to_curve of 32-byte messages", "g1_hash_to_curve_msg", lambda n: eng.g1_hash_to_curve_batch_dev(U.data_ptr(), 32, bls.DST, O.data_ptr(), n, s0)))
    for what, scope, call in calls:
        say("-- %s" % what)
        for n in (1, 1 << (16 - sh), n1):
            v = repeat(lambda: kernel_ms((scope,), lambda: call(n)), a.repeats, a.warmup)
            d = repeat(lambda: kernel_ms(("g1_decompress",), lambda: eng.g1_decompress_batch_dev(B1.data_ptr(), P1.data_ptr(), ST.data_ptr(), n, "ark", s0)), a.repeats, a.warmup)
            ms = statistics.median(v)
            say("n = %-7d | kernel ms %s | %9.3f M points/s | g1_decompress_batch_dev on %d records (one chain each) %s, this call takes %.2f x"
                % (n, fmt(v), n / ms / 1e3, n, fmt(d), ms / statistics.median(d)))

    m = 1 << (12 - sh)
    say("-- bls.verify_batch on %d signatures of 32-byte messages, wall ms: the whole call, and its hash call alone" % m)
    rng = np.random.default_rng(22)
    sks = np.stack([Fr.random(rng).limbs for _ in range(m)])
    pks = np.stack([p.limbs for p in bls.public_keys(sks)])
    msgs = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    sigs = np.stack([s.limbs for s in bls.sign_batch(sks, msgs)])

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def verify():
        assert bls.verify_batch(pks, msgs, sigs).all()
    whole = repeat(lambda: wall(verify), a.repeats, a.warmup)
    hashing = repeat(lambda: wall(lambda: eng.g1_hash_to_curve_batch(msgs, bls.DST)), a.repeats, a.warmup)
    say("verify_batch %s | hashing (host buffers in and out) %s | negation and pairing check, by difference of the medians %9.4f | %.1f k signatures/s"
        % (fmt(whole), fmt(hashing), statistics.median(whole) - statistics.median(hashing), m / statistics.median(whole)))

    if a.variants:
        say("-- inv0, fe_inverse_fermat against the candidate chain: map_to_curve of 2^%d elements through each library (tools/build_variant.sh, UNITS=bn254_hash), interleaved, events on the stream" % (20 - sh))
        libs = []
        for path in a.variants:
            l = C.CDLL(str(pathlib.Path(path).resolve()))
            l.bn254_g1_map_to_curve_batch_dev.argtypes = _native.SIGNATURES["bn254_g1_map_to_curve_batch_dev"]
            l.bn254_hash_inv0_form.argtypes = []
            libs.append(l)
        assert [l.bn254_hash_inv0_form() for l in libs] == [0, 1], "--variants takes the Fermat library first, the candidate-chain one second"
        outs = [torch.zeros(n1 * 12, dtype=torch.int64, device=dev) for _ in libs]

        def one_run(l, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert l.bn254_g1_map_to_curve_batch_dev(None, U.data_ptr(), out.data_ptr(), n1, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        times = ([], [])
        for rep in range(a.warmup + a.repeats):
            for k in (0, 1):
                ms = one_run(libs[k], outs[k])
                if rep >= a.warmup:
                    times[k].append(ms)
        eng.g1_map_to_curve_batch_dev(U.data_ptr(), O.data_ptr(), n1, s0); torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], O), "the two variants differ in their bytes"
        say("fe_inverse_fermat (254 squarings, 110 products)                             | ms %s" % fmt(times[0]))
        say("candidate chain (fe_sqrt_cand's 4-bit window, then 3 products and a squaring) | ms %s | %.3f x the other; the bytes are equal" % (fmt(times[1]), statistics.median(times[1]) / statistics.median(times[0])))
        wins = statistics.median(times[1]) < statistics.median(times[0])
        say("the rule (fixed before measuring): the form with the smaller median of %d ships -> %s (the library measured above carries %s)"
            % (a.repeats, forms[int(wins)], forms[shipped]))
    say("   not built: hash to G2, encode_to_curve, expand_message_xof, messages of mixed length on the device, a map with three chains instead of four, multi-GPU forms")


if __name__ == "__main__":
    main()
