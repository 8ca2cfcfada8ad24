#!/usr/bin/env python3
"""The compressed G1 / G2 encodings (bn254_g{1,2}_compress_batch, bn254_g{1,2}_decompress_batch) on one GPU, one process; every figure is the
median [min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - G1 decompression at n = 1, 2^16, 2^20 against two floors, as ratios: a device-to-device copy of the bytes moved (32 in, 96 out per
    record) and bn254_fr_pow_batch_dev on as many elements, the nearest existing exponentiation of fixed length
  - G2 decompression at n = 1, 2^15, 2^18 against the kernel time of bn254_g2_decode_batch on the uncompressed records of the same points:
    both pay the subgroup chain, so the difference is the two square roots minus the parsing of y
  - compression, both groups, at the same sizes
  - groth16.verify_batch_compressed against groth16.verify_batch in wall time on 2^12 proofs: one proof of a one-constraint circuit
    (groth16.setup / groth16.prove), repeated
  - the VGPRs, spills and private bytes of the four kernel instances (tools/kernel_meta.py)
  - with --variants PLAIN.so WINDOW.so (two libraries from tools/build_variant.sh, UNITS=bn254_wire, with -DBN254_SQRT_WINDOW=0 and =1):
    G1 decompression of 2^20 records through each library, interleaved, timed by events on the stream, and the decision by the rule fixed
    before measuring - the form with the smaller median ships
Reported, not gated.  Everything printed is also written to --out (default profiles/r21_compress.txt).
usage: tools/time_compress.py [--repeats 5] [--warmup 1] [--small] [--variants PLAIN.so WINDOW.so]"""
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
    ap.add_argument("--variants", nargs=2, metavar=("PLAIN.so", "WINDOW.so"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r21_compress.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, groth16
    from bn_amd.api import Fr, G1, G2
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_compress_sqrt_window.argtypes = []
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    window = lib.bn254_compress_sqrt_window()
    forms = ("square-and-multiply over the bits of (q - 3) / 4", "a fixed 4-bit window over (q - 3) / 4")
    say("shipped library: square roots by %s; kernel ms; median [min max] over %d runs after %d warm-up, one process%s"
        % (forms[window], a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    s0 = torch.cuda.current_stream().cuda_stream
    n1, n2 = 1 << (20 - sh), 1 << (18 - sh)
    K = torch.empty(n1 * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(21, 0, n1, 0, K.data_ptr(), s0)
    P1 = torch.empty(n1 * 12, dtype=torch.int64, device=dev)
    P2 = torch.empty(n2 * 24, dtype=torch.int64, device=dev)
    eng.g1_mul_base_batch_dev(G1.one().limbs, K.data_ptr(), P1.data_ptr(), n1, s0)
    eng.g2_mul_base_batch_dev(G2.one().limbs, K.data_ptr(), P2.data_ptr(), n2, s0)
    B1 = torch.empty(n1 * 32, dtype=torch.uint8, device=dev)
    B2 = torch.empty(n2 * 64, dtype=torch.uint8, device=dev)
    O1 = torch.empty(n1 * 12, dtype=torch.int64, device=dev)
    O2 = torch.empty(n2 * 24, dtype=torch.int64, device=dev)
    ST = torch.empty(n1, dtype=torch.int32, device=dev)
    E = torch.empty(n1 * 4, dtype=torch.int64, device=dev)
    eng.g1_compress_batch_dev(P1.data_ptr(), B1.data_ptr(), n1, "ark", s0)
    eng.g2_compress_batch_dev(P2.data_ptr(), B2.data_ptr(), n2, "ark", s0)
    torch.cuda.synchronize()

    def kernel_ms(scopes, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        got = [eng.kernel_stats(s) for s in scopes]
        eng.profile(False)
        return sum(ms for ms, _ in got)

    def copy_ms(nbytes):
        """a device-to-device copy of nbytes: it moves 2 * nbytes"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert hip.hipMemcpyAsync(O1.data_ptr(), P1.data_ptr(), nbytes, 3, s0) == 0
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    say("-- kernel instances (tools/kernel_meta.py): VGPRs, the waves per SIMD they allow (512 registers, allocated in eights), spill, private bytes")
    for name, m in sorted(kernel_meta.instances(_native.LIB_PATH).items()):
        mm = re.search(r"\d+(G[12](?:Dec|C)ompressOp)E", name)
        if mm:
            say("%s<%s> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (kernel_meta.short_name(name), mm.group(1), m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    say("-- G1 decompression: bn254_g1_decompress_batch_dev (ark layout)")
    for n in (1, 1 << (16 - sh), n1):
        v = repeat(lambda: kernel_ms(("g1_decompress",), lambda: eng.g1_decompress_batch_dev(B1.data_ptr(), O1.data_ptr(), ST.data_ptr(), n, "ark", s0)), a.repeats, a.warmup)
        assert not ST[:n].any().item(), "a generated record was rejected"
        ms = statistics.median(v)
        moved = (32 + 96) * n
        c = repeat(lambda: copy_ms(max(moved // 2, 16)), a.repeats, a.warmup)
        p = repeat(lambda: kernel_ms(("fr_pow",), lambda: eng.fr_pow_batch_dev(K.data_ptr(), K.data_ptr(), E.data_ptr(), n, s0)), a.repeats, a.warmup)
        say("n = %-7d | kernel ms %s | %9.3f M points/s | d2d copy of the %d bytes moved %s, decompression takes %.1f x | fr_pow_batch_dev on %d elements %s, decompression takes %.2f x"
            % (n, fmt(v), n / ms / 1e3, moved, fmt(c), ms / statistics.median(c), n, fmt(p), ms / statistics.median(p)))
    assert torch.equal(O1, P1), "decompress(compress(p)) differs from p"

    say("-- G2 decompression: bn254_g2_decompress_batch_dev (ark layout) against bn254_g2_decode_batch (\"wire_decode\") on the uncompressed records of the same points")
    for n in (1, 1 << (15 - sh), n2):
        v = repeat(lambda: kernel_ms(("g2_decompress",), lambda: eng.g2_decompress_batch_dev(B2.data_ptr(), O2.data_ptr(), ST.data_ptr(), n, "ark", s0)), a.repeats, a.warmup)
        assert not ST[:n].any().item(), "a generated record was rejected"
        wire = eng.g2_encode_batch(P2[:n * 24].cpu().numpy().view(np.uint64).reshape(n, 24))
        w = repeat(lambda: kernel_ms(("wire_decode",), lambda: eng.g2_decode_batch(wire)), a.repeats, a.warmup)
        ms = statistics.median(v)
        say("n = %-7d | kernel ms %s | %9.3f M points/s | g2_decode_batch of the 129-byte records %s, decompression takes %.2f x: the two roots cost %.4f ms more than parsing y"
            % (n, fmt(v), n / ms / 1e3, fmt(w), ms / statistics.median(w), ms - statistics.median(w)))
    assert torch.equal(O2, P2), "decompress(compress(p)) differs from p"

    say("-- compression: bn254_g{1,2}_compress_batch_dev (ark layout; one inversion per point)")
    for g, P, B, sizes, fn in ((1, P1, B1, (1, 1 << (16 - sh), n1), eng.g1_compress_batch_dev), (2, P2, B2, (1, 1 << (15 - sh), n2), eng.g2_compress_batch_dev)):
        for n in sizes:
            v = repeat(lambda: kernel_ms(("g%d_compress" % g,), lambda: fn(P.data_ptr(), B.data_ptr(), n, "ark", s0)), a.repeats, a.warmup)
            say("G%d, n = %-7d | kernel ms %s | %9.3f M points/s" % (g, n, fmt(v), n / statistics.median(v) / 1e3))

    m = 1 << (12 - sh)
    say("-- groth16: verify_batch_compressed against verify_batch, wall ms, %d proofs (one proof of the circuit x * x = y, repeated)" % m)
    one = Fr.one().limbs[None]
    row = lambda col: (np.array([0, 1], np.uint64), np.array([col], np.uint64), one)
    system = groth16.R1CS(1, 3, row(2), row(2), row(1))                            # z = (1, y, x)
    Z = np.stack([Fr(1).limbs, Fr(49).limbs, Fr(7).limbs])
    pk, vk = groth16.setup(system, np.random.default_rng(1))
    proof = groth16.prove(pk, system, Z, np.random.default_rng(2))
    proofs, inputs = [proof] * m, [[Fr(49)]] * m
    blob = groth16.encode_proofs(proofs, "ark")

    def wall(fn):
        t0 = time.perf_counter()
        ok = fn()
        ms = (time.perf_counter() - t0) * 1e3
        assert ok.all()
        return ms
    for prepared in (False, True):
        u = repeat(lambda: wall(lambda: groth16.verify_batch(vk, proofs, inputs, prepared=prepared)), a.repeats, a.warmup)
        c = repeat(lambda: wall(lambda: groth16.verify_batch_compressed(vk, blob, inputs, "ark", prepared=prepared)), a.repeats, a.warmup)
        say("prepared=%-5s | verify_batch %s | verify_batch_compressed (%d bytes) %s | %.2f x" % (prepared, fmt(u), len(blob), fmt(c), statistics.median(c) / statistics.median(u)))

    if a.variants:
        say("-- the exponentiation chain, square-and-multiply against the 4-bit window: G1 decompression of 2^%d records through each library (tools/build_variant.sh, UNITS=bn254_wire), interleaved, events on the stream" % (20 - sh))
        libs = []
        for path in a.variants:
            l = C.CDLL(str(pathlib.Path(path).resolve()))
            l.bn254_g1_decompress_batch_dev.argtypes = _native.SIGNATURES["bn254_g1_decompress_batch_dev"]
            l.bn254_compress_sqrt_window.argtypes = []
            libs.append(l)
        assert [l.bn254_compress_sqrt_window() for l in libs] == [0, 1], "--variants takes the square-and-multiply library first, the window one second"
        outs = [torch.zeros(n1 * 12, dtype=torch.int64, device=dev) for _ in libs]

        def one_run(l, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert l.bn254_g1_decompress_batch_dev(None, B1.data_ptr(), 0, out.data_ptr(), ST.data_ptr(), n1, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        times = ([], [])
        for rep in range(a.warmup + a.repeats):
            for k in (0, 1):
                ms = one_run(libs[k], outs[k])
                if rep >= a.warmup:
                    times[k].append(ms)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], P1), "the two variants differ in their bytes"
        say("square-and-multiply (251 squarings, 108 products)          | ms %s" % fmt(times[0]))
        say("4-bit window (248 squarings, 14 + 56 products, 16 entries) | ms %s | %.3f x the other; the bytes are equal" % (fmt(times[1]), statistics.median(times[1]) / statistics.median(times[0])))
        wins = statistics.median(times[1]) < statistics.median(times[0])
        say("the rule (fixed before measuring): the form with the smaller median of %d ships -> %s (the library measured above carries %s)"
            % (a.repeats, forms[int(wins)], forms[window]))
    say("   not built: compressed Gt, compressed stream forms, multi-GPU forms, gnark's or snarkjs' own proof-file framing")


if __name__ == "__main__":
    main()
