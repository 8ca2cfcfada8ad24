#!/usr/bin/env python3
"""Validation of raw points (bn254_g1_validate_batch, bn254_g2_validate_batch) and the membership test of the G2 decoders on one GPU, one process;
every figure is the median [min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - bn254_g2_validate_batch_dev at n = 1, 2^15, 2^18 beside bn254_g2_clear_cofactor_batch_dev on the same points: the same [u] chain plus a normalisation
  - bn254_g1_validate_batch_dev at n = 1, 2^16, 2^20 beside a device-to-device copy of its bytes
  - bn254_g2_decode_batch and bn254_g2_decompress_batch_dev at the sizes of profiles/r21_compress.txt, and groth16.verify_batch_compressed on 2^12
    proofs against verify_batch as tools/time_compress.py measures it
  - with --variants CHAIN.so ENDO.so (two libraries from tools/build_variant.sh, UNITS=bn254_wire, with -DBN254_G2_SUBGROUP_ENDO=0 and =1): the rule
    for which test the decoders ship with - bn254_g2_decompress_batch_dev over 2^18 valid records through each library, interleaved, events on the
    stream, equal bytes and statuses asserted; the endomorphism test ships if its [min, max] lies wholly below the chain's (and bn254_g2_decode_k
    keeps its spill ceiling: tests/test_build_quality.py)
Reported, not gated.  Everything printed is also written to --out (default profiles/r24_validate.txt).
usage: tools/time_validate.py [--repeats 5] [--warmup 1] [--small] [--variants CHAIN.so ENDO.so]"""
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
TESTS = ("the r - 1 chain (253 doublings, 127 additions)", "the endomorphism test (one [u] chain: 63 doublings, 31 additions, three psi maps)")


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
    ap.add_argument("--variants", nargs=2, metavar=("CHAIN.so", "ENDO.so"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r24_validate.txt"))
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
    lib.bn254_wire_subgroup_endo.argtypes = []
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    shipped = lib.bn254_wire_subgroup_endo()
    say("shipped library: the G2 decoders prove membership with %s; the validate calls always run the endomorphism test; kernel ms; median [min max] over %d runs after %d warm-up, one process%s"
        % (TESTS[shipped], a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    s0 = torch.cuda.current_stream().cuda_stream
    n1, n2 = 1 << (20 - sh), 1 << (18 - sh)
    K = torch.empty(n1 * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(24, 0, n1, 0, K.data_ptr(), s0)
    P1 = torch.empty(n1 * 12, dtype=torch.int64, device=dev)
    P2 = torch.empty(n2 * 24, dtype=torch.int64, device=dev)
    eng.g1_mul_base_batch_dev(G1.one().limbs, K.data_ptr(), P1.data_ptr(), n1, s0)
    eng.g2_mul_base_batch_dev(G2.one().limbs, K.data_ptr(), P2.data_ptr(), n2, s0)
    B2 = torch.empty(n2 * 64, dtype=torch.uint8, device=dev)
    O1 = torch.empty(n1 * 12, dtype=torch.int64, device=dev)
    O2 = torch.empty(n2 * 24, dtype=torch.int64, device=dev)
    ST = torch.full((n1,), -1, dtype=torch.int32, device=dev)
    eng.g2_compress_batch_dev(P2.data_ptr(), B2.data_ptr(), n2, "ark", s0)
    # points of the twist outside G2 for the rejecting side: maps of 96 random bytes
    gen = torch.Generator(device=dev); gen.manual_seed(24)
    U = torch.randint(0, 256, (n2 * 96,), dtype=torch.uint8, device=dev, generator=gen)
    M2 = torch.empty(n2 * 24, dtype=torch.int64, device=dev)
    eng.g2_map_to_curve_batch_dev(U.data_ptr(), M2.data_ptr(), n2, s0)
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
        mm = re.search(r"\d+(G[12]ValidateOp|G2DecompressOp|G2ClearCofactorOp)E", name)
        if mm or (kernel_meta.short_name(name) == "bn254_g2_decode_k" and "Op" not in name):
            say("%s<%s> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (kernel_meta.short_name(name), mm.group(1) if mm else "the wire decoder", m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    say("-- G2 validation: bn254_g2_validate_batch_dev on points of G2, beside bn254_g2_clear_cofactor_batch_dev on the same points (the same [u] chain plus a normalisation)")
    for n in (1, 1 << (15 - sh), n2):
        v = repeat(lambda: kernel_ms(("g2_validate",), lambda: eng.g2_validate_batch_dev(P2.data_ptr(), ST.data_ptr(), n, s0)), a.repeats, a.warmup)
        assert not ST[:n].any().item(), "a point of G2 was rejected"
        c = repeat(lambda: kernel_ms(("g2_clear_cofactor",), lambda: eng.g2_clear_cofactor_batch_dev(P2.data_ptr(), O2.data_ptr(), n, s0)), a.repeats, a.warmup)
        ms = statistics.median(v)
        say("n = %-7d | kernel ms %s | %9.3f M points/s | g2_clear_cofactor_batch_dev %s, validation takes %.2f x" % (n, fmt(v), n / ms / 1e3, fmt(c), ms / statistics.median(c)))
    v = repeat(lambda: kernel_ms(("g2_validate",), lambda: eng.g2_validate_batch_dev(M2.data_ptr(), ST.data_ptr(), n2, s0)), a.repeats, a.warmup)
    assert (ST[:n2] == 5).all().item(), "a mapped point was accepted"
    say("n = %-7d | kernel ms %s | the same on mapped points (on the twist, outside G2): every status is 5" % (n2, fmt(v)))

    say("-- G1 validation: bn254_g1_validate_batch_dev (range and curve equation; cofactor 1)")
    for n in (1, 1 << (16 - sh), n1):
        v = repeat(lambda: kernel_ms(("g1_validate",), lambda: eng.g1_validate_batch_dev(P1.data_ptr(), ST.data_ptr(), n, s0)), a.repeats, a.warmup)
        assert not ST[:n].any().item(), "a point of G1 was rejected"
        ms = statistics.median(v)
        moved = (96 + 4) * n
        c = repeat(lambda: copy_ms(max(moved // 2, 16)), a.repeats, a.warmup)
        say("n = %-7d | kernel ms %s | %9.3f M points/s | d2d copy of the %d bytes moved %s, validation takes %.1f x" % (n, fmt(v), n / ms / 1e3, moved, fmt(c), ms / statistics.median(c)))

    say("-- the G2 decoders of the shipped library: bn254_g2_decompress_batch_dev (ark layout) against bn254_g2_decode_batch (\"wire_decode\") on the uncompressed records of the same points")
    for n in (1, 1 << (15 - sh), n2):
        v = repeat(lambda: kernel_ms(("g2_decompress",), lambda: eng.g2_decompress_batch_dev(B2.data_ptr(), O2.data_ptr(), ST.data_ptr(), n, "ark", s0)), a.repeats, a.warmup)
        assert not ST[:n].any().item(), "a generated record was rejected"
        wire = eng.g2_encode_batch(P2[:n * 24].cpu().numpy().view(np.uint64).reshape(n, 24))
        w = repeat(lambda: kernel_ms(("wire_decode",), lambda: eng.g2_decode_batch(wire)), a.repeats, a.warmup)
        ms = statistics.median(v)
        say("n = %-7d | kernel ms %s | %9.3f M points/s | g2_decode_batch of the 129-byte records %s, decompression takes %.2f x" % (n, fmt(v), n / ms / 1e3, fmt(w), ms / statistics.median(w)))
    assert torch.equal(O2, P2), "decompress(compress(p)) differs from p"

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
        say("-- the decoders' membership test, the r - 1 chain against the endomorphism test: G2 decompression of 2^%d valid records through each library (tools/build_variant.sh, UNITS=bn254_wire), interleaved, events on the stream" % (18 - sh))
        libs = []
        for path in a.variants:
            l = C.CDLL(str(pathlib.Path(path).resolve()))
            l.bn254_g2_decompress_batch_dev.argtypes = _native.SIGNATURES["bn254_g2_decompress_batch_dev"]
            l.bn254_wire_subgroup_endo.argtypes = []
            libs.append(l)
        assert [l.bn254_wire_subgroup_endo() for l in libs] == [0, 1], "--variants takes the chain library first, the endomorphism one second"
        outs = [torch.zeros(n2 * 24, dtype=torch.int64, device=dev) for _ in libs]
        sts = [torch.full((n2,), -1, dtype=torch.int32, device=dev) for _ in libs]

        def one_run(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert libs[k].bn254_g2_decompress_batch_dev(None, B2.data_ptr(), 0, outs[k].data_ptr(), sts[k].data_ptr(), n2, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        times = ([], [])
        for rep in range(a.warmup + a.repeats):
            for k in (0, 1):
                ms = one_run(k)
                if rep >= a.warmup:
                    times[k].append(ms)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], P2), "the two variants differ in their bytes"
        assert torch.equal(sts[0], sts[1]) and not sts[0].any().item(), "the two variants differ in their statuses"
        say("the r - 1 chain        | ms %s" % fmt(times[0]))
        say("the endomorphism test  | ms %s | %.3f x the other; bytes and statuses are equal" % (fmt(times[1]), statistics.median(times[1]) / statistics.median(times[0])))
        wins = max(times[1]) < min(times[0])
        say("the rule (fixed before measuring): the endomorphism test ships in the decoders if the [min, max] of its %d runs lies wholly below the chain's and bn254_g2_decode_k keeps its "
            "ceiling of 18 spilled VGPRs -> the timing condition %s (the library measured above carries %s)" % (a.repeats, "holds" if wins else "FAILS", TESTS[shipped]))
    say("   not built: validation fused into the pairing and MSM entry points, a shorter addition chain for u, multi-GPU forms")


if __name__ == "__main__":
    main()
