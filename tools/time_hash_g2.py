#!/usr/bin/env python3
"""Hash-to-curve for G2 and cofactor clearing (bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch, bn254_g2_hash_to_curve_uniform_batch,
bn254_g2_hash_to_curve_batch) on one GPU, one process; every figure is the median [min max] of --repeats runs after --warmup.  Kernel ms come
from bn254_kernel_stats around the _dev call.
  - the map and the two hash calls at n = 1, 2^15, 2^18 (32-byte messages), each beside bn254_g2_decompress_batch_dev on as many records: that
    call proves membership (the r - 1 chain when profiles/r23_hash_g2.txt was written, the endomorphism subgroup test since), which clearing the cofactor by psi avoids
  - bn254_g2_clear_cofactor_batch_dev on points of G2 beside bn254_g2_mul_batch_dev by k = u + 3u lambda + u lambda^2 + lambda^3 on the same
    points: on the subgroup the two give equal bytes (asserted)
  - the VGPRs, spills and private bytes of the four kernel instances (tools/kernel_meta.py) and the launch shape that shipped
  - bls_minpk.verify_batch on 2^12 signatures as wall time beside bls.verify_batch
Reported, not gated.  Everything printed is also written to --out (default profiles/r23_hash_g2.txt).
usage: tools/time_hash_g2.py [--repeats 5] [--warmup 1] [--small]"""
import argparse
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
U_BN = 4965661367192848881
R_ORD = 36 * U_BN**4 + 36 * U_BN**3 + 18 * U_BN**2 + 6 * U_BN + 1


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r23_hash_g2.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, bls, bls_minpk
    from bn_amd.api import Fr, G2
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    say("shipped library: one launch per call (field reduction, both maps, the sum, the cofactor clearing and the normalisation in one lane; no scratch); "
        "kernel ms; median [min max] over %d runs after %d warm-up, one process%s" % (a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    say("neither the constants nor the outputs are checked against gnark-crypto or any other library")
    s0 = torch.cuda.current_stream().cuda_stream
    n1 = 1 << (18 - sh)
    sizes = (1, 1 << (15 - sh), n1)
    gen = torch.Generator(device=dev); gen.manual_seed(23)
    U = torch.randint(0, 256, (n1 * 192,), dtype=torch.uint8, device=dev, generator=gen)         # 96-byte elements, 192-byte records or 32-byte messages
    O = torch.empty(n1 * 24, dtype=torch.int64, device=dev)
    K = torch.empty(n1 * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(23, 0, n1, 0, K.data_ptr(), s0)
    P2 = torch.empty(n1 * 24, dtype=torch.int64, device=dev)
    eng.g2_mul_base_batch_dev(G2.one().limbs, K.data_ptr(), P2.data_ptr(), n1, s0)                # points of G2
    B2 = torch.empty(n1 * 64, dtype=torch.uint8, device=dev)
    D2 = torch.empty(n1 * 24, dtype=torch.int64, device=dev)
    ST = torch.empty(n1, dtype=torch.int32, device=dev)
    eng.g2_compress_batch_dev(P2.data_ptr(), B2.data_ptr(), n1, "ark", s0)
    lam = 6 * U_BN * U_BN % R_ORD
    k = (U_BN + 3 * U_BN * lam + U_BN * lam * lam + lam ** 3) % R_ORD
    KK = torch.from_numpy(np.tile(Fr(k).limbs, (n1, 1)).view(np.int64).reshape(-1).copy()).to(dev)
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
        mm = re.search(r"\d+(G2(?:MapToCurve|ClearCofactor|HashUniform|HashMsg)Op)E", name)
        if mm:
            say("%s<%s> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (kernel_meta.short_name(name), mm.group(1), m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    calls = (("map_to_curve (96-byte elements; the result is NOT in G2)", "g2_map_to_curve", lambda n: eng.g2_map_to_curve_batch_dev(U.data_ptr(), O.data_ptr(), n, s0)),
             ("hash_to_curve from 192 uniform bytes", "g2_hash_to_curve", lambda n: eng.g2_hash_to_curve_uniform_batch_dev(U.data_ptr(), O.data_ptr(), n, s0)),
             ("hash_to_curve of 32-byte messages", "g2_hash_to_curve_msg", lambda n: eng.g2_hash_to_curve_batch_dev(U.data_ptr(), 32, bls_minpk.DST, O.data_ptr(), n, s0)))
    for what, scope, call in calls:
        say("-- %s" % what)
        for n in sizes:
            v = repeat(lambda: kernel_ms((scope,), lambda: call(n)), a.repeats, a.warmup)
            d = repeat(lambda: kernel_ms(("g2_decompress",), lambda: eng.g2_decompress_batch_dev(B2.data_ptr(), D2.data_ptr(), ST.data_ptr(), n, "ark", s0)), a.repeats, a.warmup)
            ms = statistics.median(v)
            say("n = %-7d | kernel ms %s | %9.3f M points/s | g2_decompress_batch_dev on %d records (two root chains and the subgroup test) %s, this call takes %.2f x"
                % (n, fmt(v), n / ms / 1e3, n, fmt(d), ms / statistics.median(d)))

    say("-- clear_cofactor on points of G2, beside g2_mul_batch_dev (GLS) by k on the same points: equal bytes on the subgroup")
    for n in sizes:
        v = repeat(lambda: kernel_ms(("g2_clear_cofactor",), lambda: eng.g2_clear_cofactor_batch_dev(P2.data_ptr(), O.data_ptr(), n, s0)), a.repeats, a.warmup)
        d = repeat(lambda: kernel_ms(("g2_mul",), lambda: eng.g2_mul_dev(P2.data_ptr(), KK.data_ptr(), D2.data_ptr(), n, s0)), a.repeats, a.warmup)
        torch.cuda.synchronize()
        assert torch.equal(O[:n * 24], D2[:n * 24]), "clear(Q) and [k]Q differ on G2"
        ms = statistics.median(v)
        say("n = %-7d | kernel ms %s | %9.3f M points/s | g2_mul_batch_dev by k %s, this call takes %.2f x; the bytes are equal"
            % (n, fmt(v), n / ms / 1e3, fmt(d), ms / statistics.median(d)))

    m = 1 << (12 - sh)
    say("-- verify_batch on %d signatures of 32-byte messages, wall ms: bls_minpk (keys in G1, hash to G2) beside bls (keys in G2, hash to G1)" % m)
    rng = np.random.default_rng(23)
    sks = np.stack([Fr.random(rng).limbs for _ in range(m)])
    msgs = rng.integers(0, 256, (m, 32), dtype=np.uint8)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    for name, mod, hash_call in (("bls_minpk", bls_minpk, lambda: eng.g2_hash_to_curve_batch(msgs, bls_minpk.DST)), ("bls      ", bls, lambda: eng.g1_hash_to_curve_batch(msgs, bls.DST))):
        pks = np.stack([p.limbs for p in mod.public_keys(sks)])
        sigs = np.stack([s.limbs for s in mod.sign_batch(sks, msgs)])

        def verify():
            assert mod.verify_batch(pks, msgs, sigs).all()
        whole = repeat(lambda: wall(verify), a.repeats, a.warmup)
        hashing = repeat(lambda: wall(hash_call), a.repeats, a.warmup)
        say("%s.verify_batch %s | hashing (host buffers in and out) %s | the rest, by difference of the medians %9.4f | %.1f k signatures/s"
            % (name, fmt(whole), fmt(hashing), statistics.median(whole) - statistics.median(hashing), m / statistics.median(whole)))
    say("   not built: encode_to_curve, mixed lengths on the device, a hash with a shorter addition chain for u, multi-GPU forms")


if __name__ == "__main__":
    main()
