#!/usr/bin/env python3
"""Batched Fr arithmetic (bn254_fr_{add,mul,inverse,pow,interpret}_batch) and groth16.verify_aggregate on one GPU, one process; every figure
is the median [min max] of --repeats runs after --warmup.
  kernel    kernel ms per operation (bn254_kernel_stats) of the _dev call at n = 1, 2^16, 2^20; for add and mul the bytes they move per
            second (96 n: two operands read, one result written) beside the floor, a device-to-device hipMemcpyAsync of 48 n bytes - the
            same 96 n bytes of traffic - timed in the same run
  wall      the host-buffer call (staging and copies included) against the Python-integer loop it replaces, at 2^16
  variants  at 2^20: inverse with run lengths 1 / 4 / 8 / 16, pow with windows of 1 / 2 / 4 bits (the library's process-wide overrides,
            internal: bn254_fr_set_inverse_run / bn254_fr_set_pow_window; the bytes do not depend on them, which is checked)
  aggregate groth16.verify_aggregate against groth16.verify_batch on the same block of 2^10 valid proofs with l = 2, wall ms
Everything printed is also written to --out (default profiles/r13_fr.txt).
usage: tools/time_fr.py [--repeats 5] [--warmup 1] [--lg 0,16,20] [--proofs 1024]"""
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
OPS = ("add", "mul", "inverse", "pow", "interpret")


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


def kernel_ms(eng, scope, call):
    import torch
    eng.profile(True); eng.profile_reset()
    torch.cuda.synchronize()
    call()
    torch.cuda.synchronize()
    ms = eng.kernel_stats(scope)[0]
    eng.profile(False)
    return ms


def wall_ms(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def groth16_block(rng, l, m):
    """a verifying key from a known trapdoor and m valid proofs (host Fr arithmetic for the trapdoor side)"""
    import bn_amd
    from bn_amd import Fr, G1, G2, groth16
    eng = bn_amd.api.default_engine()
    alpha, beta, gamma, delta = (Fr.random(rng) for _ in range(4))
    ic = [Fr.random(rng) for _ in range(l + 1)]
    g1, g2 = G1.one().limbs, G2.one().limbs
    pts = eng.g1_mul_batch(np.tile(g1, (l + 2, 1)), np.stack([alpha.limbs] + [c.limbs for c in ic]))
    q = eng.g2_mul_batch(np.tile(g2, (3, 1)), np.stack([beta.limbs, gamma.limbs, delta.limbs]))
    vk = groth16.VerifyingKey(G1(pts[0]), G2(q[0]), G2(q[1]), G2(q[2]), [G1(p) for p in pts[1:]])
    inputs = [[Fr.random(rng) for _ in range(l)] for _ in range(m)]
    a = [Fr.random(rng) for _ in range(m)]; b = [Fr.random(rng) for _ in range(m)]
    dinv = delta.inverse()
    c = []
    for ai, bi, inp in zip(a, b, inputs):
        s = ic[0]
        for x, w in zip(inp, ic[1:]):
            s = s + x * w
        c.append((ai * bi - alpha * beta - gamma * s) * dinv)
    AC = eng.g1_mul_batch(np.tile(g1, (2 * m, 1)), np.stack([x.limbs for x in a + c]))
    Bp = eng.g2_mul_batch(np.tile(g2, (m, 1)), np.stack([x.limbs for x in b]))
    return vk, [(G1(AC[i]), G2(Bp[i]), G1(AC[m + i])) for i in range(m)], inputs


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lg", default="0,16,20")
    ap.add_argument("--proofs", type=int, default=1 << 10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13_fr.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import Fr, _native, groth16
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    for fn in (lib.bn254_fr_inverse_run, lib.bn254_fr_pow_window):
        fn.argtypes = []; fn.restype = C.c_uint
    lib.bn254_fr_set_inverse_run.argtypes = [C.c_uint]; lib.bn254_fr_set_pow_window.argtypes = [C.c_uint]
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    K, WB = lib.bn254_fr_inverse_run(), lib.bn254_fr_pow_window()
    say("shipped library: inverse run length K = %d, pow window %d bits; median [min max] over %d runs after %d warm-up, one process" % (K, WB, a.repeats, a.warmup))
    lgs = [int(x) for x in a.lg.split(",")]
    nmax = 1 << max(lgs)
    s0 = torch.cuda.current_stream().cuda_stream
    A = torch.empty(nmax * 4, dtype=torch.int64, device=dev); B = torch.empty_like(A); O = torch.empty_like(A); O2 = torch.empty_like(A)
    OK = torch.empty(nmax, dtype=torch.int32, device=dev)
    eng.synthetic_scalars_dev(7, 0, nmax, 0, A.data_ptr(), s0); eng.synthetic_scalars_dev(7, 0, nmax, 1, B.data_ptr(), s0)
    BUF = torch.randint(0, 256, (nmax * 64,), dtype=torch.uint8, device=dev)
    CP_SRC = torch.zeros(nmax * 48, dtype=torch.uint8, device=dev); CP_DST = torch.empty_like(CP_SRC)      # the copy that sets the floor: 48 n bytes
    torch.cuda.synchronize()

    def dev_call(op, n, out=O):
        return {"add": lambda: eng.fr_add_batch_dev(A.data_ptr(), B.data_ptr(), out.data_ptr(), n, False, s0),
                "mul": lambda: eng.fr_mul_batch_dev(A.data_ptr(), B.data_ptr(), out.data_ptr(), n, s0),
                "inverse": lambda: eng.fr_inverse_batch_dev(A.data_ptr(), out.data_ptr(), OK.data_ptr(), n, s0),
                "pow": lambda: eng.fr_pow_batch_dev(A.data_ptr(), B.data_ptr(), out.data_ptr(), n, s0),
                "interpret": lambda: eng.fr_interpret_batch_dev(BUF.data_ptr(), out.data_ptr(), n, s0)}[op]

    say("-- kernel ms of the _dev calls")
    for lg in lgs:
        n = 1 << lg
        label = "n=%-5s" % ("1" if lg == 0 else "2^%d" % lg)
        med = {}
        for op in OPS:
            v = repeat(lambda: kernel_ms(eng, "fr_" + op, dev_call(op, n)), a.repeats, a.warmup)
            med[op] = statistics.median(v)
            say("%s fr_%-9s | kernel ms %s | %8.2f M elements/s" % (label, op, fmt(v), n / med[op] / 1e3))

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert hip.hipMemcpyAsync(CP_DST.data_ptr(), CP_SRC.data_ptr(), 48 * n, 3, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        v = repeat(copy, a.repeats, a.warmup)
        floor = statistics.median(v)
        say("%s d2d memcpy   | event  ms %s | 48 n bytes copied = 96 n bytes of traffic: %8.1f GB/s" % (label, fmt(v), 96 * n / floor / 1e6))
        for op in ("add", "mul"):
            say("%s fr_%-9s | 96 n bytes in %.4f ms = %8.1f GB/s, %.2f x the copy's time" % (label, op, med[op], 96 * n / med[op] / 1e6, med[op] / floor))

    say("-- wall ms at n = 2^16: the host-buffer call (staging, copies) against the Python-integer loop over Fr objects")
    n = 1 << 16
    ha = A[:n * 4].cpu().numpy().view(np.uint64).reshape(n, 4); hb = B[:n * 4].cpu().numpy().view(np.uint64).reshape(n, 4)
    hbuf = BUF[:n * 64].cpu().numpy().reshape(n, 64)
    fa = [Fr.from_limbs(x) for x in ha]; fb = [Fr.from_limbs(x) for x in hb]
    raw = [bytes(x) for x in hbuf]
    host = {"add": (lambda: eng.fr_add_batch(ha, hb), lambda: [x + y for x, y in zip(fa, fb)]),
            "mul": (lambda: eng.fr_mul_batch(ha, hb), lambda: [x * y for x, y in zip(fa, fb)]),
            "inverse": (lambda: eng.fr_inverse_batch(ha), lambda: [x.inverse() for x in fa]),
            "pow": (lambda: eng.fr_pow_batch(ha, hb), lambda: [x.pow(y) for x, y in zip(fa, fb)]),
            "interpret": (lambda: eng.fr_interpret_batch(hbuf), lambda: [Fr.interpret(x) for x in raw])}
    for op, (gpu, py) in host.items():
        vg = repeat(lambda: wall_ms(gpu), a.repeats, a.warmup)
        vp = repeat(lambda: wall_ms(py), 1 if op == "pow" else a.repeats, 0)
        say("n=2^16 fr_%-9s | host-buffer call %s | Python loop %s | %.0f x" % (op, fmt(vg), fmt(vp), statistics.median(vp) / statistics.median(vg)))

    say("-- variants at n = 2^%d, kernel ms" % max(lgs))
    ref = {}
    for op in ("inverse", "pow"):
        dev_call(op, nmax, O2)(); torch.cuda.synchronize(); ref[op] = O2.clone()
    best = {}
    try:
        for k in (1, 4, 8, 16):
            assert lib.bn254_fr_set_inverse_run(k) == 0
            v = repeat(lambda: kernel_ms(eng, "fr_inverse", dev_call("inverse", nmax)), a.repeats, a.warmup)
            assert torch.equal(O, ref["inverse"]), k
            best[("inverse", k)] = statistics.median(v)
            say("fr_inverse K=%-2d      | kernel ms %s%s" % (k, fmt(v), "   (shipped)" if k == K else ""))
        assert lib.bn254_fr_set_inverse_run(0) == 0
        for w in (1, 2, 4):
            assert lib.bn254_fr_set_pow_window(w) == 0
            v = repeat(lambda: kernel_ms(eng, "fr_pow", dev_call("pow", nmax)), a.repeats, a.warmup)
            assert torch.equal(O, ref["pow"]), w
            best[("pow", w)] = statistics.median(v)
            say("fr_pow window %d bits | kernel ms %s%s" % (w, fmt(v), "   (shipped)" if w == WB else ""))
    finally:
        lib.bn254_fr_set_inverse_run(0); lib.bn254_fr_set_pow_window(0)
    for op in ("inverse", "pow"):
        k = min((v, key[1]) for key, v in best.items() if key[0] == op)[1]
        say("fastest fr_%s variant: %d" % (op, k))

    m = a.proofs
    say("-- groth16: one block of %d valid proofs, l = 2, wall ms" % m)
    vk, proofs, inputs = groth16_block(np.random.default_rng(13), 2, m)
    assert groth16.verify_batch(vk, proofs, inputs).all() and groth16.verify_aggregate(vk, proofs, inputs)
    vb = repeat(lambda: wall_ms(lambda: groth16.verify_batch(vk, proofs, inputs)), a.repeats, a.warmup)
    va = repeat(lambda: wall_ms(lambda: groth16.verify_aggregate(vk, proofs, inputs)), a.repeats, a.warmup)
    say("verify_batch     (4 m Miller loops, m final exponentiations) | %s" % fmt(vb))
    say("verify_aggregate (m + 3 Miller loops, 1 final exponentiation) | %s" % fmt(va))
    say("verify_batch / verify_aggregate = %.2f (medians); ranges %s" % (statistics.median(vb) / statistics.median(va), "do not overlap" if max(va) < min(vb) or max(vb) < min(va) else "OVERLAP"))


if __name__ == "__main__":
    main()
