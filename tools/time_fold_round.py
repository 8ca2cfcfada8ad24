#!/usr/bin/env python3
"""The fused fold-then-round call (bn254_fr_sumcheck_fold_round_dev) and the resident sumcheck prover on one GPU, one process; every figure is
the median [min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev calls; tables are made on the
device by synthetic_scalars_dev.  Before anything is timed the bytes of everything compared are asserted equal (out of place, from the same
tables); the timed calls then run in place on a working copy, as a prover runs them.
  (a)  k = 4 tables (eq, A, B, C), degree 3, groups (1, [0,1,2]) and (r-1, [0,3]), input tables of n = 2^16 / 2^18 / 2^20 / 2^22 entries:
       the fused call at P = 4 / 8 / 16 (bn254_fr_sumcheck_fold_set_piece) and at the adaptive choice (nothing forced); beside it the
       composition it replaces - fr_mle_fold_dev in place, then fr_sumcheck_round_dev on n / 2 with the round's shipped piece -, a
       device-to-device copy of the 1.5 n k records the fused call must move, and fr_mul_batch_dev on the products it executes (per index of
       n / 4: two per table for the fold, and the round's)
  (b)  k = 1, degree 1, n = 2^24: the bandwidth case
  (c)  VGPRs, spill and waves per SIMD of the four new kernel instances, beside the round's four (tools/kernel_meta.py)
  (d)  a whole proof at nv = 20 over the four tables, three ways, each as the sum of its kernel time and as wall time: prove_resident with the
       fused call, the same loop with the two _dev calls per round, and prove through the host buffers
The rules, fixed before measuring: the fastest of P = 4 / 8 / 16 on (a) at 2^22 ships; the adaptive choice ships unless at some swept size it
is slower than the fixed shipped piece with non-overlapping [min, max]; prove_resident uses the fused call if the [min, max] of its
whole-proof kernel time lies wholly below that of the two-call loop.  Everything printed is also written to --out.
usage: tools/time_fold_round.py [--repeats 5] [--warmup 1] [--small]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
OUT = None
PIECES = (4, 8, 16)
FUSED = ("fr_sumcheck_fold_round", "fr_sumcheck_sum")
TWO = ("fr_mle_fold", "fr_sumcheck_round", "fr_sumcheck_sum")
ALL = ("fr_mle_fold", "fr_sumcheck_round", "fr_sumcheck_fold_round", "fr_sumcheck_sum")


def products(k, groups, degree):
    """Montgomery products the fused kernel executes per index of n / 4: the fold's two per table, and the round's - per group two for the
    coefficient and degree + 1 per further factor"""
    return 2 * k + sum(2 + (len(m) - 1) * (degree + 1) for _, m in groups)


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


def below(a, b):
    """the [min, max] of a lies wholly below that of b"""
    return max(a) < min(b)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="sizes divided by 2^6: a dry run of the tool, not a measurement")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r20_fold_round.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, sumcheck
    from bn_amd.api import R_MOD, Fr
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_fr_sumcheck_piece.argtypes = []; lib.bn254_fr_sumcheck_piece.restype = C.c_uint
    lib.bn254_fr_sumcheck_fold_piece.argtypes = []; lib.bn254_fr_sumcheck_fold_piece.restype = C.c_uint
    lib.bn254_fr_sumcheck_fold_set_piece.argtypes = [C.c_uint]
    lib.bn254_fr_sumcheck_fold_piece_for.argtypes = [C.c_size_t, C.c_size_t]; lib.bn254_fr_sumcheck_fold_piece_for.restype = C.c_uint
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P0, PR = lib.bn254_fr_sumcheck_fold_piece(), lib.bn254_fr_sumcheck_piece()
    sh = 6 if a.small else 0
    say("shipped library: fused piece P = %d (adaptive below %d lanes on %d compute units), round piece %d; kernel ms of the fused call = %s, of the two calls = %s; "
        "median [min max] over %d runs after %d warm-up, one process%s"
        % (P0, cus * 512, cus, PR, " + ".join('"%s"' % s for s in FUSED), " + ".join('"%s"' % s for s in TWO), a.repeats, a.warmup,
           "   ** --small: a dry run, not a measurement **" if a.small else ""))
    one, minus_one = Fr.one().limbs, Fr(R_MOD - 1).limbs
    r1cs = [(one, [0, 1, 2]), (minus_one, [0, 3])]
    r = Fr(0x1234567890abcdef1234567890abcdef).limbs
    shapes = [("a", 4, 3, r1cs, 1 << (e - sh)) for e in (16, 18, 20, 22)] + [("b", 1, 1, [(one, [0])], 1 << (24 - sh))]
    records = max(k * n for _, k, _, _, n in shapes)
    s0 = torch.cuda.current_stream().cuda_stream
    T = torch.empty(records * 4, dtype=torch.int64, device=dev)
    W = torch.empty_like(T)
    Fd = torch.empty(records * 2, dtype=torch.int64, device=dev)
    O = torch.empty(2 * 8 * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(17, 0, records, 0, T.data_ptr(), s0)
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
        assert nbytes <= W.numel() * 8 and hip.hipMemcpyAsync(W.data_ptr(), T.data_ptr(), nbytes, 3, s0) == 0     # W: the working copy, rewritten per shape
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    sweep = {}
    try:
        for name, k, degree, groups, n in shapes:
            h2, words = n // 4, (degree + 1) * 4
            say("-- (%s)  k = %d tables, degree %d, %d groups, n = %d entries per table: the fused call reads %d and writes %d bytes, %d products per index of n / 4"
                % (name, k, degree, len(groups), n, 32 * k * n, 16 * k * n, products(k, groups, degree)))
            # the bytes first, out of place from T: the two calls, then the fused call at every piece
            eng.fr_mle_fold_dev(T.data_ptr(), n * k, r, Fd.data_ptr(), s0)
            eng.fr_sumcheck_round_dev(Fd.data_ptr(), n // 2, k, groups, O.data_ptr(), degree, s0)
            torch.cuda.synchronize()
            ref_f, ref_o = Fd[:n // 2 * k * 4].clone(), O[:words].clone()
            for P in PIECES + (0,):
                assert lib.bn254_fr_sumcheck_fold_set_piece(P) == 0
                Fd.zero_(); O.zero_()
                eng.fr_sumcheck_fold_round_dev(T.data_ptr(), n, k, r, groups, Fd.data_ptr(), O.data_ptr(), degree, s0)
                torch.cuda.synchronize()
                assert torch.equal(Fd[:n // 2 * k * 4], ref_f) and torch.equal(O[:words], ref_o), (name, n, P)
            W[:n * k * 4].copy_(T[:n * k * 4])
            eng.fr_sumcheck_fold_round_dev(W.data_ptr(), n, k, r, groups, W.data_ptr(), O.data_ptr(), degree, s0)      # and in place
            torch.cuda.synchronize()
            assert torch.equal(W[:n // 2 * k * 4], ref_f) and torch.equal(W[n // 2 * k * 4:n * k * 4], T[n // 2 * k * 4:n * k * 4]) and torch.equal(O[:words], ref_o), (name, n)
            del ref_f
            fused = lambda: eng.fr_sumcheck_fold_round_dev(W.data_ptr(), n, k, r, groups, W.data_ptr(), O.data_ptr(), degree, s0)
            for P in PIECES + (0,):
                assert lib.bn254_fr_sumcheck_fold_set_piece(P) == 0
                eff = lib.bn254_fr_sumcheck_fold_piece_for(h2, cus)
                v = repeat(lambda: kernel_ms(FUSED, fused), a.repeats, a.warmup)
                sweep[name, n, P] = v
                ms = statistics.median(v)
                say("(%s) n = 2^%-2d fused, %-12s | kernel ms %s | %8.1f M indices/s | %7.1f GB/s moved%s"
                    % (name, n.bit_length() - 1, "P = %d" % P if P else "adaptive: %d" % eff, fmt(v), h2 / ms / 1e3, 48 * k * n / ms / 1e6, "   (shipped)" if P == P0 else ""))
            lib.bn254_fr_sumcheck_fold_set_piece(0)

            def two():
                eng.fr_mle_fold_dev(W.data_ptr(), n * k, r, W.data_ptr(), s0)
                eng.fr_sumcheck_round_dev(W.data_ptr(), n // 2, k, groups, O.data_ptr(), degree, s0)
            w = repeat(lambda: kernel_ms(TWO, two), a.repeats, a.warmup)
            sweep[name, n, "two"] = w
            v = sweep[name, n, 0]
            say("(%s) n = 2^%-2d fr_mle_fold_dev in place + fr_sumcheck_round_dev (P = %d) | kernel ms %s | the fused call (adaptive) is %.2f x faster; the [min max] ranges %s"
                % (name, n.bit_length() - 1, PR, fmt(w), statistics.median(w) / statistics.median(v), "do not overlap" if below(v, w) or below(w, v) else "OVERLAP"))
            c = repeat(lambda: copy_ms(24 * k * n), a.repeats, a.warmup)
            count = products(k, groups, degree) * h2
            part = count // 4
            X = torch.empty(part * 4, dtype=torch.int64, device=dev)
            mul4 = lambda: [eng.fr_mul_batch_dev(T.data_ptr(), T.data_ptr() + 32 * part, X.data_ptr(), part, s0) for _ in range(4)]
            m = repeat(lambda: kernel_ms(("fr_mul",), mul4), a.repeats, a.warmup)
            del X
            ms = statistics.median(v)
            say("(%s) n = 2^%-2d floors: d2d copy that moves the %d bytes | ms %s: the fused call takes %.2f x | fr_mul_batch_dev on %d elements (four calls) | kernel ms %s: %.2f x | nearer: %s"
                % (name, n.bit_length() - 1, 48 * k * n, fmt(c), ms / statistics.median(c), count, fmt(m), ms / statistics.median(m),
                   "the product floor" if abs(np.log(ms / statistics.median(m))) < abs(np.log(ms / statistics.median(c))) else "the copy floor"))
    finally:
        lib.bn254_fr_sumcheck_fold_set_piece(0)
    big = shapes[3][4]
    win = min((statistics.median(sweep["a", big, P]), P) for P in PIECES)[1]
    say("-- rule 1 (fixed before measuring): the fastest P on (a) at n = %d ships: P = %d (the library carries %d)" % (big, win, P0))
    worse = [n for name, _, _, _, n in shapes if name == "a" and below(sweep["a", n, P0], sweep["a", n, 0])]
    say("-- rule 2: the adaptive choice is slower than the fixed P = %d with non-overlapping [min, max] at: %s -> %s ships"
        % (P0, ", ".join("n = %d" % n for n in worse) or "no swept size", "the FIXED piece" if worse else "the adaptive choice"))
    for name, _, _, _, n in shapes[:4]:
        say("   n = 2^%-2d: adaptive %s against fixed P = %d %s: %.2f x" % (n.bit_length() - 1, fmt(sweep["a", n, 0]), P0, fmt(sweep["a", n, P0]),
                                                                          statistics.median(sweep["a", n, P0]) / statistics.median(sweep["a", n, 0])))

    say("-- (c) the round's four kernel instances and the four new ones (tools/kernel_meta.py): registers (VGPRs and AGPRs of 512), spill, waves per SIMD")
    try:
        meta = kernel_meta.instances()
        for nm in sorted(meta):
            if "FrSumcheckFoldRoundOp" in nm or "FrSumcheckRoundOp" in nm:
                m = meta[nm]
                say("   %-28s degree %s | %3d registers | spill %d | private %d | %d waves per SIMD"
                    % ("FrSumcheckFoldRoundOp" if "FoldRound" in nm else "FrSumcheckRoundOp", nm.split("ILi")[1][0], m["vgpr"], m["spill"], m["private"], 512 // (-(-m["vgpr"] // 8) * 8)))
    except Exception as exc:                                                                    # no llvm tools on this machine
        say("   not available here: %r" % (exc,))

    nvp = 20 - sh
    say("-- (d) a whole proof at nv = %d: four tables eq, A, B, C = A o B, degree 3" % nvp)
    np_n = 1 << nvp
    host = lambda t, cnt: t[:cnt * 4].cpu().numpy().view(np.uint64).reshape(cnt, 4)
    A, B = host(T, np_n), host(T[np_n * 4:], np_n)
    tables = np.stack([eng.fr_mle_eq(host(T[2 * np_n * 4:], nvp)), A, B, eng.fr_mul_batch(A, B)], axis=1)
    groups = [(Fr.one(), [0, 1, 2]), (Fr(R_MOD - 1), [0, 3])]
    ways = [("prove_resident, the fused call     ", lambda: sumcheck._prove_resident(tables, groups, None, eng, True)),
            ("prove_resident, two _dev calls     ", lambda: sumcheck._prove_resident(tables, groups, None, eng, False)),
            ("prove through the host buffers     ", lambda: sumcheck.prove(tables, groups, engine=eng))]
    proofs, kern = [], {}
    for label, fn in ways:
        def wall():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            proofs.append(fn())
            return (time.perf_counter() - t0) * 1e3
        kv = repeat(lambda: kernel_ms(ALL, fn), a.repeats, a.warmup)
        wv = repeat(wall, a.repeats, a.warmup)
        kern[label] = kv
        say("%s | kernel ms %s | wall ms %s" % (label, fmt(kv), fmt(wv)))
    assert all(p == proofs[0] for p in proofs) and proofs[0][0].claim == Fr.zero()
    f, t = kern[ways[0][0]], kern[ways[1][0]]
    say("-- rule 3: prove_resident uses the fused call if the [min, max] of its whole-proof kernel time lies wholly below that of the two-call loop: %s -> %s (the library carries FUSED = %s)"
        % ("it does" if below(f, t) else "it does NOT", "the fused call" if below(f, t) else "the two calls", sumcheck.FUSED))
    say("   whole-proof kernel time, two calls / fused: %.2f x" % (statistics.median(t) / statistics.median(f)))


if __name__ == "__main__":
    main()
