#!/usr/bin/env python3
"""Multilinear tables and sumcheck rounds over Fr (bn254_fr_mle_eq, bn254_fr_mle_fold, bn254_fr_sumcheck_round) on one GPU, one process; every
figure is the median [min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
The round, on three shapes:
  (a)  k = 4 tables (eq, A, B, C), degree 3, groups (1, [0,1,2]) and (r-1, [0,3]), n = 2^22 indices   - the Spartan / R1CS-style round
  (b)  the same at n = 2^16
  (c)  k = 1, degree 1, n = 2^24                                                                        - a plain sum of two halves
and for each of them piece lengths 4 / 8 / 16 / 32 through the library's process-wide override (internal: bn254_fr_sumcheck_set_piece; the
bytes do not depend on it, which is checked).  The rule for the shipped piece length was fixed before measuring: the fastest on (a) ships;
how far it is behind the best on (b) and (c) is recorded next to the choice.  The fan (16) is not swept.
Then, for the shipped setting on (a), in the same process:
  - a device-to-device hipMemcpyAsync that moves the 32 k n bytes the round must read
  - bn254_fr_mul_batch_dev on as many elements as the round executes products (PRODUCTS below: per index and group, two for the
    coefficient and degree + 1 per further factor), in four calls over the same buffers
  - the same round composed from existing _dev calls over table-major copies of the tables: the differences hi - lo once
    (fr_add_batch_dev), and per t the interpolated tables (t = 0: lo, t = 1: hi, then one fr_add_batch_dev per table), the product of the
    first two factors of the long group (fr_mul_batch_dev) and the two sums (fr_dot_batch_dev without an index, which multiplies the last
    factor in); the coefficients would be applied to the 2 (degree + 1) sums on the host
Then fold (len = 2^22) and eq (nv = 22) against a copy of the bytes they must move, eq also against nv fr_mul_batch_dev calls on 2^22
elements; and the whole bn_amd.sumcheck.prove at nv = 20 (four tables, host-buffer calls, wall time) against the integer model prover of
tests/mle_cases.py at nv = 12, EXTRAPOLATED per element.
Reported, not gated.  Everything printed is also written to --out (default profiles/r17_mle.txt).
usage: tools/time_mle.py [--repeats 5] [--warmup 1] [--small]"""
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
OUT = None
PIECES = (4, 8, 16, 32)
SCOPES = ("fr_sumcheck_round", "fr_sumcheck_sum")
COMPOSED = ("fr_add", "fr_mul", "fr_dot", "fr_dot_fold")


def products(groups, degree):
    """Montgomery products the round kernel executes per index: per group two for the coefficient and degree + 1 per further factor"""
    return sum(2 + (len(m) - 1) * (degree + 1) for _, m in groups)


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r17_mle.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import _native, sumcheck
    from bn_amd.api import R_MOD, Fr
    import mle_cases as MC
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_fr_sumcheck_piece.argtypes = []; lib.bn254_fr_sumcheck_piece.restype = C.c_uint
    lib.bn254_fr_sumcheck_fan.argtypes = []; lib.bn254_fr_sumcheck_fan.restype = C.c_uint
    lib.bn254_fr_sumcheck_set_piece.argtypes = [C.c_uint]
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    P0, F = lib.bn254_fr_sumcheck_piece(), lib.bn254_fr_sumcheck_fan()
    sh = 6 if a.small else 0
    say("shipped library: piece length P = %d, fan F = %d; kernel ms of the round = %s; median [min max] over %d runs after %d warm-up, one process%s"
        % (P0, F, " + ".join('"%s"' % s for s in SCOPES), a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    one, minus_one = Fr.one().limbs, Fr(R_MOD - 1).limbs
    r1cs = [(one, [0, 1, 2]), (minus_one, [0, 3])]
    shapes = [("a", 4, 3, r1cs, 1 << (22 - sh)), ("b", 4, 3, r1cs, 1 << (16 - sh)), ("c", 1, 1, [(one, [0])], 1 << (24 - sh))]
    records = max(k * n for _, k, _, _, n in shapes)
    s0 = torch.cuda.current_stream().cuda_stream
    T = torch.empty(records * 4, dtype=torch.int64, device=dev)
    O = torch.empty(8 * 4, dtype=torch.int64, device=dev)
    dst = torch.empty_like(T)
    eng.synthetic_scalars_dev(17, 0, records, 0, T.data_ptr(), s0)
    torch.cuda.synchronize()

    def kernel_ms(scopes, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        got = [eng.kernel_stats(s) for s in scopes]
        eng.profile(False)
        return sum(ms for ms, _ in got), [l for _, l in got]

    def copy_ms(nbytes):
        """a device-to-device copy of nbytes: it moves 2 * nbytes"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert hip.hipMemcpyAsync(dst.data_ptr(), T.data_ptr(), nbytes, 3, s0) == 0
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    best = {}
    try:
        for name, k, degree, groups, n in shapes:
            say("-- (%s)  k = %d tables, degree %d, %d groups, n = %d indices: %d bytes read, %d products per index" % (name, k, degree, len(groups), n, 32 * k * n, products(groups, degree)))
            call = lambda: eng.fr_sumcheck_round_dev(T.data_ptr(), n, k, groups, O.data_ptr(), degree, s0)
            lib.bn254_fr_sumcheck_set_piece(0)
            call(); torch.cuda.synchronize()
            ref = O[:(degree + 1) * 4].clone()
            for P in PIECES:
                assert lib.bn254_fr_sumcheck_set_piece(P) == 0
                call(); torch.cuda.synchronize()
                assert torch.equal(O[:(degree + 1) * 4], ref), (name, P)
                launches = kernel_ms(SCOPES, call)[1]
                v = repeat(lambda: kernel_ms(SCOPES, call)[0], a.repeats, a.warmup)
                best[name, P] = statistics.median(v)
                say("(%s) P = %-2d | kernel ms %s | %8.1f M indices/s | %7.1f GB/s read | launches: %d round, %d sum%s"
                    % (name, P, fmt(v), n / 2 / best[name, P] / 1e3, 32 * k * n / best[name, P] / 1e6, launches[0], launches[1], "   (shipped)" if P == P0 else ""))
            lib.bn254_fr_sumcheck_set_piece(0)
    finally:
        lib.bn254_fr_sumcheck_set_piece(0)
    win = min((best["a", P], P) for P in PIECES)[1]
    say("-- the rule (fixed before measuring): the fastest P on (a) ships: P = %d (the library carries %d)" % (win, P0))
    for name in ("b", "c"):
        t, p = min((best[name, P], P) for P in PIECES)
        say("   on (%s) P = %d takes %.4f ms against the best there, %.4f ms (P = %d): %+.1f %%" % (name, win, best[name, win], t, p, 100 * (best[name, win] / t - 1)))
    say("   the fan F = %d was not swept" % F)

    name, k, degree, groups, n = shapes[0]
    h = n // 2
    say("-- the shipped setting (P = %d) on (a) against its floors and against the same round composed from existing calls" % P0)
    call = lambda: eng.fr_sumcheck_round_dev(T.data_ptr(), n, k, groups, O.data_ptr(), degree, s0)
    v = repeat(lambda: kernel_ms(SCOPES, call)[0], a.repeats, a.warmup)
    ms = statistics.median(v)
    say("bn254_fr_sumcheck_round_dev                                  | kernel ms %s" % fmt(v))
    c = repeat(lambda: copy_ms(32 * k * n // 2), a.repeats, a.warmup)
    say("d2d copy that moves the %d bytes the round reads            | ms        %s | the round takes %.2f x" % (32 * k * n, fmt(c), ms / statistics.median(c)))
    count = products(groups, degree) * h
    part = count // 4
    X = torch.empty(part * 4, dtype=torch.int64, device=dev)
    mul4 = lambda: [eng.fr_mul_batch_dev(T.data_ptr(), T.data_ptr() + 32 * part, X.data_ptr(), part, s0) for _ in range(4)]
    m = repeat(lambda: kernel_ms(("fr_mul",), mul4)[0], a.repeats, a.warmup)
    say("fr_mul_batch_dev on %d elements (%d per index, four calls) | kernel ms %s | the round takes %.2f x" % (count, products(groups, degree), fmt(m), ms / statistics.median(m)))
    nearer = "the product floor" if abs(np.log(ms / statistics.median(m))) < abs(np.log(ms / statistics.median(c))) else "the copy floor"
    say("   nearer: %s" % nearer)
    del X
    # the composed round: table-major copies of the four tables, their differences, the running interpolated tables, one product array
    cols = [torch.empty(n * 4, dtype=torch.int64, device=dev) for _ in range(k)]
    for j, col in enumerate(cols):
        eng.synthetic_scalars_dev(18 + j, 0, n, 0, col.data_ptr(), s0)
    D = [torch.empty(h * 4, dtype=torch.int64, device=dev) for _ in range(k)]
    V = [torch.empty(h * 4, dtype=torch.int64, device=dev) for _ in range(k)]
    Pr = torch.empty(h * 4, dtype=torch.int64, device=dev)
    S = torch.empty(2 * (degree + 1) * 4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def composed():
        for j in range(k):
            eng.fr_add_batch_dev(cols[j].data_ptr() + 32 * h, cols[j].data_ptr(), D[j].data_ptr(), h, True, s0)
        for t in range(degree + 1):
            if t == 0:
                cur = [col.data_ptr() for col in cols]
            elif t == 1:
                cur = [col.data_ptr() + 32 * h for col in cols]
            else:
                for j in range(k):
                    eng.fr_add_batch_dev(cur[j], D[j].data_ptr(), V[j].data_ptr(), h, False, s0)
                cur = [x.data_ptr() for x in V]
            eng.fr_mul_batch_dev(cur[0], cur[1], Pr.data_ptr(), h, s0)
            eng.fr_dot_batch_dev(Pr.data_ptr(), None, cur[2], h, [0, h], 1, S.data_ptr() + 64 * t, s0)
            eng.fr_dot_batch_dev(cur[0], None, cur[3], h, [0, h], 1, S.data_ptr() + 64 * t + 32, s0)
    w = repeat(lambda: kernel_ms(COMPOSED, composed)[0], a.repeats, a.warmup)
    launches = kernel_ms(COMPOSED, composed)[1]
    overlap = max(v) >= min(w)
    say("the same round from fr_add / fr_mul / fr_dot _dev calls       | kernel ms %s | %d launches | the new call is %.2f x faster; the [min max] ranges %s"
        % (fmt(w), sum(launches), statistics.median(w) / ms, "OVERLAP" if overlap else "do not overlap"))
    del cols, D, V, Pr

    n2 = 1 << (22 - sh)
    say("-- fold and eq at 2^%d" % (22 - sh))
    r = Fr(12345).limbs
    f = repeat(lambda: kernel_ms(("fr_mle_fold",), lambda: eng.fr_mle_fold_dev(T.data_ptr(), n2, r, dst.data_ptr(), s0))[0], a.repeats, a.warmup)
    must = 48 * n2
    c = repeat(lambda: copy_ms(must // 2), a.repeats, a.warmup)
    say("bn254_fr_mle_fold_dev, len = %d (%d bytes to move)        | kernel ms %s | d2d copy of them %s | the fold takes %.2f x"
        % (n2, must, fmt(f), fmt(c), statistics.median(f) / statistics.median(c)))
    nv = 22 - sh
    Z = torch.empty(nv * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(30, 0, nv, 0, Z.data_ptr(), s0)
    e = repeat(lambda: kernel_ms(("fr_mle_eq",), lambda: eng.fr_mle_eq_dev(Z.data_ptr(), nv, dst.data_ptr(), s0))[0], a.repeats, a.warmup)
    must = 32 * n2
    c = repeat(lambda: copy_ms(must // 2), a.repeats, a.warmup)
    m = repeat(lambda: kernel_ms(("fr_mul",), lambda: eng.fr_mul_batch_dev(T.data_ptr(), T.data_ptr() + 32 * n2, dst.data_ptr(), n2, s0))[0], a.repeats, a.warmup)
    say("bn254_fr_mle_eq_dev, nv = %d (%d bytes written)           | kernel ms %s | d2d copy that moves them %s: %.2f x | %d x fr_mul_batch_dev on %d elements (%s each): %.2f x"
        % (nv, must, fmt(e), fmt(c), statistics.median(e) / statistics.median(c), nv, n2, fmt(m), statistics.median(e) / (nv * statistics.median(m))))

    nvp, nvm = 20 - sh, (12 - sh if a.small else 12)
    say("-- the whole sumcheck.prove at nv = %d: four tables eq, A, B, C = A o B, degree 3, host-buffer calls" % nvp)
    np_n = 1 << nvp
    host = lambda t, cnt: t[:cnt * 4].cpu().numpy().view(np.uint64).reshape(cnt, 4)
    A, B = host(T, np_n), host(T[np_n * 4:], np_n)
    tables = np.stack([eng.fr_mle_eq(host(T[2 * np_n * 4:], nvp)), A, B, eng.fr_mul_batch(A, B)], axis=1)
    groups = [(Fr.one(), [0, 1, 2]), (Fr(R_MOD - 1), [0, 3])]

    def prove_ms():
        t0 = time.perf_counter()
        proof, _ = sumcheck.prove(tables, groups, engine=eng)
        assert proof.claim == Fr.zero()
        return (time.perf_counter() - t0) * 1e3
    p = repeat(prove_ms, a.repeats, a.warmup)
    rows = MC.rows_of(1 << nvm, 4, 5)
    t0 = time.perf_counter()
    MC.prove(rows, [(1, [0, 1, 2]), (R_MOD - 1, [0, 3])], lambda s, g: 7 + s)
    model = (time.perf_counter() - t0) * 1e3
    say("sumcheck.prove, nv = %d (%d rounds, %d + %d calls)        | wall ms %s" % (nvp, nvp, nvp, nvp, fmt(p)))
    say("the integer model prover at nv = %d                        | wall ms %9.1f (one run) | EXTRAPOLATED per element to nv = %d: %.0f ms, %.0f x the GPU prover"
        % (nvm, model, nvp, model * (1 << (nvp - nvm)), model * (1 << (nvp - nvm)) / statistics.median(p)))
    say("   not built here: a factored eq table (low bits times high bits), a sweep of the fan; the fused fold-then-round call and the resident prover are timed by tools/time_fold_round.py")


if __name__ == "__main__":
    main()
