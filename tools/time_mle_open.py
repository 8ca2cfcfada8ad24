#!/usr/bin/env python3
"""The quotients of a multilinear opening (bn254_fr_mle_quotients) and bn_amd.mkzg.open on one GPU, one process; every figure is the median
[min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - bn254_fr_mle_quotients_dev at nv = 16 / 20 / 22 for rho = 1 / 2 / 3 / 4 levels per launch, through the library's process-wide override
    (internal: bn254_fr_mle_quotients_set_levels; the bytes do not depend on it, which is checked), with the register counts of the four
    kernel instances from tools/kernel_meta.py.  The rule for the shipped rho was fixed before measuring: the fastest on one table of 2^22
    records ships, an instance that spills being out of the sweep.
  - the same quotients composed from existing _dev calls: per variable one fr_add_batch_dev(negate_b) for the differences, written straight
    to their heap positions, and one fr_mle_fold_dev (the first out of place, the others in place) - 2 nv launches; equal bytes asserted
  - a device-to-device hipMemcpyAsync of n records, which moves the 2 n records the call must move (read a, write out)
  - wall time of mkzg.open at nv = 16 (host-buffer calls), split into its one fr_mle_quotients and its one g1_msm_batch
Reported, not gated: the ratio to the composition is a measurement in the same process, not a target.  Everything printed is also written
to --out (default profiles/r19_mle_open.txt).
usage: tools/time_mle_open.py [--repeats 5] [--warmup 1] [--small]"""
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
RHOS = (1, 2, 3, 4)
SCOPE = ("fr_mle_quotients",)
COMPOSED = ("fr_add", "fr_mle_fold")


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


def instances():
    """{rho: the metadata of its kernel instance}"""
    import kernel_meta
    meta = kernel_meta.instances(ROOT / "bn_amd" / "libbn254_hip.so")
    out = {}
    for name, m in meta.items():
        hit = re.search(r"\d+FrMleQuotOpILi(\d+)E", name)
        if hit:
            out[int(hit.group(1))] = m
    return out


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="sizes divided by 2^6: a dry run of the tool, not a measurement")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r19_mle_open.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    from bn_amd import _native, mkzg
    from bn_amd.api import Fr
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_fr_mle_quotients_levels.argtypes = []; lib.bn254_fr_mle_quotients_levels.restype = C.c_uint
    lib.bn254_fr_mle_quotients_set_levels.argtypes = [C.c_uint]
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    rho0 = int(lib.bn254_fr_mle_quotients_levels())
    sh = 6 if a.small else 0
    sizes = [16 - sh, 20 - sh, 22 - sh]
    top = max(sizes)
    say("shipped library: rho = %d levels per launch; kernel ms = \"%s\"; median [min max] over %d runs after %d warm-up, one process%s"
        % (rho0, SCOPE[0], a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    meta = instances()
    for rho in RHOS:
        m = meta.get(rho)
        say("instance rho = %d | %s" % (rho, "vgpr %(vgpr)d, sgpr %(sgpr)d, spilled vgpr %(spill)d, private bytes %(private)d, lds %(lds)d" % m if m else "NOT FOUND"))
    swept = [rho for rho in RHOS if rho in meta and meta[rho]["spill"] == 0 and meta[rho]["private"] == 0]
    say("in the sweep (no spill, no private memory): rho = %s" % ", ".join(map(str, swept)))

    s0 = torch.cuda.current_stream().cuda_stream
    n_top = 1 << top
    A = torch.empty(n_top * 4, dtype=torch.int64, device=dev)
    O = torch.empty(n_top * 4, dtype=torch.int64, device=dev)
    O2 = torch.empty(n_top * 4, dtype=torch.int64, device=dev)
    W = torch.empty(n_top // 2 * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(19, 0, n_top, 0, A.data_ptr(), s0)
    Zd = torch.empty(top * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(20, 0, top, 0, Zd.data_ptr(), s0)
    torch.cuda.synchronize()
    Z = Zd.cpu().numpy().view(np.uint64).reshape(top, 4)

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
        assert hip.hipMemcpyAsync(O2.data_ptr(), A.data_ptr(), nbytes, 3, s0) == 0
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def composed(nv):
        """the heap into O2 from 2 nv existing launches: the differences of level j go straight to records [2^j, 2^(j+1)), the folds keep the
        working table in W"""
        src = A.data_ptr()
        for j in range(nv - 1, -1, -1):
            half = 1 << j
            eng.fr_add_batch_dev(src + 32 * half, src, O2.data_ptr() + 32 * half, half, True, s0)
            eng.fr_mle_fold_dev(src, 2 * half, Z[j], W.data_ptr(), s0)
            src = W.data_ptr()
        assert hip.hipMemcpyAsync(O2.data_ptr(), W.data_ptr(), 32, 3, s0) == 0

    best = {}
    try:
        for nv in sizes:
            n = 1 << nv
            z = np.ascontiguousarray(Z[:nv])
            say("-- nv = %d: one table of n = %d records; the call must move 2 n records = %d bytes" % (nv, n, 64 * n))
            call = lambda: eng.fr_mle_quotients_dev(A.data_ptr(), z, O.data_ptr(), s0)
            O2.zero_(); composed(nv); torch.cuda.synchronize()
            ref = O2[:n * 4].clone()
            for rho in RHOS:
                assert lib.bn254_fr_mle_quotients_set_levels(rho) == 0
                O.zero_(); call(); torch.cuda.synchronize()
                assert torch.equal(O[:n * 4], ref), (nv, rho)                                   # equal bytes: every rho and the composition
                launches = kernel_ms(SCOPE, call)[1][0]
                v = repeat(lambda: kernel_ms(SCOPE, call)[0], a.repeats, a.warmup)
                best[nv, rho] = statistics.median(v)
                say("nv = %-2d rho = %d | kernel ms %s | %8.1f M records/s | %7.1f GB/s moved | %2d launches%s%s"
                    % (nv, rho, fmt(v), n / best[nv, rho] / 1e3, 64 * n / best[nv, rho] / 1e6, launches, "   (shipped)" if rho == rho0 else "", "" if rho in swept else "   (out of the sweep)"))
            assert lib.bn254_fr_mle_quotients_set_levels(0) == 0
            w = repeat(lambda: kernel_ms(COMPOSED, lambda: composed(nv))[0], a.repeats, a.warmup)
            launches = kernel_ms(COMPOSED, lambda: composed(nv))[1]
            assert sum(launches) == 2 * nv, launches
            say("nv = %-2d composed from fr_add_batch_dev(negate_b) and fr_mle_fold_dev, %d launches | kernel ms %s | the shipped rho = %d takes %.2f x of it (%.2f x faster)"
                % (nv, sum(launches), fmt(w), rho0, best[nv, rho0] / statistics.median(w), statistics.median(w) / best[nv, rho0]))
            c = repeat(lambda: copy_ms(32 * n), a.repeats, a.warmup)
            say("nv = %-2d d2d copy of n records (moves the same %d bytes)                         | ms        %s | the shipped rho = %d takes %.2f x"
                % (nv, 64 * n, fmt(c), rho0, best[nv, rho0] / statistics.median(c)))
    finally:
        lib.bn254_fr_mle_quotients_set_levels(0)
    t, win = min((best[top, rho], rho) for rho in swept)
    say("-- the rule (fixed before measuring): the fastest rho in the sweep on one table of 2^%d records ships: rho = %d, %.4f ms (the library carries %d)" % (top, win, t, rho0))
    for nv in sizes[:-1]:
        t, r = min((best[nv, rho], rho) for rho in swept)
        say("   at nv = %d rho = %d takes %.4f ms against the best there, %.4f ms (rho = %d): %+.1f %%" % (nv, win, best[nv, win], t, r, 100 * (best[nv, win] / t - 1)))
    del O2, W

    nvo = 16 - sh
    say("-- mkzg.open at nv = %d (host-buffer calls, wall ms): one fr_mle_quotients, one g1_msm_batch of %d segments over %d terms" % (nvo, nvo, (1 << nvo) - 1))
    srs = mkzg.setup(nvo, np.random.default_rng(7), engine=eng)
    table = A[:(4 << nvo)].cpu().numpy().view(np.uint64).reshape(-1, 4)
    point = [Fr.from_limbs(r) for r in Z[:nvo]]
    zl = np.ascontiguousarray(Z[:nvo])
    offsets = np.array([(1 << j) - 1 for j in range(nvo + 1)], np.uint64)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    whole = repeat(lambda: wall(lambda: mkzg.open(srs, table, point, engine=eng)), a.repeats, a.warmup)
    heap = eng.fr_mle_quotients(table, zl)
    q = repeat(lambda: wall(lambda: eng.fr_mle_quotients(table, zl)), a.repeats, a.warmup)
    m = repeat(lambda: wall(lambda: eng.g1_msm_batch(srs.g1_levels[1:1 << nvo], heap[1:], offsets)), a.repeats, a.warmup)
    y, proofs = mkzg.open(srs, table, point, engine=eng)
    assert mkzg.verify(srs, mkzg.commit(srs, table, engine=eng), point, y, proofs, engine=eng)
    say("mkzg.open                       | wall ms %s" % fmt(whole))
    say("  its fr_mle_quotients          | wall ms %s | %.1f %% of the whole" % (fmt(q), 100 * statistics.median(q) / statistics.median(whole)))
    say("  its g1_msm_batch              | wall ms %s | %.1f %% of the whole" % (fmt(m), 100 * statistics.median(m) / statistics.median(whole)))
    say("   the opening verifies; not built: opening several tables at one point, a random-linear-combination verify, a bucket-method route for the top proof levels")


if __name__ == "__main__":
    main()
