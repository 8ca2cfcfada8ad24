#!/usr/bin/env python3
"""Poseidon hashes and Merkle trees over Fr (bn254_fr_poseidon_batch, bn254_fr_merkle_tree) on one GPU, one process; every figure is the
median [min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - hashes of arity 1 .. 4 at n = 1, 2^16, 2^20, each against two floors, as ratios: bn254_fr_mul_batch_dev on as many elements as the hash
    executes products ((R_F t + R_P) * 3 for the S-boxes + (R_F + R_P) t^2 for the matrix, per hash), and a device-to-device copy of the
    (arity + 1) * 32 n bytes the hash moves
  - the tree at log_n = 10, 16, 20: the whole call, and every level on its own (the same kernel on the level's size)
  - the same permutation composed from existing _dev calls at n = 2^16, arity 2: per round one fr_add_batch_dev for the constants (tiled per
    lane; the tiling is not counted), three fr_mul_batch_dev for the S-boxes (over all elements, or over element 0), one fr_dot_batch_dev for
    the matrix (segments of t terms over a column-major state); the digests are compared with the kernel's
  - the host wall time of bn_amd.merkle.Tree against the bn_amd.poseidon.hash_host loop at log_n = 10
  - the VGPRs and the waves per SIMD they allow of every kernel instance (tools/kernel_meta.py)
  - with --variants PLAIN.so FUSED.so (two libraries from tools/build_variant.sh, UNITS=bn254_poseidon, with -DBN254_POSEIDON_FUSED_ROW=0 and
    -DBN254_POSEIDON_FUSED_ROW=1): 2^20 hashes of arity 2 through each library, interleaved, timed by events on the stream, and the decision
    by the rule fixed before measuring - the fused row ships if its [min, max] lies wholly below the plain one's
Reported, not gated.  Everything printed is also written to --out (default profiles/r18_poseidon.txt).
usage: tools/time_poseidon.py [--repeats 5] [--warmup 1] [--small] [--variants PLAIN.so FUSED.so]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
OUT = None
COMPOSED = ("fr_add", "fr_mul", "fr_dot", "fr_dot_fold")


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
    ap.add_argument("--variants", nargs=2, metavar=("PLAIN.so", "FUSED.so"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r18_poseidon.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, merkle, poseidon
    from bn_amd.api import Fr
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    hip = C.CDLL(_native._preload_shared_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.bn254_fr_poseidon_fused_row.argtypes = []
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    fused = lib.bn254_fr_poseidon_fused_row()
    say("shipped library: matrix rows %s; kernel ms of \"fr_poseidon\" / \"fr_merkle_level\"; median [min max] over %d runs after %d warm-up, one process%s"
        % ("as ONE product-sum (fr_dot)" if fused else "as t products and t - 1 sums (plain)", a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    products = lambda t: (poseidon.R_F * t + poseidon.R_P[t]) * 3 + (poseidon.R_F + poseidon.R_P[t]) * t * t
    big = 1 << (20 - sh)
    chunk = 1 << (24 - sh)                                                      # elements of one fr_mul_batch_dev call of the product floor
    s0 = torch.cuda.current_stream().cuda_stream
    T = torch.empty(max(2 * chunk, 4 * big) * 4, dtype=torch.int64, device=dev)
    dst = torch.empty(chunk * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(17, 0, T.numel() // 4, 0, T.data_ptr(), s0)
    torch.cuda.synchronize()

    def kernel_ms(scopes, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        got = [eng.kernel_stats(s) for s in scopes]
        eng.profile(False)
        return sum(ms for ms, _ in got), sum(l for _, l in got)

    def copy_ms(nbytes):
        """a device-to-device copy of nbytes: it moves 2 * nbytes"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert hip.hipMemcpyAsync(dst.data_ptr(), T.data_ptr(), nbytes, 3, s0) == 0
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def mul_calls(count):
        full, rest = divmod(count, chunk)
        for _ in range(full):
            eng.fr_mul_batch_dev(T.data_ptr(), T.data_ptr() + 32 * chunk, dst.data_ptr(), chunk, s0)
        if rest:
            eng.fr_mul_batch_dev(T.data_ptr(), T.data_ptr() + 32 * chunk, dst.data_ptr(), rest, s0)

    say("-- kernel instances (tools/kernel_meta.py): VGPRs, the waves per SIMD they allow (512 registers, allocated in eights), spill, private bytes")
    for name, m in sorted(kernel_meta.instances(_native.LIB_PATH).items()):
        mm = __import__("re").search(r"\d+(FrPoseidonOp)ILi(\d)E", name)
        if mm:
            say("bn254_fr_decode_k<%s<%s>> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (mm.group(1), mm.group(2), m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    say("-- hashes: bn254_fr_poseidon_batch_dev")
    record = {}
    for arity in (1, 2, 3, 4):
        t = arity + 1
        for n in (1, 1 << (16 - sh), big):
            call = lambda: eng.fr_poseidon_batch_dev(T.data_ptr(), arity, dst.data_ptr(), n, s0)
            v = repeat(lambda: kernel_ms(("fr_poseidon",), call)[0], a.repeats, a.warmup)
            ms = statistics.median(v)
            count = products(t) * n
            m = repeat(lambda: kernel_ms(("fr_mul",), lambda: mul_calls(count))[0], a.repeats, a.warmup)
            moved = (arity + 1) * 32 * n
            c = repeat(lambda: copy_ms(max(moved // 2, 16)), a.repeats, a.warmup)
            record[arity, n] = v
            say("arity %d, n = %-7d | kernel ms %s | %9.3f M hashes/s | %d products per hash: fr_mul_batch_dev on %d elements %s, the hash takes %.2f x | d2d copy of the %d bytes moved %s, the hash takes %.1f x"
                % (arity, n, fmt(v), n / ms / 1e3, products(t), count, fmt(m), ms / statistics.median(m), moved, fmt(c), ms / statistics.median(c)))

    say("-- trees: bn254_fr_merkle_tree_dev, then every level on its own (bn254_fr_poseidon_batch_dev of arity 2 on the level's size)")
    for log_n in (10 - min(sh, 4), 16 - sh, 20 - sh):
        n = 1 << log_n
        nodes = torch.empty(n * 4, dtype=torch.int64, device=dev)
        call = lambda: eng.fr_merkle_tree_dev(T.data_ptr(), log_n, nodes.data_ptr(), s0)
        v = repeat(lambda: kernel_ms(("fr_merkle_level",), call)[0], a.repeats, a.warmup)
        launches = kernel_ms(("fr_merkle_level",), call)[1]
        say("log_n = %-2d | kernel ms %s | %d launches | %.3f M nodes/s" % (log_n, fmt(v), launches, (n - 1) / statistics.median(v) / 1e3))
        levels = []
        for l in range(log_n):
            cnt = n >> (l + 1)
            w = repeat(lambda: kernel_ms(("fr_poseidon",), lambda: eng.fr_poseidon_batch_dev(T.data_ptr(), 2, nodes.data_ptr(), cnt, s0))[0], a.repeats, a.warmup)
            levels.append(statistics.median(w))
            say("   level %-2d | %-7d hashes | kernel ms %s" % (l, cnt, fmt(w)))
        single = [x for x, l in zip(levels, range(log_n)) if n >> (l + 1) <= 64]
        say("   the levels sum to %.4f ms; the %d levels of at most one wave (<= 64 hashes) take %.4f ms of it, %.1f %%; level 0 takes %.4f ms"
            % (sum(levels), len(single), sum(single), 100 * sum(single) / sum(levels), levels[0]))
        del nodes

    n = 1 << (16 - sh)
    t = 3
    say("-- the same permutation (t = 3: a hash of arity 2) composed from existing _dev calls at n = %d" % n)
    Cs, M = poseidon.constants(t)
    X = T[:2 * n * 4].cpu().numpy().view(np.uint64).reshape(n, 2, 4)          # the kernel's input rows
    state = np.concatenate([np.zeros((n, 4), np.uint64), X[:, 0], X[:, 1]])   # column-major: [j][lane]
    S = [torch.from_numpy(state.view(np.int64).reshape(-1).copy()).to(dev), torch.empty(t * n * 4, dtype=torch.int64, device=dev)]
    S0 = S[0].clone()
    tmp = torch.empty(t * n * 4, dtype=torch.int64, device=dev)
    ctile = torch.empty(t * n * 4, dtype=torch.int64, device=dev)
    crec = torch.from_numpy(np.stack([Fr(c).limbs for c in Cs]).view(np.int64).reshape(-1).copy()).to(dev)
    coeff = np.empty((t, n, t, 4), np.uint64)
    index = np.empty((t, n, t), np.uint64)
    for i in range(t):
        for j in range(t):
            coeff[i, :, j] = Fr(M[i][j]).limbs
            index[i, :, j] = j * n + np.arange(n, dtype=np.uint64)
    d_coeff = torch.from_numpy(coeff.view(np.int64).reshape(-1).copy()).to(dev)
    d_index = torch.from_numpy(index.view(np.int64).reshape(-1).copy()).to(dev)
    offsets = np.arange(t * n + 1, dtype=np.uint64) * t
    half = poseidon.R_F // 2

    def composed():
        S[0].copy_(S0)
        cur = 0
        for rnd in range(poseidon.R_F + poseidon.R_P[t]):
            for i in range(t):                                                  # not counted: the round's constants, one per lane
                eng.tile_dev(crec.data_ptr() + 32 * (rnd * t + i), 32, n, ctile.data_ptr() + 32 * n * i, s0)
            p = S[cur].data_ptr()
            eng.fr_add_batch_dev(p, ctile.data_ptr(), p, t * n, False, s0)
            cnt = t * n if rnd < half or rnd >= half + poseidon.R_P[t] else n
            eng.fr_mul_batch_dev(p, p, tmp.data_ptr(), cnt, s0)
            eng.fr_mul_batch_dev(tmp.data_ptr(), tmp.data_ptr(), tmp.data_ptr(), cnt, s0)
            eng.fr_mul_batch_dev(tmp.data_ptr(), p, p, cnt, s0)
            eng.fr_dot_batch_dev(d_coeff.data_ptr(), d_index.data_ptr(), p, t * n, offsets, t * n, S[1 - cur].data_ptr(), s0)
            cur = 1 - cur
        return cur
    if hasattr(eng, "tile_dev"):
        cur = composed(); torch.cuda.synchronize()
        eng.fr_poseidon_batch_dev(T.data_ptr(), 2, dst.data_ptr(), n, s0); torch.cuda.synchronize()
        same = torch.equal(S[cur][:n * 4], dst[:n * 4])
        w = repeat(lambda: kernel_ms(COMPOSED, composed)[0], a.repeats, a.warmup)
        launches = kernel_ms(COMPOSED, composed)[1]
        v = record[2, n]
        say("composed: fr_add + 3 fr_mul + fr_dot per round           | kernel ms %s | %d launches | digests %s the kernel's" % (fmt(w), launches, "EQUAL" if same else "DIFFER FROM"))
        say("bn254_fr_poseidon_batch_dev, arity 2                      | kernel ms %s | the new call is %.1f x faster; the [min max] ranges %s"
            % (fmt(v), statistics.median(w) / statistics.median(v), "OVERLAP" if max(v) >= min(w) else "do not overlap"))
    del S, S0, tmp, ctile, d_coeff, d_index

    log_n = 10 - min(sh, 4)
    say("-- host wall time at log_n = %d: bn_amd.merkle.Tree (one host-buffer call) against the bn_amd.poseidon.hash_host loop" % log_n)
    leaves = T[:(1 << log_n) * 4].cpu().numpy().view(np.uint64).reshape(-1, 4)

    def tree_ms():
        t0 = time.perf_counter()
        tree = merkle.Tree(leaves, engine=eng)
        ms = (time.perf_counter() - t0) * 1e3
        tree_ms.root = tree.root
        return ms
    p = repeat(tree_ms, a.repeats, a.warmup)
    ints = [Fr.from_limbs(r).v for r in leaves]
    t0 = time.perf_counter()
    level = ints
    while len(level) > 1:
        level = [poseidon.hash_host(level[i:i + 2]) for i in range(0, len(level), 2)]
    host = (time.perf_counter() - t0) * 1e3
    assert level[0] == tree_ms.root.v
    say("merkle.Tree, %d leaves (conversion to Fr included)       | wall ms %s" % (1 << log_n, fmt(p)))
    say("the hash_host loop over the same tree                     | wall ms %9.1f (one run), %.0f x; the roots are equal" % (host, host / statistics.median(p)))

    if a.variants:
        say("-- the matrix row, plain against fused: 2^%d hashes of arity 2 through each library (tools/build_variant.sh, UNITS=bn254_poseidon), interleaved, events on the stream" % (20 - sh))
        libs = []
        for path in a.variants:
            l = C.CDLL(str(pathlib.Path(path).resolve()))
            l.bn254_fr_poseidon_batch_dev.argtypes = _native.SIGNATURES["bn254_fr_poseidon_batch_dev"]
            l.bn254_fr_poseidon_fused_row.argtypes = []
            libs.append(l)
        assert [l.bn254_fr_poseidon_fused_row() for l in libs] == [0, 1], "--variants takes the plain library first, the fused one second"
        outs = [torch.zeros(big * 4, dtype=torch.int64, device=dev) for _ in libs]

        def one(l, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert l.bn254_fr_poseidon_batch_dev(None, T.data_ptr(), 2, out.data_ptr(), big, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        times = ([], [])
        for rep in range(a.warmup + a.repeats):
            for k in (0, 1):
                ms = one(libs[k], outs[k])
                if rep >= a.warmup:
                    times[k].append(ms)
        assert torch.equal(outs[0], outs[1]), "the two variants differ in their bytes"
        say("plain row (t products, t - 1 sums, t reductions)          | ms %s" % fmt(times[0]))
        say("fused row (fr_dot: t product rows per word, 1 reduction)  | ms %s | %.3f x the plain one; the bytes are equal" % (fmt(times[1]), statistics.median(times[1]) / statistics.median(times[0])))
        wins = max(times[1]) < min(times[0])
        say("the rule (fixed before measuring): the fused row ships if its [min, max] lies wholly below the plain one's: %s -> the %s row ships (the library measured above carries the %s one)"
            % ("it does" if wins else "it does not", "fused" if wins else "plain", "fused" if fused else "plain"))
    say("   not built: the factored partial rounds (2 t - 1 products instead of t^2), a several-lanes-per-hash mapping for the top of a tree, Poseidon2, a sponge or transcript, trees of arity 4, multi-GPU forms")


if __name__ == "__main__":
    main()
