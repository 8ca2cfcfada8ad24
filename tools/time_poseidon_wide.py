#!/usr/bin/env python3
"""Wide Poseidon over Fr (bn254_fr_poseidon_ex_batch, bn254_fr_poseidon_chain_batch) on one GPU, one process; every figure is the median [min max] of
--repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - with --variants G4.so G8.so G16.so (three libraries from tools/build_variant.sh, UNITS=bn254_poseidon_wide, with -DBN254_POSEIDON_WIDE_LANES=4 / 8 /
    16): 2^16 rows of 16 inputs through bn254_fr_poseidon_ex_batch_dev of each library, interleaved, timed by events on the stream, equal bytes
    asserted, and the decision by the rule fixed before measuring - the smallest median of five runs ships
  - the shipped library: PoseidonEx at n = 1, 2^16, 2^20 for n_inputs = 2, 4, 8, 16, each beside bn254_fr_mul_batch_dev on as many elements as the
    permutation executes products ((R_F t + R_P) * 3 for the S-boxes + (R_F + R_P) t^2 for the matrix), and - n_inputs 2 and 4 - beside
    bn254_fr_poseidon_batch_dev, which does the same work in one lane per hash (equal bytes asserted)
  - the chain call on 2^16 records of 1 .. 40 elements at rate 16
  - VGPRs, spill, LDS bytes and waves per SIMD of each Op (tools/kernel_meta.py)
Reported, not gated.  Everything printed is also written to --out (default profiles/r27_poseidon_wide.txt).
usage: tools/time_poseidon_wide.py [--repeats 5] [--warmup 1] [--small] [--variants G4.so G8.so G16.so] [--note TEXT ...]"""
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


def say(line):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def fmt(v):
    return "%10.4f [%10.4f %10.4f]" % (statistics.median(v), min(v), max(v))


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
    ap.add_argument("--variants", nargs=3, metavar=("G4.so", "G8.so", "G16.so"))
    ap.add_argument("--note", action="append", default=[], help="a line copied into the report (the build times, taken on the build machine)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r27_poseidon_wide.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, poseidon
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    lib.bn254_fr_poseidon_wide_lanes.argtypes = []
    lib.bn254_fr_poseidon_wide_block.argtypes = []
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    G, block = lib.bn254_fr_poseidon_wide_lanes(), lib.bn254_fr_poseidon_wide_block()
    say("shipped library: %d lanes per permutation, workgroups of %d lanes; kernel ms of \"fr_poseidon_ex\" / \"fr_poseidon_chain\"; median [min max] over %d runs after %d warm-up, one process%s"
        % (G, block, a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    for note in a.note:
        say(note)
    products = lambda t: (poseidon.R_F * t + poseidon.R_P[t]) * 3 + (poseidon.R_F + poseidon.R_P[t]) * t * t
    big = 1 << (20 - sh)
    mid = 1 << (16 - sh)
    chunk = 1 << (24 - sh)                                                      # elements of one fr_mul_batch_dev call of the product floor
    s0 = torch.cuda.current_stream().cuda_stream
    T = torch.empty(max(2 * chunk, 17 * big) * 4, dtype=torch.int64, device=dev)
    dst = torch.empty(chunk * 4, dtype=torch.int64, device=dev)
    dst2 = torch.empty(big * 4, dtype=torch.int64, device=dev)
    eng.synthetic_scalars_dev(27, 0, T.numel() // 4, 0, T.data_ptr(), s0)
    torch.cuda.synchronize()

    def kernel_ms(scopes, call):
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        got = [eng.kernel_stats(s) for s in scopes]
        eng.profile(False)
        return sum(ms for ms, _ in got)

    def mul_calls(count):
        full, rest = divmod(count, chunk)
        for _ in range(full):
            eng.fr_mul_batch_dev(T.data_ptr(), T.data_ptr() + 32 * chunk, dst.data_ptr(), chunk, s0)
        if rest:
            eng.fr_mul_batch_dev(T.data_ptr(), T.data_ptr() + 32 * chunk, dst.data_ptr(), rest, s0)

    if a.variants:
        say("-- lanes per permutation: 2^%d rows of 16 inputs through bn254_fr_poseidon_ex_batch_dev of each library (tools/build_variant.sh, UNITS=bn254_poseidon_wide), interleaved, events on the stream"
            % (16 - sh))
        libs = []
        for path in a.variants:
            l = C.CDLL(str(pathlib.Path(path).resolve()))
            l.bn254_fr_poseidon_ex_batch_dev.argtypes = _native.SIGNATURES["bn254_fr_poseidon_ex_batch_dev"]
            l.bn254_fr_poseidon_wide_lanes.argtypes = []
            libs.append(l)
        assert [l.bn254_fr_poseidon_wide_lanes() for l in libs] == [4, 8, 16], "--variants takes the libraries of 4, 8 and 16 lanes in this order"
        outs = [torch.zeros(mid * 4, dtype=torch.int64, device=dev) for _ in libs]

        def one(l, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert l.bn254_fr_poseidon_ex_batch_dev(None, T.data_ptr(), 16, None, 1, out.data_ptr(), mid, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        times = ([], [], [])
        for rep in range(a.warmup + a.repeats):
            for k in range(3):
                ms = one(libs[k], outs[k])
                if rep >= a.warmup:
                    times[k].append(ms)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "the variants differ in their bytes"
        for k, g in enumerate((4, 8, 16)):
            say("G = %-2d | ms %s | %9.3f k permutations/s" % (g, fmt(times[k]), mid / statistics.median(times[k])))
        best = min(range(3), key=lambda k: statistics.median(times[k]))
        say("the bytes of the three are equal.  The rule (fixed before measuring): the smallest median of %d runs ships -> G = %d (the library measured below carries G = %d)"
            % (a.repeats, (4, 8, 16)[best], G))

    say("-- kernel instances (tools/kernel_meta.py): VGPRs, the waves per SIMD they allow (512 registers, allocated in eights), spill, private bytes, LDS bytes per workgroup")
    for name, m in sorted(kernel_meta.instances(_native.LIB_PATH).items()):
        mm = re.search(r"\d+(FrPoseidonWide\w+?Op)ILi(\d+)E", name)
        if mm:
            say("bn254_fr_decode_k<%s<%s>> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | LDS %d | %d SGPRs"
                % (mm.group(1), mm.group(2), m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["lds"], m["sgpr"]))

    say("-- PoseidonEx: bn254_fr_poseidon_ex_batch_dev (init NULL, one output)")
    for n_inputs in (2, 4, 8, 16):
        t = n_inputs + 1
        for n in (1, mid, big):
            call = lambda: eng.fr_poseidon_ex_batch_dev(T.data_ptr(), n_inputs, None, 1, dst2.data_ptr(), n, s0)
            v = repeat(lambda: kernel_ms(("fr_poseidon_ex",), call), a.repeats, a.warmup)
            ms = statistics.median(v)
            count = products(t) * n
            m = repeat(lambda: kernel_ms(("fr_mul",), lambda: mul_calls(count)), a.repeats, a.warmup)
            line = ("n_inputs %2d, n = %-7d | kernel ms %s | %9.3f k permutations/s | %d products each: fr_mul_batch_dev on %d elements %s, the call takes %.2f x"
                    % (n_inputs, n, fmt(v), n / ms, products(t), count, fmt(m), ms / statistics.median(m)))
            if n_inputs <= 4:
                ref = torch.empty(n * 4, dtype=torch.int64, device=dev)
                w = repeat(lambda: kernel_ms(("fr_poseidon",), lambda: eng.fr_poseidon_batch_dev(T.data_ptr(), n_inputs, ref.data_ptr(), n, s0)), a.repeats, a.warmup)
                torch.cuda.synchronize()
                assert torch.equal(ref, dst2[:n * 4]), "the wide kernel and the one-lane kernel differ"
                line += " | bn254_fr_poseidon_batch_dev (one lane per hash, equal bytes) %s, the call takes %.2f x" % (fmt(w), ms / statistics.median(w))
            say(line)

    m_rec = mid
    lengths = (np.arange(m_rec, dtype=np.uint64) * 2654435761 % 40 + 1).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    blocks = int(np.maximum(1, -(-lengths.astype(np.int64) // 16)).sum())
    say("-- the chain: bn254_fr_poseidon_chain_batch_dev on %d records of 1 .. 40 elements (%d elements, %d blocks) at rate 16" % (m_rec, int(off[-1]), blocks))
    v = repeat(lambda: kernel_ms(("fr_poseidon_chain",), lambda: eng.fr_poseidon_chain_batch_dev(T.data_ptr(), off, 16, dst2.data_ptr(), s0)), a.repeats, a.warmup)
    w = repeat(lambda: kernel_ms(("fr_poseidon_ex",), lambda: eng.fr_poseidon_ex_batch_dev(T.data_ptr(), 16, None, 1, dst2.data_ptr(), blocks, s0)), a.repeats, a.warmup)
    say("chain                                   | kernel ms %s | %9.3f k records/s, %9.3f k blocks/s" % (fmt(v), m_rec / statistics.median(v), blocks / statistics.median(v)))
    say("PoseidonEx on as many rows as blocks    | kernel ms %s | the chain takes %.2f x" % (fmt(w), statistics.median(v) / statistics.median(w)))
    say("   not built: an additive sponge, the factored partial rounds (2 t - 1 products instead of t^2), rerouting the small calls or the top of a tree onto these kernels, Poseidon2, multi-GPU forms")


if __name__ == "__main__":
    main()
