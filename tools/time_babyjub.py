#!/usr/bin/env python3
"""Baby Jubjub and EdDSA-Poseidon (bn254_bjj_{validate,add,mul}_batch_dev, bn254_eddsa_poseidon_{challenge,verify}_batch_dev) on one GPU, one process;
every figure is the median [min max] of --repeats runs after --warmup.  Kernel ms come from bn254_kernel_stats around the _dev call.
  - validate, add, mul, challenge and verify at n = 1, 2^16 and 2^20, on valid points and valid signatures (signed here: keys, nonces and the
    challenge on the device, S = rho + 8 hm s mod l in host integers)
  - beside each, two reference figures: (a) bn254_fr_mul_batch_dev on the number of field products the formulas execute - the count is printed;
    measured at 2^22 products and scaled linearly, because n times the count does not fit the device - and (b), for verify, the composition
    challenge + 2 x mul + add from the new calls themselves (the comparison of two points is not timed)
  - VGPRs and private bytes per kernel instance (tools/kernel_meta.py)
  - with --variants W1.so W2.so (two libraries from tools/build_variant.sh, UNITS=bn254_babyjub, with -DBN254_EDDSA_WINDOW=1 and =2): the rule for the
    joint window the verifier ships with, fixed before measuring - the smaller median of five bn254_eddsa_poseidon_verify_batch_dev runs over 2^18
    valid signatures ships (interleaved, events on the stream, equal statuses asserted; both must keep bn254_fr_decode_k's zero spills)
Reported, not gated.  Everything printed is also written to --out (default profiles/r25_babyjub.txt).
usage: tools/time_babyjub.py [--repeats 5] [--warmup 1] [--small] [--variants W1.so W2.so]"""
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

# field products per record, from the formulas of babyjub_ops.hpp (a product by the constants a or d counts as one; a fused matrix row of T
# elements counts as T products; the word-serial reductions of fr_from_mont are not counted)
ADD, DBL, INV = 11, 9, 2 + 127 * 3                     # unified addition; doubling; Fermat inversion with 2-bit windows (table, 127 windows)
POSEIDON6 = 8 * (6 * 3 + 36) + 60 * (3 + 36)            # 8 full and 60 partial rounds at width 6
MUL_CHAIN = 14 * ADD + 252 * DBL + 63 * ADD             # the table [2 .. 15]P, 63 windows of 4 doublings and one addition
JOINT = {1: 2 * ADD + 253 * (DBL + ADD), 2: DBL + ADD + 12 * ADD + 126 * (2 * DBL + ADD)}      # table and chain of the verifier per window width
PRODUCTS = {"validate": 5 + 1 + MUL_CHAIN, "add": 2 + ADD + INV + 2, "mul": 1 + MUL_CHAIN + INV + 2, "challenge": POSEIDON6}


def verify_products(w):
    return 10 + POSEIDON6 + 1 + 3 * DBL + JOINT[w] + 2


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


def ints(t):
    """(n*4,) int64 device tensor of Montgomery images -> list of integers"""
    a = t.cpu().numpy().view(np.uint64).reshape(-1, 4)
    from bn_amd.api import R_MOD
    inv = pow(1 << 256, -1, R_MOD)
    return [(int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192) * inv % R_MOD for r in a]


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="sizes divided by 2^6: a dry run of the tool, not a measurement")
    ap.add_argument("--variants", nargs=2, metavar=("W1.so", "W2.so"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r25_babyjub.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, babyjub as BJ
    from bn_amd.api import R_MOD
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    lib.bn254_eddsa_window.argtypes = []
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    shipped = lib.bn254_eddsa_window()
    say("shipped library: the verifier's joint window is %d bit(s) per scalar (a table of %d points); kernel ms; median [min max] over %d runs after %d warm-up, one process%s"
        % (shipped, 4 ** shipped, a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    s0 = torch.cuda.current_stream().cuda_stream
    n_big, n_sig = 1 << (20 - sh), 1 << (18 - sh)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1)).to(dev)
    i64 = lambda words: torch.empty(words, dtype=torch.int64, device=dev)

    # ---- inputs: n_sig valid signatures, tiled to n_big
    B = up(np.tile(BJ.point_limbs(BJ.B8), (n_sig, 1, 1)))
    SEC, RHO, MSG = i64(n_sig * 4), i64(n_sig * 4), i64(n_sig * 4)
    for j, t in enumerate((SEC, RHO, MSG)):
        eng.synthetic_scalars_dev(25 + j, 0, n_sig, 0, t.data_ptr(), s0)
    A, R8, HM = i64(n_sig * 8), i64(n_sig * 8), i64(n_sig * 4)
    eng.bjj_mul_batch_dev(B.data_ptr(), SEC.data_ptr(), A.data_ptr(), n_sig, s0)
    eng.bjj_mul_batch_dev(B.data_ptr(), RHO.data_ptr(), R8.data_ptr(), n_sig, s0)
    eng.eddsa_poseidon_challenge_batch_dev(A.data_ptr(), R8.data_ptr(), MSG.data_ptr(), HM.data_ptr(), n_sig, s0)
    torch.cuda.synchronize()
    s_int = [(rho + 8 * hm * sec) % BJ.L for sec, rho, hm in zip(ints(SEC), ints(RHO), ints(HM))]          # [rho]B8 = [rho mod l]B8: B8 has order l
    mont = np.array([[(v >> (64 * j)) & ((1 << 64) - 1) for j in range(4)] for v in (s * (1 << 256) % R_MOD for s in s_int)], np.uint64)
    S = up(mont)
    rep = n_big // n_sig
    A4, R84, S4, M4, K4 = A.repeat(rep), R8.repeat(rep), S.repeat(rep), MSG.repeat(rep), SEC.repeat(rep)
    O8, O4 = i64(n_big * 8), i64(n_big * 4)
    ST = torch.full((n_big,), -1, dtype=torch.int32, device=dev)
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
        mm = re.search(r"\d+(BjjValidateOp|BjjAddOp|BjjMulOp|EddsaChallengeOp|EddsaVerifyOp)E", name)
        if mm:
            say("%s<%s> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (kernel_meta.short_name(name), mm.group(1), m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    n_ref = 1 << (22 - sh)
    X = i64(n_ref * 4); Y = i64(n_ref * 4); Z = i64(n_ref * 4)
    eng.synthetic_scalars_dev(31, 0, n_ref, 0, X.data_ptr(), s0); eng.synthetic_scalars_dev(32, 0, n_ref, 0, Y.data_ptr(), s0)
    ref = repeat(lambda: kernel_ms(("fr_mul",), lambda: eng.fr_mul_batch_dev(X.data_ptr(), Y.data_ptr(), Z.data_ptr(), n_ref, s0)), a.repeats, a.warmup)
    per_product = statistics.median(ref) / n_ref
    say("-- reference (a): bn254_fr_mul_batch_dev on 2^%d products: kernel ms %s = %.3f ps per product (it moves 96 bytes per product; the chains keep theirs in registers)" % (22 - sh, fmt(ref), per_product * 1e9))

    calls = {
        "validate": (("bjj_validate",), lambda n: eng.bjj_validate_batch_dev(A4.data_ptr(), ST.data_ptr(), n, s0)),
        "add": (("bjj_add",), lambda n: eng.bjj_add_batch_dev(A4.data_ptr(), R84.data_ptr(), O8.data_ptr(), n, s0)),
        "mul": (("bjj_mul",), lambda n: eng.bjj_mul_batch_dev(A4.data_ptr(), K4.data_ptr(), O8.data_ptr(), n, s0)),
        "challenge": (("eddsa_poseidon_challenge",), lambda n: eng.eddsa_poseidon_challenge_batch_dev(A4.data_ptr(), R84.data_ptr(), M4.data_ptr(), O4.data_ptr(), n, s0)),
        "verify": (("eddsa_poseidon_verify",), lambda n: eng.eddsa_poseidon_verify_batch_dev(A4.data_ptr(), R84.data_ptr(), S4.data_ptr(), M4.data_ptr(), ST.data_ptr(), n, s0)),
    }
    med = {}
    for what, (scopes, call) in calls.items():
        count = verify_products(shipped) if what == "verify" else PRODUCTS[what]
        say("-- bn254_%s_batch_dev: %d field products per record" % (("bjj_" if what in ("validate", "add", "mul") else "eddsa_poseidon_") + what, count))
        for n in (1, 1 << (16 - sh), n_big):
            ST.fill_(-1)
            v = repeat(lambda: kernel_ms(scopes, lambda: call(n)), a.repeats, a.warmup)
            if what in ("validate", "verify"):
                assert not ST[:n].any().item(), "a valid record was rejected"
            ms = med[(what, n)] = statistics.median(v)
            line = "n = %-7d | kernel ms %s | %9.3f M/s | (a) fr_mul_batch_dev on %d x n products, scaled: %9.4f ms, the call takes %.2f x" % (n, fmt(v), n / ms / 1e3, count, per_product * count * n, ms / (per_product * count * n))
            if what == "verify":
                comp = med[("challenge", n)] + 2 * med[("mul", n)] + med[("add", n)]
                line += " | (b) challenge + 2 x mul + add: %9.4f ms, the call takes %.2f x" % (comp, ms / comp)
            say(line)

    if a.variants:
        say("-- the verifier's joint window, 1 bit against 2 bits per scalar: bn254_eddsa_poseidon_verify_batch_dev over 2^%d valid signatures through each library (tools/build_variant.sh, UNITS=bn254_babyjub), interleaved, events on the stream" % (18 - sh))
        libs = []
        for path in a.variants:
            l = C.CDLL(str(pathlib.Path(path).resolve()))
            l.bn254_eddsa_poseidon_verify_batch_dev.argtypes = _native.SIGNATURES["bn254_eddsa_poseidon_verify_batch_dev"]
            l.bn254_eddsa_window.argtypes = []
            libs.append(l)
        assert [l.bn254_eddsa_window() for l in libs] == [1, 2], "--variants takes the 1-bit library first, the 2-bit one second"
        sts = [torch.full((n_sig,), -1, dtype=torch.int32, device=dev) for _ in libs]
        # one wrong row, so that equal statuses say something
        S_bad = S.clone(); S_bad[4:8] = S[0:4]

        def one_run(k, s_buf):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert libs[k].bn254_eddsa_poseidon_verify_batch_dev(None, A.data_ptr(), R8.data_ptr(), s_buf.data_ptr(), MSG.data_ptr(), sts[k].data_ptr(), n_sig, s0) == 0
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        for k in (0, 1):
            one_run(k, S_bad)
        assert torch.equal(sts[0], sts[1]) and sts[0][1].item() == 6 and int(sts[0].count_nonzero().item()) == 1, "the two variants differ on a batch with one wrong row"
        times = ([], [])
        for r in range(a.warmup + a.repeats):
            for k in (0, 1):
                ms = one_run(k, S)
                if r >= a.warmup:
                    times[k].append(ms)
        assert torch.equal(sts[0], sts[1]) and not sts[0].any().item(), "the two variants differ in their statuses"
        for k, w in enumerate((1, 2)):
            say("W = %d (%d products per signature) | ms %s | %9.3f M signatures/s" % (w, verify_products(w), fmt(times[k]), n_sig / statistics.median(times[k]) / 1e3))
        m1, m2 = statistics.median(times[0]), statistics.median(times[1])
        say("the rule (fixed before measuring): the smaller median of the %d runs ships, both variants at zero spilled VGPRs -> W = %d (%.3f x the other); statuses are equal; the library measured above carries W = %d"
            % (a.repeats, 1 if m1 < m2 else 2, min(m1, m2) / max(m1, m2), shipped))
    say("   not built: Pedersen hash, point packing (the square root in Fr has 2-adicity 28), EdDSA-MiMC, a fixed-base table, BLAKE-512 key derivation, multi-GPU forms")


if __name__ == "__main__":
    main()
