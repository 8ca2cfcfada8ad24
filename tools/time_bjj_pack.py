#!/usr/bin/env python3
"""The square root in Fr, Baby Jubjub point packing and the packed EdDSA-Poseidon verifier (bn254_fr_sqrt_batch_dev, bn254_bjj_{pack,unpack}_batch_dev,
bn254_eddsa_poseidon_verify_packed_batch_dev) on one GPU, one process; every figure is the median [min max] of --repeats runs after --warmup.
Kernel ms come from bn254_kernel_stats around the _dev call.
  - fr_sqrt in both forms of the correction (the internal override bn254_fr_set_sqrt_form), pack, unpack and the packed verifier at n = 1, 2^16
    and 2^20, on random elements (about half are squares), valid points and valid signatures (signed here like tools/time_babyjub.py)
  - beside each: bn254_fr_pow_batch_dev on as many elements (one 254-bit exponentiation each), a device-to-device copy of the bytes the call
    moves (events on the stream), and the field products of the formulas per record, as in profiles/r25_babyjub.txt
  - the packed verifier against bn254_eddsa_poseidon_verify_batch_dev on the same signatures unpacked, and against the composition of two unpack
    calls and that call
  - the rule for the form of the square root that ships, fixed before measuring: the smaller median of five bn254_bjj_unpack_batch_dev runs over
    2^20 valid packed points ships (both forms are in the library behind bn254_bjj_set_sqrt_form; interleaved; equal output bytes asserted)
  - VGPRs, spills and private bytes of each new kernel instance (tools/kernel_meta.py)
Reported, not gated.  Everything printed is also written to --out (default profiles/r26_bjj_pack.txt).
usage: tools/time_bjj_pack.py [--repeats 5] [--warmup 1] [--small]"""
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
import gen_fr_sqrt_constants as G  # noqa: E402
from time_babyjub import fmt, repeat, ints, verify_products  # noqa: E402

OUT = None

# field products per record, from the formulas of fr_sqrt_ops.hpp and babyjub_ops.hpp (squarings count as products; compares, selects and the
# word-serial reductions of fr_from_mont are not counted)
_E = (G.T - 1) // 2
_DIGITS = [(_E >> (4 * i)) & 15 for i in range((_E.bit_length() + 3) // 4)]
CHAIN = 14 + 4 * (len(_DIGITS) - 1) + sum(1 for d in _DIGITS[:-1] if d)          # the table, 4 squarings per window, a product per non-zero digit
RATIO = 2 * 27 + 3 + CHAIN + 1 + 3                                                # v^(2^28 - 1), u V^2 v, the chain, W, x / w / b
CORRECT = {0: 351 + 27 + 2 * 27, 1: 84 + 7 + 2 * 7 + 1}                           # Tonelli-Shanks: squarings of tt, of cc, z cc and tt cc; logarithm: squarings, b g, g and h, x h
SQRT = {f: RATIO + CORRECT[f] for f in (0, 1)}
UNPACK = {f: 1 + 1 + 1 + SQRT[f] for f in (0, 1)}                                 # y to Montgomery form, y^2, d y^2


def say(line):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="sizes divided by 2^6: a dry run of the tool, not a measurement")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r26_bjj_pack.txt"))
    a = ap.parse_args()
    import torch
    import bn_amd
    import kernel_meta
    from bn_amd import _native, babyjub as BJ
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    OUT = open(a.out, "w")
    lib = _native.lib()
    lib.bn254_fr_set_sqrt_form.argtypes = [C.c_int]
    lib.bn254_bjj_set_sqrt_form.argtypes = [C.c_int]
    eng = bn_amd.api.default_engine()
    dev = torch.device("cuda", 0)
    sh = 6 if a.small else 0
    shipped, window = lib.bn254_fr_sqrt_form(), lib.bn254_eddsa_window()
    say("shipped library: form %d of the square root's correction (0 constant-flow Tonelli-Shanks, 1 digit-wise logarithm); kernel ms; median [min max] over %d runs after %d warm-up, one process%s"
        % (shipped, a.repeats, a.warmup, "   ** --small: a dry run, not a measurement **" if a.small else ""))
    s0 = torch.cuda.current_stream().cuda_stream
    n_big, n_sig = 1 << (20 - sh), 1 << (16 - sh)
    sizes = (1, 1 << (16 - sh), n_big)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1)).to(dev)
    i64 = lambda words: torch.empty(words, dtype=torch.int64, device=dev)

    # ---- inputs: n_sig valid signatures, packed on the device, tiled to n_big
    B = up(np.tile(BJ.point_limbs(BJ.B8), (n_sig, 1, 1)))
    SEC, RHO, MSG = i64(n_sig * 4), i64(n_sig * 4), i64(n_sig * 4)
    for j, t in enumerate((SEC, RHO, MSG)):
        eng.synthetic_scalars_dev(26 + j, 0, n_sig, 0, t.data_ptr(), s0)
    A, R8, HM = i64(n_sig * 8), i64(n_sig * 8), i64(n_sig * 4)
    eng.bjj_mul_batch_dev(B.data_ptr(), SEC.data_ptr(), A.data_ptr(), n_sig, s0)
    eng.bjj_mul_batch_dev(B.data_ptr(), RHO.data_ptr(), R8.data_ptr(), n_sig, s0)
    eng.eddsa_poseidon_challenge_batch_dev(A.data_ptr(), R8.data_ptr(), MSG.data_ptr(), HM.data_ptr(), n_sig, s0)
    A32, R32 = i64(n_sig * 4), i64(n_sig * 4)
    eng.bjj_pack_batch_dev(A.data_ptr(), A32.data_ptr(), n_sig, s0)
    eng.bjj_pack_batch_dev(R8.data_ptr(), R32.data_ptr(), n_sig, s0)
    torch.cuda.synchronize()
    s_int = [(rho + 8 * hm * sec) % BJ.L for sec, rho, hm in zip(ints(SEC), ints(RHO), ints(HM))]
    words = lambda vals: np.array([[(v >> (64 * j)) & ((1 << 64) - 1) for j in range(4)] for v in vals], np.uint64)
    S_RAW, S_MONT = up(words(s_int)), up(words(s * (1 << 256) % G.R for s in s_int))
    SIG = torch.stack([R32.view(-1, 4), S_RAW.view(-1, 4)], 1).reshape(-1).contiguous()            # 64 bytes per signature: the packed R8, then S
    rep = n_big // n_sig
    A4, R84, S4, M4, A324, R324, SIG4 = (t.repeat(rep) for t in (A, R8, S_MONT, MSG, A32, R32, SIG))
    X = i64(n_big * 4); E = i64(n_big * 4)
    eng.synthetic_scalars_dev(33, 0, n_big, 0, X.data_ptr(), s0); eng.synthetic_scalars_dev(34, 0, n_big, 0, E.data_ptr(), s0)
    O8, O8b, O4, O4b = i64(n_big * 8), i64(n_big * 8), i64(n_big * 4), i64(n_big * 4)
    ST = torch.full((n_big,), -1, dtype=torch.int32, device=dev)
    ST2 = torch.full((n_big,), -1, dtype=torch.int32, device=dev)
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
        src, dst = torch.empty(max(nbytes // 2, 8), dtype=torch.uint8, device=dev), torch.empty(max(nbytes // 2, 8), dtype=torch.uint8, device=dev)
        def one():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        return repeat(one, a.repeats, a.warmup)

    say("-- kernel instances (tools/kernel_meta.py): VGPRs, the waves per SIMD they allow (512 registers, allocated in eights), spill, private bytes")
    for name, m in sorted(kernel_meta.instances(_native.LIB_PATH).items()):
        mm = re.search(r"\d+(FrSqrtOp|BjjPackOp|BjjUnpackOp|EddsaVerifyPackedOp|EddsaVerifyOp)(?:ILi(\d)E)?E", name)
        if mm:
            say("%s<%s%s> | %3d VGPRs | %d waves per SIMD | spill %d | private %d | %d SGPRs"
                % (kernel_meta.short_name(name), mm.group(1), "<%s>" % mm.group(2) if mm.group(2) else "", m["vgpr"], min(8, 512 // (-(-m["vgpr"] // 8) * 8)), m["spill"], m["private"], m["sgpr"]))

    pow_ms = {n: statistics.median(repeat(lambda: kernel_ms(("fr_pow",), lambda: eng.fr_pow_batch_dev(X.data_ptr(), E.data_ptr(), O4.data_ptr(), n, s0)), a.repeats, a.warmup)) for n in sizes}
    say("-- reference: bn254_fr_pow_batch_dev (254 squarings and 127 products per element) at n = %s: kernel ms %s" % (", ".join(str(n) for n in sizes), ", ".join("%.4f" % pow_ms[n] for n in sizes)))

    def table(title, count, nbytes, scopes, call, check=None, extra=None):
        say("-- %s: %d field products per record, %d bytes moved per record" % (title, count, nbytes))
        out = {}
        for n in sizes:
            v = repeat(lambda: kernel_ms(scopes, lambda: call(n)), a.repeats, a.warmup)
            if check:
                check(n)
            ms = out[n] = statistics.median(v)
            cp = statistics.median(copy_ms(nbytes * n))
            line = "n = %-7d | kernel ms %s | %9.3f M/s | fr_pow_batch_dev on n elements: %9.4f ms, the call takes %.2f x | a device copy of %d bytes: %8.4f ms" % (n, fmt(v), n / ms / 1e3, pow_ms[n], ms / pow_ms[n], nbytes * n, cp)
            say(line + (extra(n, ms) if extra else ""))
        return out

    def valid(st):
        def check(n):
            assert not st[:n].any().item(), "a valid record was rejected"
        return check

    try:
        for form in (0, 1):
            assert lib.bn254_fr_set_sqrt_form(form) == 0
            table("bn254_fr_sqrt_batch_dev, form %d%s" % (form, " (shipped)" if form == shipped else ""), SQRT[form], 68, ("fr_sqrt",),
                  lambda n: eng.fr_sqrt_batch_dev(X.data_ptr(), (O4 if form == 0 else O4b).data_ptr(), ST.data_ptr(), n, s0))
        assert torch.equal(O4, O4b), "the two forms of the square root differ"
    finally:
        assert lib.bn254_fr_set_sqrt_form(-1) == 0
    say("   the two forms gave equal bytes on the 2^%d elements; %d of them are squares" % (20 - sh, int(ST.count_nonzero().item())))
    table("bn254_bjj_pack_batch_dev", 0, 96, ("bjj_pack",), lambda n: eng.bjj_pack_batch_dev(A4.data_ptr(), O4.data_ptr(), n, s0))
    assert torch.equal(O4, A324), "pack(unpack) is not the identity"
    unpack = table("bn254_bjj_unpack_batch_dev (shipped form %d)" % shipped, UNPACK[shipped], 100, ("bjj_unpack",),
                   lambda n: eng.bjj_unpack_batch_dev(A324.data_ptr(), O8.data_ptr(), ST.data_ptr(), n, s0), valid(ST))
    assert torch.equal(O8, A4), "unpack(pack) is not the identity"
    plain = table("bn254_eddsa_poseidon_verify_batch_dev on the same signatures unpacked (W = %d)" % window, verify_products(window), 164, ("eddsa_poseidon_verify",),
                  lambda n: eng.eddsa_poseidon_verify_batch_dev(A4.data_ptr(), R84.data_ptr(), S4.data_ptr(), M4.data_ptr(), ST.data_ptr(), n, s0), valid(ST))
    table("bn254_eddsa_poseidon_verify_packed_batch_dev (one launch; W = %d, form %d)" % (window, shipped), verify_products(window) - 10 + 2 * UNPACK[shipped], 132, ("eddsa_poseidon_verify_packed",),
          lambda n: eng.eddsa_poseidon_verify_packed_batch_dev(A324.data_ptr(), SIG4.data_ptr(), M4.data_ptr(), ST2.data_ptr(), n, s0), valid(ST2),
          lambda n, ms: " | the unpacked verifier: %9.4f ms, the call takes %.2f x | 2 x unpack + the unpacked verifier: %9.4f ms, the call takes %.2f x"
          % (plain[n], ms / plain[n], 2 * unpack[n] + plain[n], ms / (2 * unpack[n] + plain[n])))

    say("-- the form of the square root: bn254_bjj_unpack_batch_dev over 2^%d valid packed points in each form (bn254_bjj_set_sqrt_form), interleaved, events on the stream" % (20 - sh))
    outs = (O8, O8b)
    sts = (ST, ST2)

    def one_run(form):
        assert lib.bn254_bjj_set_sqrt_form(form) == 0
        outs[form].fill_(0); sts[form].fill_(-1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        eng.bjj_unpack_batch_dev(A324.data_ptr(), outs[form].data_ptr(), sts[form].data_ptr(), n_big, s0)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    times = ([], [])
    try:
        for r in range(a.warmup + a.repeats):
            for form in (0, 1):
                ms = one_run(form)
                if r >= a.warmup:
                    times[form].append(ms)
    finally:
        assert lib.bn254_bjj_set_sqrt_form(-1) == 0
    assert torch.equal(O8, O8b) and torch.equal(O8, A4) and not ST.any().item() and not ST2.any().item(), "the two forms differ in their output"
    for form in (0, 1):
        say("form %d (%d products per point) | ms %s | %9.3f M points/s" % (form, UNPACK[form], fmt(times[form]), n_big / statistics.median(times[form]) / 1e3))
    m0, m1 = statistics.median(times[0]), statistics.median(times[1])
    say("the rule (fixed before measuring): the smaller median of the %d runs ships -> form %d (%.3f x the other); output bytes are equal; the library measured above carries form %d"
        % (a.repeats, 0 if m0 < m1 else 1, min(m0, m1) / max(m0, m1), shipped))
    say("   not built: Pedersen hash, packed key derivation (BLAKE-512), multi-GPU forms")


if __name__ == "__main__":
    main()
