#!/usr/bin/env python3
"""The Montgomery product leaves with every COLUMN's multiply-add chain as ONE inline-asm statement -> bn_amd/csrc/fe_asm.hpp
(what the GPU runs since the A/B of profiles/r03_ab_asm_leaf.txt: +3.6 % pairings/s; the host simulation
always uses the C++ leaves - same arithmetic, the asm only fixes the instruction ORDER).

What the compiler does with the C++ leaf (fe.hpp fe_mul2): 243 v_mad_u64_u32 + 9 v_mul_lo_u32 + 17 v_and + 16 v_lshrrev_b64 and 16
v_lshl_add_u64 - it splits each column sum into two chains (instruction-level parallelism) and joins them with a 64-bit add.  With
the chain of a column inside one asm statement the accumulator stays ONE serial chain (carry of the previous column -> 2(c+1)
products -> c reduction terms), the 16 adds disappear, and there are 17 asm statements per product (round 2 tried one statement
per INSTRUCTION: the compiler answered each with an s_nop, 234 per product, and lost 2 %; here it is 14).  Measured on one box,
libraries alternating: Miller 3.99 -> 3.82 ms, final exponentiation 3.565 -> 3.465 ms, 8.69 -> 9.00 M pairings/s; the Miller kernel
also drops from 3 spilled VGPRs to 0 (246 VGPRs).

DPP in hand-written or generated asm (none is emitted here - the lane exchanges are v_mov_b32_dpp around the chains, fq2.hpp): on gfx950 a lane
permutation attached to a REVERSED opcode lands on the other source (v_subrev_u32 + DPP16 computes dpp(S1) - S0, not S1 - dpp(S0):
profiles/r06_dpp_subrev_encoding.txt - the assembler encodes what the ISA says, the silicon swaps the operands before the permutation stage).
Safe forms: v_mov_b32_dpp; DPP on commutative VOP2 opcodes; DPP on the non-reversed v_sub_u32 with the permuted value as src0.  Never *rev + DPP.

usage: tools/gen_asm_leaf.py [--check] [path]       --check writes nothing: "up to date" and status 0, or "stale" and status 1
(tests/test_hostsim_leaf.py runs the check; tests/test_gpu_leaf.py runs every generated leaf against its C++ twin on the GPU)
"""
import pathlib
import sys

def chain(col, pairs, red, signed=False):
    """asm text + operand lists for one column: pairs = [(xname, yname)] product operand arrays (or "sqr": the squaring's 45 products
    against the doubled limbs a2[]), red = True adds m_i * Q_(col-i)"""
    lines, ins = [], []
    def op(expr, cons="v"):
        ins.append((cons, expr)); return "%%%d" % len(ins)          # %0 is the accumulator
    lo, hi = (0, col) if col < 9 else (col - 8, 8)
    for i in range(lo, hi + 1):
        if pairs == "sqr":
            j = col - i
            if i < j: lines.append("v_mad_u64_u32 %%0, vcc, %s, %s, %%0" % (op("a.l[%d]" % i), op("a2[%d]" % j)))
            elif i == j: lines.append("v_mad_u64_u32 %%0, vcc, %s, %s, %%0" % (op("a.l[%d]" % i), op("a.l[%d]" % i)))
            continue
        for (x, y) in pairs:
            lines.append("%s %%0, vcc, %s, %s, %%0" % ("v_mad_i64_i32" if signed else "v_mad_u64_u32", op("%s.l[%d]" % (x, i)), op("%s.l[%d]" % (y, col - i))))
    if red:
        rlo, rhi = (0, col - 1) if col < 9 else (col - 8, 8)
        for i in range(rlo, rhi + 1):
            lines.append("v_mad_u64_u32 %%0, vcc, %s, %s, %%0" % (op("m[%d]" % i), op("k::Q[%d]" % (col - i), "s")))
    return lines, ins

def func(name, args, pairs, signed=False):
    # column 0 starts its chain from the inline constant 0 (an early-clobber output: the statement reads its inputs after writing it)
    o = ["BN_FN Fe %s(%s) {" % (name, ", ".join("const Fe &%s" % a for a in args)),
         "    uint64_t acc;", "    uint32_t m[9];", "    Fe r;"]
    if pairs == "sqr":
        o.append("    uint32_t a2[9];")
        o.append("    for (int i = 0; i < 9; ++i) a2[i] = a.l[i] << 1;")
    for col in range(17):
        lines, ins = chain(col, pairs, True, signed)
        # the statement clobbers vcc (the carry-out operand of v_mad_u64_u32)
        if col == 0:
            lines[0] = lines[0][:lines[0].rindex("%0")] + "0"
            o.append('    asm("%s" : "=&v"(acc) : %s : "vcc");' % ("\\n\\t".join(lines), ", ".join('"%s"(%s)' % (c, e) for c, e in ins)))
        else:
            o.append('    asm("%s" : "+v"(acc) : %s : "vcc");' % ("\\n\\t".join(lines), ", ".join('"%s"(%s)' % (c, e) for c, e in ins)))
        shift = "acc = (uint64_t)((int64_t)acc >> 29);" if signed else "acc >>= 29;"
        if col < 9:
            o.append("    m[%d] = ((uint32_t)acc * k::QINV) & MASK29; acc += (uint64_t)m[%d] * k::Q[0]; %s" % (col, col, shift))
        else:
            o.append("    r.l[%d] = (uint32_t)acc & MASK29; %s" % (col - 9, shift))
    o += ["    r.l[8] = (uint32_t)acc;", "    return r;", "}"]
    return "\n".join(o)

def wide(name, signed=False):
    """the dual product WITHOUT reduction (fe.hpp fe_wmul2 / fe_wmul2s): 17 product columns, carry-propagated into 18 limbs"""
    o = ["BN_FN FeW %s(const Fe &a, const Fe &u, const Fe &c, const Fe &v) {" % name, "    uint64_t acc;", "    FeW r;"]
    for col in range(17):
        lines, ins = chain(col, [("a", "u"), ("c", "v")], False, signed)
        if col == 0:
            lines[0] = lines[0][:lines[0].rindex("%0")] + "0"
        o.append('    asm("%s" : "%s"(acc) : %s : "vcc");' % ("\\n\\t".join(lines), "=&v" if col == 0 else "+v", ", ".join('"%s"(%s)' % (c, e) for c, e in ins)))
        o.append("    r.l[%d] = (uint32_t)acc & MASK29; %s" % (col, "acc = (uint64_t)((int64_t)acc >> 29);" if signed else "acc >>= 29;"))
    o += ["    r.l[17] = (uint32_t)acc;", "    return r;", "}"]
    return "\n".join(o)

def wred(xi, sub):
    """the wide reduction (fe.hpp fe_wred): per column the terms of the linear combination, the Montgomery terms m_i q_(c-i) and - in the
    upper nine columns - the quotient estimate against the NEGATED modulus limb and the subtrahend, as one signed chain"""
    o = ["template <> BN_FN Fe fe_wred_asm<%s, %s>(const FeW &n, const FeW &x, const FeW &px, int32_t s, const Fe &d, int32_t kq) {" % ("true" if xi else "false", "true" if sub else "false"),
         "    uint64_t acc;", "    uint32_t m[9];", "    Fe r;"]
    for col in range(18):
        lines, ins = [], []
        def op(expr, cons="v"):
            ins.append((cons, expr)); return "%%%d" % len(ins)
        lines.append("%s %%0, vcc, 1, %s, %%0" % ("v_mad_u64_u32" if col < 17 else "v_mad_i64_i32", op("n.l[%d]" % col)))
        if xi:
            lines.append("v_mad_i64_i32 %%0, vcc, 9, %s, %%0" % op("x.l[%d]" % col))
            lines.append("v_mad_i64_i32 %%0, vcc, %s, %s, %%0" % (op("s"), op("px.l[%d]" % col)))
        rlo, rhi = (0, col - 1) if col < 9 else (col - 8, 8)
        for i in range(rlo, rhi + 1):
            lines.append("v_mad_u64_u32 %%0, vcc, %s, %s, %%0" % (op("m[%d]" % i), op("k::Q[%d]" % (col - i), "s")))
        if col >= 9:
            lines.append("v_mad_i64_i32 %%0, vcc, %s, %s, %%0" % (op("kq"), op("-(int32_t)k::Q[%d]" % (col - 9), "s")))
            if sub:
                lines.append("v_mad_i64_i32 %%0, vcc, -1, %s, %%0" % op("d.l[%d]" % (col - 9)))
        if col == 0:
            lines[0] = lines[0][:lines[0].rindex("%0")] + "0"
        o.append('    asm("%s" : "%s"(acc) : %s : "vcc");' % ("\\n\\t".join(lines), "=&v" if col == 0 else "+v", ", ".join('"%s"(%s)' % (c, e) for c, e in ins)))
        shift = "acc = (uint64_t)((int64_t)acc >> 29);"
        if col < 9:
            o.append("    m[%d] = ((uint32_t)acc * k::QINV) & MASK29; acc += (uint64_t)m[%d] * k::Q[0]; %s" % (col, col, shift))
        elif col < 17:
            o.append("    r.l[%d] = (uint32_t)acc & MASK29; %s" % (col - 9, shift))
        else:
            o.append("    r.l[8] = (uint32_t)acc;")
    o += ["    return r;", "}"]
    return "\n".join(o)

text = "\n".join(["// GENERATED by tools/gen_asm_leaf.py - do not edit.  The GPU forms of the multiplier leaves of fe.hpp (fe_mul_body, fe_sqr_body, fe_mul2, fe_mul2s, fe_mul6, fe_mul5) and of its double-width leaves (fe_wmul2, fe_wmul2s, fe_wred): one asm statement per column.", "#pragma once", "namespace bn254 {",
                  func("fe_mul_asm", ["a", "b"], [("a", "b")]), func("fe_mul2_asm", ["a", "u", "c", "v"], [("a", "u"), ("c", "v")]), func("fe_sqr_asm", ["a"], "sqr"),
                  # the dual product over SIGNED limbs (|limb| < 2^29: differences of standard elements, tower.hpp's Karatsuba cross products): the products
                  # through v_mad_i64_i32, the column carries by arithmetic shifts; the result is a signed lazy value (its top limb carries the sign)
                  func("fe_mul2s_asm", ["a", "u", "c", "v"], [("a", "u"), ("c", "v")], signed=True),
                  # six products under one reduction (the lazily reduced sparse line product of tower.hpp): 63 column terms - every operand limb below 2^29
                  func("fe_mul6_asm", ["a1", "u1", "c1", "v1", "a2", "u2", "c2", "v2", "a3", "u3", "c3", "v3"],
                       [("a1", "u1"), ("c1", "v1"), ("a2", "u2"), ("c2", "v2"), ("a3", "u3"), ("c3", "v3")]),
                  # five products under one reduction: two Fq2 products and one product of the lane's own component by an Fq scalar (the native
                  # prepared line product of tower.hpp f12_mul_by_line_native)
                  func("fe_mul5_asm", ["a1", "u1", "c1", "v1", "a2", "u2", "c2", "v2", "a3", "u3"],
                       [("a1", "u1"), ("c1", "v1"), ("a2", "u2"), ("c2", "v2"), ("a3", "u3")]),
                  # the lazily reduced Karatsuba products of the lane-pair tower (tower.hpp f6_mul_lazy): dual products that stay unreduced at
                  # double width, and the ONE Montgomery reduction per Fq6 coefficient that takes their linear combination
                  wide("fe_wmul2_asm"), wide("fe_wmul2s_asm", signed=True),
                  "template <bool XI, bool SUB> BN_FN Fe fe_wred_asm(const FeW &n, const FeW &x, const FeW &px, int32_t s, const Fe &d, int32_t kq);",
                  wred(False, False), wred(False, True), wred(True, False), wred(True, True), "}  // namespace bn254", ""])
if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    p = pathlib.Path(args[0]) if args else pathlib.Path(__file__).resolve().parents[1] / "bn_amd" / "csrc" / "fe_asm.hpp"
    if p.exists() and p.read_text() == text:
        print("up to date:", p)
    elif "--check" in sys.argv[1:]:
        print("stale:", p)
        sys.exit(1)
    else:
        p.write_text(text); print("wrote", p)
