// The per-lane bodies of the sparse linear maps over Fr (bn254_dot.hip): bn254_fr_dot_batch and its _dev twin,
//     out[j] = sum over t in [offsets[j], offsets[j+1]) of coeff[t] * x[index[t]].
// A lane owns one PIECE of the host's work list (io.hpp BnDotPiece, host_plan.hpp bn_dot_plan): at most P consecutive terms of one segment in
// the product level, at most F consecutive partial sums in a fold level - so the length of a lane's serial chain is a constant of the plan,
// never a property of the data.  Every product and every sum is canonical (fr.hpp), hence the result is the Python-integer sum whichever
// way the plan cuts a segment.  Everything is pure and takes plain pointers and a lane index, so the host simulation
// (tests/hostsim/hostsim_dot.cpp) runs the very same bodies over host arrays.
#pragma once
#include "fr_ops.hpp"
#include "io.hpp"

namespace bn254 {

// The shipped choices (plain constants; bn254_dot.hip carries a run-time override of the piece length for the sweep of tools/time_dot.py
// only).  Terms per lane of the product level: the fastest of the measured 4 / 8 / 16 / 32 on the R1CS-like shape (profiles/r15_dot.txt),
// which is the rule fixed before measuring - on ONE long segment 32 is a third faster.  Partial sums per lane of a fold level: not swept.
constexpr uint32_t FR_DOT_PIECE = 4;
constexpr uint32_t FR_DOT_FAN = 16;

// piece `lane` of the product level: sum of coeff[t] * x[index[t]] (index == NULL: x[t]) over its terms.  An index >= nx is outside the
// contract of the _dev entry point (the host-buffer one rejects it) but memory safe: it is compared BEFORE anything is loaded through it,
// and such a term contributes zero.
BN_FN void fr_dot_piece_body(const uint32_t *coeff, const uint64_t *index, const uint32_t *x, uint64_t nx, const BnDotPiece *list, uint32_t *part, uint32_t *out,
                             size_t lane) {
    const BnDotPiece pc = list[lane];
    const uint64_t first = dot_piece_first(pc);
    const uint32_t len = dot_piece_len(pc);
    Fr acc = fr_zero();
#pragma unroll 1
    for (uint32_t j = 0; j < len; ++j) {
        const uint64_t t = first + j, at = index ? index[t] : t;
        if (at < nx) acc = fr_add(acc, fr_mul(fr_load(x, at), fr_load(coeff, t)));
    }
    fr_store(acc, dot_piece_to_out(pc) ? out : part, pc.dst);
}
// piece `lane` of a fold level: sum of its partial sums (additions only).  A level reads slots only earlier levels wrote and writes slots
// of its own, so the lanes of one launch never meet.
BN_FN void fr_dot_fold_body(const BnDotPiece *list, uint32_t *part, uint32_t *out, size_t lane) {
    const BnDotPiece pc = list[lane];
    const uint64_t first = dot_piece_first(pc);
    const uint32_t len = dot_piece_len(pc);
    Fr acc = fr_zero();
#pragma unroll 1
    for (uint32_t j = 0; j < len; ++j) acc = fr_add(acc, fr_load(part, first + j));
    fr_store(acc, dot_piece_to_out(pc) ? out : part, pc.dst);
}

}  // namespace bn254
