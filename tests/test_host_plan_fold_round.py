"""host_plan.hpp bn_sumcheck_fold_piece, the indices per lane of the fused fold-then-round kernel, without a GPU: the pure function through
tests/hostsim/hostsim_fold_round.cpp against its model, on both sides of every threshold, and the library's own choice with and without
the override of bn254_fr_sumcheck_fold_set_piece."""
import ctypes as C

import pytest

import fold_round_cases as FR
import hostsim_fold_round_lib as HF


def test_fill_is_two_waves_on_every_simd():
    sim = HF.lib()
    assert sim.hfr_fill(256) == 256 * 4 * 64 * 2 == 131072 and sim.hfr_fill(1) == 512


@pytest.mark.parametrize("fill", [2, 20, 512, 131072])
def test_the_piece_on_both_sides_of_every_threshold(fill):
    """from P = 16: the lanes fill the machine from (fill - 1) * P + 1 indices on, below that P is halved, and 4 is the floor"""
    sim = HF.lib()
    piece = lambda h2, P=16: int(sim.hfr_piece(h2, P, fill))
    assert [piece(fill * 16), piece(fill * 16 - 15), piece(fill * 16 - 16)] == [16, 16, 8]
    assert [piece(fill * 8), piece(fill * 8 - 7), piece(fill * 8 - 8)] == [8, 8, 4]
    assert [piece(fill * 4), piece(fill * 4 - 3), piece(fill * 4 - 4), piece(1)] == [4, 4, 4, 4]                  # the floor
    assert [piece(fill * 8, 8), piece(fill * 8 - 8, 8), piece(1, 4), piece(1 << 30, 4)] == [8, 4, 4, 4]            # another shipped piece
    for h2 in (1, 2, 3, fill, 3 * fill + 1, 4 * fill, 5 * fill, 8 * fill - 8, 8 * fill - 7, 8 * fill, 12 * fill, 16 * fill - 16, 16 * fill - 15, 16 * fill, 1 << 30):
        for P in (4, 8, 16):
            assert piece(h2, P) == FR.fold_piece(h2, P, fill), (h2, P)
            assert piece(h2, P) == 4 or -(-h2 // piece(h2, P)) >= fill       # a piece above the floor always fills


def test_the_library_takes_the_adaptive_piece_and_an_override_wins():
    from bn_amd import _native
    lib = _native.lib()
    lib.bn254_fr_sumcheck_fold_piece.argtypes = []; lib.bn254_fr_sumcheck_fold_piece.restype = C.c_uint
    lib.bn254_fr_sumcheck_fold_set_piece.argtypes = [C.c_uint]
    lib.bn254_fr_sumcheck_fold_piece_for.argtypes = [C.c_size_t, C.c_size_t]; lib.bn254_fr_sumcheck_fold_piece_for.restype = C.c_uint
    P = lib.bn254_fr_sumcheck_fold_piece()
    assert P == HF.lib().hfr_shipped_piece() and P in (4, 8, 16)
    sizes = (1, 4097, 131072 * 4, 131072 * 8 - 8, 131072 * 8, 131072 * 16 - 16, 131072 * 16, 1 << 28)
    for h2 in sizes:
        assert lib.bn254_fr_sumcheck_fold_piece_for(h2, 256) == FR.fold_piece(h2, P, 131072)
    assert lib.bn254_fr_sumcheck_fold_piece_for(4097, 256) == 4 and lib.bn254_fr_sumcheck_fold_piece_for(1 << 28, 256) == P
    try:
        assert lib.bn254_fr_sumcheck_fold_set_piece(65) == -2
        for forced in (4, 8, 16, 64):
            assert lib.bn254_fr_sumcheck_fold_set_piece(forced) == 0
            assert [lib.bn254_fr_sumcheck_fold_piece_for(h2, 256) for h2 in sizes] == [forced] * len(sizes)       # at every size
    finally:
        assert lib.bn254_fr_sumcheck_fold_set_piece(0) == 0
    assert lib.bn254_fr_sumcheck_fold_piece_for(4097, 256) == 4 and lib.bn254_fr_sumcheck_fold_piece() == P
