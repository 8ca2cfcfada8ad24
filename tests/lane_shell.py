"""TEST INFRASTRUCTURE - what "the kernels of this unit are instances of bn254_fr_decode_k" means in the sources (the one shell is
bn_amd/csrc/lane_launch.hpp's), for the tests/test_*_abi.py files of the families of integer kernels."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parents[1] / "bn_amd" / "csrc"
HEADER = "lane_launch.hpp"


def shell_definitions():
    """the files of csrc/ that define a kernel bn254_fr_decode_k templated on its Op"""
    return [p.name for p in sorted(CSRC.iterdir()) if p.suffix in (".hip", ".hpp") and re.search(r"__global__[^\n]*?bn254_fr_decode_k\(Op\b", p.read_text())]


def unit_source(unit, own_kernels=False):
    """The text of csrc/<unit> after the checks: the one Op-templated shell of csrc/ is the header's, with the block size as a template
    argument; the unit includes the header; and - unless it keeps plain kernels of its own (bn254_wire.hip) - it defines no kernel at all,
    so every kernel it launches is an instance of that name."""
    assert shell_definitions() == [HEADER]
    assert re.search(r"template <unsigned B, class Op>\s*__global__ void __launch_bounds__\(B\) bn254_fr_decode_k\(Op op\)", (CSRC / HEADER).read_text())
    src = (CSRC / unit).read_text()
    assert f'#include "{HEADER}"' in src
    if not own_kernels:
        assert "__global__" not in src
    return src
