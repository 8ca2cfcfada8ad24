"""bn_amd/csrc/fr_sqrt_constants.hpp is what tools/gen_fr_sqrt_constants.py writes, and what it holds is what the square root needs: c of order
exactly 2^28, the subgroup of order 16, the two tables of the digit-wise logarithm and the two plain integers.  No GPU."""
import pathlib
import re
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
HDR = ROOT / "bn_amd" / "csrc" / "fr_sqrt_constants.hpp"


def test_the_header_is_up_to_date():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_fr_sqrt_constants.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "up to date" in r.stdout, r.stdout + r.stderr
    stale = ROOT / "tests" / "hostsim" / "no_such_header.hpp"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_fr_sqrt_constants.py"), "--check", str(stale)], capture_output=True, text=True)
    assert r.returncode == 1 and "stale" in r.stdout and not stale.exists()


def _values(text):
    """{name: [integers]} of every array of the header, each element read back from its eight words"""
    out = {}
    for name, body in re.findall(r"BN254_CONSTANT uint32_t (\w+)(?:\[\d+\])+ = (.*?);\n", text, re.S):
        words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", body)]
        assert len(words) % 8 == 0
        out[name] = [sum(w << (32 * i) for i, w in enumerate(words[j:j + 8])) for j in range(0, len(words), 8)]
    return out


def test_the_constants_are_what_the_root_needs():
    import gen_fr_sqrt_constants as G
    R, T = G.R, G.T
    v = _values(HDR.read_text())
    unmont = lambda m: m * pow(1 << 256, -1, R) % R
    assert (R - 1) == T << 28 and T % 2 == 1
    c = unmont(v["C_M"][0])
    assert c == pow(5, T, R) and pow(c, 1 << 27, R) == R - 1                       # c^(2^27) == -1: the order is exactly 2^28
    assert v["EXP_RAW"] == [(T - 1) // 2] and v["HALF_RAW"] == [(R - 1) // 2]
    assert "EXP_BITS = %d;" % ((T - 1) // 2).bit_length() in HDR.read_text()
    root16 = [unmont(m) for m in v["ROOT16_M"]]
    assert root16 == [pow(c, k << 24, R) for k in range(16)] and len(set(root16)) == 16 and all(pow(x, 16, R) == 1 for x in root16)
    neg, half = [unmont(m) for m in v["NEG_M"]], [unmont(m) for m in v["NEG_HALF_M"]]
    assert len(neg) == len(half) == 7 * 16
    for j in range(7):
        for d in range(16):
            assert neg[16 * j + d] * pow(c, d << (4 * j), R) % R == 1
            if j or d % 2 == 0:
                assert half[16 * j + d] ** 2 % R == neg[16 * j + d]
    for m in sum(v.values(), []):
        assert m < R or m in v["EXP_RAW"] + v["HALF_RAW"]
