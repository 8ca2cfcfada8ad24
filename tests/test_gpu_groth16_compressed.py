"""groth16.verify_batch_compressed on an MI355X (run with -m gpu): a block of eight proofs travels as 128-byte compressed proofs in both layouts;
a flipped sign bit, an x without a point and a B outside the subgroup must each fail their proof and nothing else."""
import numpy as np
import pytest

import compress_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def block():
    from bn_amd import Fr
    from test_gpu_msm import _groth16_setup
    rng = np.random.default_rng(880)
    vk, prove = _groth16_setup(rng, 2)
    inputs = [[Fr.random(rng) for _ in range(2)] for _ in range(8)]
    return vk, prove(inputs), inputs


@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("fmt", sorted(CC.FORMATS))
def test_compressed_block(block, fmt, prepared):
    from bn_amd import groth16
    vk, proofs, inputs = block
    f = CC.FORMATS[fmt]
    blob = groth16.encode_proofs(proofs, fmt)
    assert len(blob) == 8 * 128
    back, status = groth16.decode_proofs(blob, fmt)
    assert status.shape == (8, 3) and not status.any() and all(x == y for p, q in zip(proofs, back) for x, y in zip(p, q))
    plain = groth16.verify_batch(vk, proofs, inputs, prepared=prepared)
    assert plain.all()
    assert np.array_equal(groth16.verify_batch_compressed(vk, blob, inputs, fmt, prepared=prepared), plain)
    bad = bytearray(blob)
    sign_at = (lambda lo: lo + 31) if fmt == "ark" else (lambda lo: lo)           # the byte of a 32-byte G1 record that holds the flags
    bad[sign_at(1 * 128)] ^= 0x80 if fmt == "ark" else 0x40                      # proof 1: A is -A
    bad[3 * 128:3 * 128 + 32] = CC.render(1, [CC.x_without_point(1)[0]], "sign0", f)             # proof 3: A.x has no point
    bad[6 * 128 + 32:6 * 128 + 96] = CC.render(2, list(CC.g2_outside_subgroup()[0]), "sign1", f)  # proof 6: B is outside the subgroup
    _, status = groth16.decode_proofs(bytes(bad), fmt)
    assert status.tolist() == [[0, 0, 0]] * 3 + [[4, 0, 0]] + [[0, 0, 0]] * 2 + [[0, 5, 0]] + [[0, 0, 0]]
    got = groth16.verify_batch_compressed(vk, bytes(bad), inputs, fmt, prepared=prepared)
    assert got.dtype == bool and got.tolist() == [True, False, True, False, True, True, False, True]
