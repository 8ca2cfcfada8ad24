"""The integer model of tests/bjj_pack_cases.py against itself - roots square back and are the smaller ones, packing and unpacking are inverse to
each other - and the host-integer twins of the package (bn_amd.babyjub.sqrt_host / pack_host / unpack_host, bn_amd.eddsa.pack_signature /
unpack_signature / verify_packed_status_host) against the model.  No GPU."""
import babyjub_cases as BC
import bjj_pack_cases as PK

R = PK.R


def test_model_roots_square_back_and_are_the_smaller_ones():
    vals = PK.sqrt_values()
    kinds = set()
    for v in vals:
        x = PK.sqrt(v)
        kinds.add(x is None)
        if x is None:
            assert pow(v, (R - 1) // 2, R) == R - 1
        else:
            assert x * x % R == v % R and 0 <= x <= PK.HALF
    assert kinds == {True, False}
    assert PK.sqrt(PK.HALF * PK.HALF % R) == PK.HALF and PK.sqrt(0) == 0 and PK.sqrt(1) == 1 and PK.sqrt(4) == 2 and PK.sqrt(5) is None
    assert pow(PK.C28, 1 << 27, R) == R - 1
    for k in range(28):                                                            # c^(2^k) has the exact order 2^(28 - k)
        v = pow(PK.C28, 1 << k, R)
        assert pow(v, 1 << (28 - k), R) == 1 and pow(v, 1 << (27 - k), R) != 1
    assert PK.sqrt(PK.C28) is None and PK.sqrt(pow(PK.C28, 2, R)) in (PK.C28, R - PK.C28)


def test_model_pack_and_unpack_are_inverse():
    recs = PK.unpack_records()
    for b, p, st in recs:
        assert len(b) == 32
        if st == 0:
            assert BC.on_curve(p) and PK.pack(p) == b and PK.unpack(PK.pack(p)) == (p, 0)
        else:
            assert p == BC.O
    for _, p in BC.edge_points():
        assert PK.unpack(PK.pack(p)) == (p, 0)
    assert {st for _, _, st in recs} == {0, 1, 3, 4}
    assert PK.unpack(b"\xff" * 32)[1] == 1 and PK.unpack(PK.pack(BC.O)) == (BC.O, 0) and PK.pack(BC.O) == (1).to_bytes(32, "little")


def test_host_twins_of_the_package_agree_with_the_model():
    from bn_amd import babyjub as BJ, eddsa
    for v in PK.sqrt_values():
        assert BJ.sqrt_host(v) == PK.sqrt(v)
    for b, p, st in PK.unpack_records():
        assert BJ.unpack_host(b) == (p, st)
        if st == 0:
            assert BJ.pack_host(p) == b and BJ.pack_host(BJ.Point(*p)) == b
    assert set(BJ.PACK_STATUS) == {0, 1, 3, 4, 6}
    for name, a32, sig64, m, st in PK.packed_signature_rows():
        if m < R:                                                                   # a message is an Fr or an integer mod r in the package
            assert eddsa.verify_packed_status_host(a32, m, sig64) == st, name
    assert eddsa.pack_signature((BC.KAT_R8, BC.KAT_S)) == PK.pack_signature(BC.KAT_R8, BC.KAT_S)
    assert eddsa.unpack_signature(PK.pack_signature(BC.KAT_R8, BC.KAT_S)) == ((BC.KAT_R8, BC.KAT_S), 0)
    assert eddsa.verify_packed_status_host(PK.pack(BC.KAT_A), BC.KAT_M, PK.pack_signature(BC.KAT_R8, BC.KAT_S)) == 0
