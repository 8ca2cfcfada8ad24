"""GPU parity of the Fq12 tower at edge elements (run with -m gpu on an MI355X): the three final-exponentiation kernels, Gt inverse,
the three Gt::pow chains, exp_by_neg_z and the product tree on the 64 edge elements of tests/edge_inputs.py (coefficients 0, q - 1, equal
ones, subfield elements, single slots) and their cyclotomic and order-r images.  The GPU leaves (v_mad_u64_u32 chains, DPP exchanges,
LDS staging) are what the CPU twins in tests/test_hostsim.py and tests/test_wave_machine.py replace.  Batches hold the list and its
rotation by one, so every element sits once on an even and once on an odd slot; odd n leave a ragged tail whose dead lanes re-read
element n - 1.  Every comparison is bit for bit against the oracle."""
import numpy as np
import pytest

import edge_inputs as E

pytestmark = pytest.mark.gpu

# final_exp_batch_dev: (name, options that force the route, the kernel that must run, the two that must not)
FE_ROUTES = (("wave", {"wave_fe_max": 1 << 20}, "final_exp_wave", ("final_exp_quad", "final_exp")),
             ("four-lane", {"wave_fe_max": 0, "quad_max": 1 << 20}, "final_exp_quad", ("final_exp_wave", "final_exp")),
             ("lane-pair", {"wave_fe_max": 0, "quad_max": 0}, "final_exp", ("final_exp_wave", "final_exp_quad")))


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


@pytest.fixture(scope="module")
def te(eng):
    import torch
    from bn_amd import distributed as D
    return D.TorchEngine(eng, torch.device("cuda", 0))


def _dev(te, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).to(te.device)      # a copy: the shared sets are read-only


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _twice(vals):
    """the list followed by its rotation by one: element i at slots i and 64 + (i - 1) % 64 - one even, one odd"""
    vals = list(vals)
    return np.stack(vals + vals[1:] + vals[:1])


def _bad(got, want, names):
    n = len(names)
    return [(i, names[i % n] if i < n else names[(i + 1) % n]) for i in range(got.shape[0]) if not np.array_equal(got[i], want[i])][:8]


@pytest.fixture(scope="module")
def sets(oracle):
    """the inputs and every oracle reference the tests share, computed once and never written to"""
    names = list(E.edge_fq12(oracle))
    edge, cyc, gt = _twice(E.edge_fq12(oracle).values()), _twice(E.edge_cyclotomic(oracle)), _twice(E.edge_gt(oracle))
    # alternate slots: every wave (32 consecutive lane pairs) holds elements of both kinds
    mix_cyc, mix_gt = edge.copy(), edge.copy()
    mix_cyc[0::2] = cyc[0::2]; mix_gt[0::2] = gt[0::2]
    ks = E.GT_EDGE_SCALARS + E.crafted_gls_by_sign()
    k = E.fr(oracle, [ks[i % len(ks)] for i in range(edge.shape[0])])
    s = {"names": names, "edge": edge, "cyc": cyc, "gt": gt, "mix_cyc": mix_cyc, "mix_gt": mix_gt, "k": k}
    for key in ("edge", "cyc", "gt", "mix_cyc", "mix_gt"):
        s["pow_" + key] = np.stack([oracle.gt_pow(a, ki) for a, ki in zip(s[key], k)])
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


@pytest.mark.parametrize("route", FE_ROUTES, ids=[r[0] for r in FE_ROUTES])
def test_final_exponentiation_kernels_on_edge_elements(oracle, eng, te, sets, route):
    """bn254_final_exp_batch_dev forced through the wave, the four-lane and the lane-pair kernel (the kernel statistics say which one
    ran): n = 1, 2, 3 (ragged quads and waves), 64 and 128, out of place and in place"""
    name, opts, kernel, others = route
    want = sets["gt"]                                    # FE(edge element), the same rotation
    eng.profile(True)
    try:
        with eng.options(**opts):
            for n in (1, 2, 3, 64, 128):
                eng.profile_reset()
                src = _dev(te, sets["edge"][:n])
                out = te.empty(n, 48)
                eng.final_exp_batch_dev(src.data_ptr(), out.data_ptr(), n, te._stream())
                got = _host(out)
                assert eng.kernel_stats(kernel)[1] >= 1 and all(eng.kernel_stats(o)[1] == 0 for o in others), (name, n)
                assert not _bad(got, want[:n], sets["names"]), (name, n, "out of place", _bad(got, want[:n], sets["names"]))
                assert np.array_equal(_host(src), sets["edge"][:n]), (name, n, "the input was written")
                eng.final_exp_batch_dev(src.data_ptr(), src.data_ptr(), n, te._stream())
                got = _host(src)
                assert not _bad(got, want[:n], sets["names"]), (name, n, "in place", _bad(got, want[:n], sets["names"]))
    finally:
        eng.profile(False)
    one = oracle.fq12_one()
    i = sets["names"].index("c0 only")
    assert np.array_equal(want[i], one) and np.array_equal(want[sets["names"].index("-1")], one)      # Fq6-subfield elements: FE = one


def test_gt_inverse_on_edge_elements(oracle, eng, sets):
    """bn254_gt_inverse_batch against fq12.rs:284-292, whole blocks and a ragged tail, and a * a^-1 == one through bn254_gt_mul_batch"""
    a = sets["edge"]
    want = np.stack([oracle.fq12_inverse(x) for x in a[:64]])
    want = np.concatenate([want, want[1:], want[:1]])
    for n in (128, 127, 1):
        inv = eng.gt_inverse_batch(a[:n])
        assert not _bad(inv, want[:n], sets["names"]), (n, _bad(inv, want[:n], sets["names"]))
    assert np.array_equal(eng.gt_mul_batch(a, eng.gt_inverse_batch(a)), np.tile(oracle.fq12_one(), (128, 1)))


def _pow_case(eng, sets, mode, key, n=128):
    eng.set_option("gt_pow_mode", mode)
    got = eng.gt_pow_batch(sets[key][:n], sets["k"][:n])
    bad = _bad(got, sets["pow_" + key][:n], sets["names"])
    assert not bad, (mode, key, n, bad)


def test_gt_pow_modes_on_edge_elements(oracle, eng, sets):
    """bn254_gt_pow_B, edge and crafted GLS scalars cycled over the elements.  Mode 1 (general chain) on the edge elements; mode 2
    (one-dimensional cyclotomic chain) on their cyclotomic images, whose order is generally not r; mode 0 (Frobenius decomposition) on
    their order-r images, `one` among them.  The choice of chain is per WAVE: in a batch that alternates such elements with plain edge
    elements every wave holds a non-cyclotomic one, takes the general chain as a whole and must still match"""
    names = sets["names"]
    for key in ("mix_cyc", "mix_gt"):                    # the mixes are what they are meant to be: no wave is all cyclotomic
        flags = [E.oracle_is_cyclotomic(oracle, a) for a in sets[key]]
        assert all(flags[0::2]) and all(not all(flags[w:w + 32]) for w in range(0, 128, 32)), key
    assert sum(np.array_equal(g, oracle.fq12_one()) for g in sets["gt"][:64]) >= 1 and names[0] == "one"
    try:
        _pow_case(eng, sets, 1, "edge"); _pow_case(eng, sets, 1, "edge", 127)
        _pow_case(eng, sets, 2, "cyc"); _pow_case(eng, sets, 2, "cyc", 127); _pow_case(eng, sets, 2, "mix_cyc")
        _pow_case(eng, sets, 0, "gt"); _pow_case(eng, sets, 0, "gt", 127); _pow_case(eng, sets, 0, "mix_gt")
    finally:
        eng.set_option("gt_pow_mode", None)


def test_exp_by_neg_z_on_edge_elements(oracle, te, sets):
    """bn254_exp_by_neg_z_dev (fq12.rs:229-246 as written, any Fq12 in) on the edge elements, whole blocks and a ragged tail"""
    want = np.stack([oracle.fq12_exp_by_neg_z(x) for x in sets["edge"][:64]])
    want = np.concatenate([want, want[1:], want[:1]])
    for n in (128, 127):
        a = _dev(te, sets["edge"][:n]); out = te.empty(n, 48)
        te.e.exp_by_neg_z_dev(a.data_ptr(), out.data_ptr(), n, te._stream())
        got = _host(out)
        assert not _bad(got, want[:n], sets["names"]), (n, _bad(got, want[:n], sets["names"]))


def test_product_tree_and_final_exp_tail_on_edge_elements(oracle, te, sets):
    """bn254_gt_product_dev and bn254_gt_product_final_exp_dev on the first n edge elements around every boundary of a wave of lane
    pairs, with the host's own tree shape and with one it would not pick (3 values per lane pair, 5 live lane pairs per wave, one
    butterfly level).  No element is zero, so no product is"""
    edge = sets["edge"]
    acc, fold, fe = oracle.fq12_one(), {}, {}
    for n in range(1, 65):
        acc = oracle.fq12_mul(acc, edge[n - 1])
        if n in (1, 2, 3, 31, 32, 33, 64):
            fold[n] = acc; fe[n] = oracle.fq12_final_exponentiation(acc)
    def check(tag):
        for n in fold:
            d = _dev(te, edge[:n])
            assert np.array_equal(_host(te.gt_product(d)), fold[n]), (tag, "product", n)
            assert np.array_equal(_host(te.product_final_exp(d)), fe[n]), (tag, "product + final exponentiation", n)
    check("default shape")
    with te.e.options(product_chunk=3, product_per_wave=5, product_bfly=1):
        check("chunk 3, 5 per wave, 1 butterfly level")
