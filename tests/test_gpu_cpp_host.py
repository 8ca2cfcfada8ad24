"""include/bn254.hpp executed on an MI355X (run with -m gpu): ONE host program, compiled with g++ against the header and run once as a child
process, calls every wrapper that the other tests only find by searching the header's text - the multi-scalar multiplications, fixed-base
multiplication, normalize and eq with the operators built on them, the Fr batch operations, the transforms, dot, scan and the multilinear
calls - on eight to forty elements per call, and dumps the words it gets.  The inputs are literal limbs printed into the program by this
module; the expected words come from the integer models of tests/ (Fr) and from the oracle (points).

The program first calls every wrapper that throws std::invalid_argument with one mismatching argument, before anything has touched a device,
and reports whether the process holds the GPU driver's device node open at its start, behind those calls and behind its first real call: the
throwing calls must leave it closed, and the first real call must open it (which shows that the probe can see a device call)."""
import pathlib
import subprocess

import numpy as np
import pytest

import dot_cases as DC
import edge_inputs as E
import fr_cases as FC
import mle_cases as MC
import ntt_cases as NC
import scan_cases as SC
from conftest import canon_infinity

pytestmark = pytest.mark.gpu

R = FC.R
ROOT = pathlib.Path(__file__).resolve().parents[1]
N_G1, N_G2 = 12, 8
G1_SEGMENTS, G2_SEGMENTS = [0, 0, 1, 5, 12], [0, 3, 3, 8]
DOT_OFFSETS, SCAN_OFFSETS = [0, 0, 3, 20], [0, 0, 7, 20]
ROOT_LOGS = [0, 1, 3, 28]

PROGRAM = r'''
#include "bn254.hpp"
#include <cstdio>
#include <dirent.h>
#include <unistd.h>
using namespace bn;
@LITERALS@
template <class T> std::vector<T> load(const uint64_t *w, size_t n) { std::vector<T> v(n); if (n) std::memcpy(static_cast<void *>(v.data()), w, n * sizeof(T)); return v; }
template <class T> void dump(const char *label, const std::vector<T> &v) {
    std::printf("%s", label);
    const uint64_t *w = reinterpret_cast<const uint64_t *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T) / 8; ++i) std::printf(" %llu", (unsigned long long)w[i]);
    std::printf("\n");
}
template <class T> void dump1(const char *label, const T &t) { dump(label, std::vector<T>(1, t)); }
void dump(const char *label, const std::vector<bool> &v) { std::printf("%s", label); for (bool b : v) std::printf(" %d", b ? 1 : 0); std::printf("\n"); }
// 1 when this process holds the GPU driver's device node open: the HIP runtime opens it with the first call that needs a device
static int device_node_open() {
    int found = 0;
    if (DIR *d = opendir("/proc/self/fd")) {
        while (dirent *e = readdir(d)) {
            char path[300], target[300];
            std::snprintf(path, sizeof path, "/proc/self/fd/%s", e->d_name);
            const ssize_t n = readlink(path, target, sizeof target - 1);
            if (n > 0) { target[n] = 0; if (std::strcmp(target, "/dev/kfd") == 0) found = 1; }
        }
        closedir(d);
    }
    return found;
}
template <class Fn> void must_throw(const char *name, Fn fn) {
    int r = 0;
    try { fn(); } catch (const std::invalid_argument &) { r = 1; } catch (const std::exception &) { r = 2; }
    std::printf("throws %s %d\n", name, r);
}
int main() {
    std::printf("device_node at_start %d\n", device_node_open());
    const std::vector<Fr> a = load<Fr>(FR_A, 24), b = load<Fr>(FR_B, 24), short_fr(a.begin(), a.begin() + 23);
    const std::vector<G1> p = load<G1>(G1_P, 12), short_p(p.begin(), p.begin() + 11);
    const std::vector<G2> q = load<G2>(G2_Q, 8), short_q(q.begin(), q.begin() + 7);
    const std::vector<Fr> k12(a.begin(), a.begin() + 12), k8(b.begin(), b.begin() + 8);
    const std::vector<size_t> off_g1 = {@G1_SEGMENTS@}, off_g2 = {@G2_SEGMENTS@}, off_dot = {@DOT_OFFSETS@}, off_scan = {@SCAN_OFFSETS@};
    const std::vector<Fr> c20(a.begin(), a.begin() + 20), x20(b.begin(), b.begin() + 20), x9(b.begin() + 10, b.begin() + 19), seg3(a.begin() + 20, a.begin() + 23);
    const std::vector<uint64_t> index = {@DOT_INDEX@};
    // ---- every wrapper that throws, with one argument that does not fit, before anything has touched a device
    must_throw("pairing_batch", [&] { pairing_batch(short_p, q); });
    must_throw("pairing_product", [&] { pairing_product(p, short_q); });
    must_throw("pairing_product_batch:lengths", [&] { pairing_product_batch(short_p, q, {0, 8}); });
    must_throw("pairing_product_batch:offsets", [&] { pairing_product_batch(std::vector<G1>(p.begin(), p.begin() + 8), q, {0, 7}); });
    must_throw("pairing_check_batch", [&] { pairing_check_batch(std::vector<G1>(p.begin(), p.begin() + 8), q, {}); });
    must_throw("g1_msm_batch:lengths", [&] { g1_msm_batch(p, short_fr, off_g1); });
    must_throw("g1_msm_batch:offsets", [&] { g1_msm_batch(p, k12, off_g2); });
    must_throw("g2_msm_batch:lengths", [&] { g2_msm_batch(short_q, k8, off_g2); });
    must_throw("g2_msm_batch:offsets", [&] { g2_msm_batch(q, k8, {}); });
    must_throw("g1_msm", [&] { g1_msm(short_p, k12); });
    must_throw("g2_msm", [&] { g2_msm(q, k12); });
    must_throw("g1_eq", [&] { g1_eq(p, short_p); });
    must_throw("g2_eq", [&] { g2_eq(short_q, q); });
    must_throw("fr_add", [&] { fr_add(a, short_fr); });
    must_throw("fr_sub", [&] { fr_sub(short_fr, b); });
    must_throw("fr_mul", [&] { fr_mul(a, short_fr); });
    must_throw("fr_pow", [&] { fr_pow(short_fr, b); });
    must_throw("fr_ntt:length", [&] { fr_ntt(a, 4); });                                              // 24 elements are not whole transforms of 16
    must_throw("fr_ntt:log_n", [&] { fr_ntt(a, BN254_NTT_LOG_MAX + 1); });
    must_throw("fr_ntt:negative", [&] { fr_ntt(a, -1); });
    must_throw("fr_dot:offsets", [&] { fr_dot(c20, &index, x9, {0, 19}); });
    must_throw("fr_dot:index", [&] { std::vector<uint64_t> i19(index.begin(), index.begin() + 19); fr_dot(c20, &i19, x9, off_dot); });
    must_throw("fr_dot:x", [&] { fr_dot(c20, nullptr, x9, off_dot); });
    must_throw("fr_scan:neither", [&] { fr_scan(nullptr, nullptr, &seg3, off_scan); });
    must_throw("fr_scan:a", [&] { fr_scan(&x9, &x20, &seg3, off_scan); });
    must_throw("fr_scan:a_per_segment", [&] { fr_scan(&c20, &x20, &seg3, off_scan, BN254_SCAN_A_PER_SEGMENT); });
    must_throw("fr_scan:b", [&] { fr_scan(&c20, &x9, &seg3, off_scan); });
    must_throw("fr_scan:init", [&] { fr_scan(&c20, &x20, &x9, off_scan); });
    must_throw("fr_scan:offsets", [&] { fr_scan(&c20, &x20, nullptr, {}); });
    must_throw("fr_mle_eq", [&] { fr_mle_eq(std::vector<Fr>(BN254_MLE_VARS_MAX + 1, Fr::one())); });
    must_throw("fr_mle_fold", [&] { fr_mle_fold(short_fr, Fr::one()); });
    must_throw("fr_sumcheck_round:k", [&] { fr_sumcheck_round(a, 0, {0, 1}, {0}, {Fr::one()}, 1); });
    must_throw("fr_sumcheck_round:tables", [&] { fr_sumcheck_round(short_fr, 3, {0, 1}, {0}, {Fr::one()}, 1); });
    must_throw("fr_sumcheck_round:coeff", [&] { fr_sumcheck_round(a, 3, {0, 1}, {0}, {}, 1); });
    must_throw("fr_sumcheck_round:members", [&] { fr_sumcheck_round(a, 3, {0, 2}, {0}, {Fr::one()}, 2); });
    must_throw("fr_sumcheck_round:degree", [&] { fr_sumcheck_round(a, 3, {0, 1}, {0}, {Fr::one()}, 0); });
    std::printf("device_node after_throws %d\n", device_node_open());
    // ---- the scalar field
    dump("fr_add", fr_add(a, b));
    std::printf("device_node after_first_call %d\n", device_node_open());
    dump("fr_sub", fr_sub(a, b));
    dump("fr_mul", fr_mul(a, b));
    dump("fr_pow", fr_pow(load<Fr>(POW_A, 16), load<Fr>(POW_E, 16)));
    { auto r = fr_inverse(load<Fr>(INV_A, 16)); dump("fr_inverse", r.first); dump("fr_inverse_ok", r.second); }
    { std::vector<std::array<uint8_t, 64>> bufs(8); std::memcpy(bufs.data(), INTERPRET, sizeof INTERPRET); dump("fr_interpret", fr_interpret(bufs)); }
    { std::vector<Fr> roots; for (int log_n : {@ROOT_LOGS@}) roots.push_back(fr_root_of_unity(log_n)); dump("fr_root_of_unity", roots); }
    const std::vector<Fr> v16(a.begin(), a.begin() + 16);
    const Fr shift = b[23];
    dump("fr_ntt forward", fr_ntt(v16, 3));
    dump("fr_ntt inverse", fr_ntt(v16, 3, true));
    dump("fr_ntt forward shift", fr_ntt(v16, 3, false, &shift));
    dump("fr_ntt inverse shift", fr_ntt(v16, 3, true, &shift));
    dump("fr_dot index", fr_dot(c20, &index, x9, off_dot));
    dump("fr_dot nullptr", fr_dot(c20, nullptr, x20, off_dot));
    dump("fr_scan no a", fr_scan(nullptr, &x20, &seg3, off_scan));
    dump("fr_scan no b", fr_scan(&c20, nullptr, &seg3, off_scan));
    dump("fr_scan no init", fr_scan(&c20, &x20, nullptr, off_scan));
    dump("fr_scan reverse", fr_scan(&c20, &x20, &seg3, off_scan, BN254_SCAN_REVERSE));
    dump("fr_scan exclusive", fr_scan(&c20, &x20, &seg3, off_scan, BN254_SCAN_EXCLUSIVE));
    { const std::vector<Fr> per(b.begin() + 20, b.begin() + 23); dump("fr_scan a_per_segment", fr_scan(&per, &x20, &seg3, off_scan, BN254_SCAN_A_PER_SEGMENT)); }
    dump("fr_mle_eq four", fr_mle_eq(std::vector<Fr>(b.begin(), b.begin() + 4)));
    dump("fr_mle_eq none", fr_mle_eq({}));
    dump("fr_mle_fold", fr_mle_fold(v16, shift));
    dump("fr_sumcheck_round", fr_sumcheck_round(a, 3, {0, 3, 4}, {0, 1, 2, 1}, {b[20], b[21]}, 3));
    // ---- the groups
    dump("g1_msm_batch", g1_msm_batch(p, k12, off_g1));
    dump("g2_msm_batch", g2_msm_batch(q, k8, off_g2));
    dump1("g1_msm", g1_msm(p, k12));
    dump1("g2_msm", g2_msm(q, k8));
    dump("g1_mul_base", g1_mul_base(p[1], k12));
    dump("g2_mul_base", g2_mul_base(q[1], k8));
    dump("g1_normalize", g1_normalize(p));
    dump("g2_normalize", g2_normalize(q));
    { std::vector<G1> inplace = {p[0], p[3], p[11]}; for (auto &g : inplace) g.normalize(); dump("G1::normalize", inplace); }
    { std::vector<G2> inplace = {q[0], q[2], q[7]}; for (auto &g : inplace) g.normalize(); dump("G2::normalize", inplace); }
    dump("g1_eq", g1_eq(p, load<G1>(G1_OTHER, 12)));
    dump("g2_eq", g2_eq(q, load<G2>(G2_OTHER, 8)));
    { const std::vector<G1> o = load<G1>(G1_OTHER, 12); dump("G1 operators", std::vector<bool>{p[0] == o[0], p[1] == o[1], p[0] != o[0], p[1] != o[1], p[3] == G1::zero()}); }
    { const std::vector<G2> o = load<G2>(G2_OTHER, 8); dump("G2 operators", std::vector<bool>{q[0] == o[0], q[1] == o[1], q[0] != o[0], q[1] != o[1], q[2] == G2::zero()}); }
    std::printf("done\n");
    return 0;
}
'''


def _literal(name, arr):
    words = np.ascontiguousarray(arr).view(np.uint64).reshape(-1)
    return "static const uint64_t %s[] = {%s};" % (name, ", ".join("0x%xull" % int(w) for w in words))


def _draws(rng, n):
    return [FC.rand(rng) for _ in range(n)]


@pytest.fixture(scope="module")
def inputs(oracle):
    """everything the program is given, as integers / host arrays - computed once, never changed"""
    rng = np.random.default_rng(777)
    a, b = FC.pairs(24, seed=5)
    a[8], b[9] = 0, 0                                                            # a zero scalar among the first twelve and the first eight
    P = oracle.g1_mul_batch_jacobian(np.tile(oracle.g1_one(), (N_G1, 1)), FC.rows(_draws(rng, N_G1)))
    Q = oracle.g2_mul_batch_jacobian(np.tile(oracle.g2_one(), (N_G2, 1)), FC.rows(_draws(rng, N_G2)))
    P[3] = oracle.g1_zero(); P[11, 8:] = 0                                       # infinity as G1::zero() and with stale x, y
    Q[2] = oracle.g2_zero(); Q[7, 16:] = 0
    # the other side of eq: even i - another representation of the same element; odd i - another element; both at infinity; one at infinity
    PO = np.stack([E.rescale_g1(oracle, P[i], E.FQ_Z[1 + i % 7]) if i % 2 == 0 else P[(i + 2) % N_G1] for i in range(N_G1)])
    QO = np.stack([E.rescale_g2(oracle, Q[i], E.FQ2_Z[i]) if i % 2 == 0 else Q[(i + 2) % N_G2] for i in range(N_G2)])
    PO[3], PO[11] = P[11], P[0]
    pow_a, pow_e = FC.pow_cases(16, seed=6)
    inv = FC.inverse_values(16, 8, 2, seed=7)
    buf, ints = FC.interpret_buffers(8, seed=8)
    index = [int(i) for i in rng.integers(0, 9, 20)]
    return dict(a=a, b=b, P=P, Q=Q, PO=PO, QO=QO, pow_a=pow_a, pow_e=pow_e, inv=inv, buf=buf, ints=ints, index=index)


@pytest.fixture(scope="module")
def ran(inputs, tmp_path_factory):
    """{label: words} of the program's one run, and its lines"""
    i = inputs
    lits = [_literal("FR_A", FC.rows(i["a"])), _literal("FR_B", FC.rows(i["b"])), _literal("G1_P", i["P"]), _literal("G2_Q", i["Q"]),
            _literal("G1_OTHER", i["PO"]), _literal("G2_OTHER", i["QO"]), _literal("POW_A", FC.rows(i["pow_a"])), _literal("POW_E", FC.rows(i["pow_e"])),
            _literal("INV_A", FC.rows(i["inv"])),
            "static const uint8_t INTERPRET[] = {%s};" % ", ".join(str(int(v)) for v in i["buf"].reshape(-1))]
    src = PROGRAM.replace("@LITERALS@", "\n".join(lits))
    for key, val in (("G1_SEGMENTS", G1_SEGMENTS), ("G2_SEGMENTS", G2_SEGMENTS), ("DOT_OFFSETS", DOT_OFFSETS), ("SCAN_OFFSETS", SCAN_OFFSETS),
                     ("DOT_INDEX", i["index"]), ("ROOT_LOGS", ROOT_LOGS)):
        src = src.replace("@%s@" % key, ", ".join(str(v) for v in val))
    tmp = tmp_path_factory.mktemp("cpp_host")
    (tmp / "host.cpp").write_text(src)
    exe = tmp / "host"
    subprocess.check_call(["g++", "-std=c++17", "-I", str(ROOT / "include"), str(tmp / "host.cpp"), "-o", str(exe),
                           "-L", str(ROOT / "bn_amd"), "-lbn254_hip", "-Wl,-rpath," + str(ROOT / "bn_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lines = subprocess.check_output([str(exe)], timeout=300).decode().strip().split("\n")
    assert lines[-1] == "done", lines[-3:]
    out = {}
    for line in lines:
        label = " ".join(w for w in line.split() if not w.isdigit())
        out[label] = np.array([int(w) for w in line.split() if w.isdigit()], np.uint64)
    return out, lines


def _same(ran, label, want):
    got = ran[0][label]
    want = np.ascontiguousarray(want).astype(np.uint64).reshape(-1)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (label, np.nonzero(got != want)[0][:8])


def test_every_throwing_wrapper_throws_before_any_device_call(ran):
    out, lines = ran
    throws = [l.split() for l in lines if l.startswith("throws ")]
    assert len(throws) == 36 and len({t[1] for t in throws}) == 36
    assert [t for t in throws if t[2] != "1"] == []                              # 1: std::invalid_argument; 0: nothing; 2: another exception
    first_dump = next(n for n, l in enumerate(lines) if l.startswith("fr_add"))
    assert all(n < first_dump for n, l in enumerate(lines) if l.startswith("throws "))
    state = {l.split()[1]: int(l.split()[2]) for l in lines if l.startswith("device_node ")}
    assert state == {"at_start": 0, "after_throws": 0, "after_first_call": 1}, state


def test_fr_arithmetic(ran, inputs):
    a, b = inputs["a"], inputs["b"]
    _same(ran, "fr_add", FC.rows([(x + y) % R for x, y in zip(a, b)]))
    _same(ran, "fr_sub", FC.rows([(x - y) % R for x, y in zip(a, b)]))
    _same(ran, "fr_mul", FC.rows([x * y % R for x, y in zip(a, b)]))
    _same(ran, "fr_pow", FC.rows([pow(x, e, R) for x, e in zip(inputs["pow_a"], inputs["pow_e"])]))
    rows, ok = FC.model_inverse(inputs["inv"])
    assert 0 in inputs["inv"] and 0 < ok.sum() < len(ok)
    _same(ran, "fr_inverse", rows)
    _same(ran, "fr_inverse_ok", ok)                                              # int32_t -> bool -> 0 / 1
    _same(ran, "fr_interpret", FC.rows([v % R for v in inputs["ints"]]))
    _same(ran, "fr_root_of_unity", FC.rows([NC.root(l) for l in ROOT_LOGS]))


def test_fr_ntt(ran, inputs):
    v, s = inputs["a"][:16], inputs["b"][23]
    assert s not in (0, 1)
    _same(ran, "fr_ntt forward", FC.rows(NC.ntt_batch(v, 3)))
    _same(ran, "fr_ntt inverse", FC.rows(NC.ntt_batch(v, 3, True)))
    _same(ran, "fr_ntt forward shift", FC.rows(NC.ntt_batch(v, 3, False, s)))
    _same(ran, "fr_ntt inverse shift", FC.rows(NC.ntt_batch(v, 3, True, s)))


def test_fr_dot_and_scan(ran, inputs):
    a, b = inputs["a"], inputs["b"]
    c20, x20, x9, seg3, per = a[:20], b[:20], b[10:19], a[20:23], b[20:23]
    _same(ran, "fr_dot index", FC.rows(DC.model(c20, x9, DOT_OFFSETS, inputs["index"])))
    _same(ran, "fr_dot nullptr", FC.rows(DC.model(c20, x20, DOT_OFFSETS)))
    _same(ran, "fr_scan no a", FC.rows(SC.model(None, x20, SCAN_OFFSETS, seg3)))
    _same(ran, "fr_scan no b", FC.rows(SC.model(c20, None, SCAN_OFFSETS, seg3)))
    _same(ran, "fr_scan no init", FC.rows(SC.model(c20, x20, SCAN_OFFSETS)))
    _same(ran, "fr_scan reverse", FC.rows(SC.model(c20, x20, SCAN_OFFSETS, seg3, reverse=True)))
    _same(ran, "fr_scan exclusive", FC.rows(SC.model(c20, x20, SCAN_OFFSETS, seg3, exclusive=True)))
    _same(ran, "fr_scan a_per_segment", FC.rows(SC.model(per, x20, SCAN_OFFSETS, seg3, a_per_segment=True)))


def test_multilinear_wrappers(ran, inputs):
    a, b = inputs["a"], inputs["b"]
    _same(ran, "fr_mle_eq four", FC.rows(MC.eq_table(b[:4])))
    _same(ran, "fr_mle_eq none", FC.rows([1]))
    _same(ran, "fr_mle_fold", FC.rows(MC.fold(a[:16], b[23])))
    rows = [a[3 * i:3 * i + 3] for i in range(8)]                                # tables[i * k + j]: eight indices of three tables
    _same(ran, "fr_sumcheck_round", FC.rows(MC.round_sums(rows, [(b[20], [0, 1, 2]), (b[21], [1])], 3)))


def _sum(oracle, g, terms):
    add, norm, zero = (oracle.g1_add, oracle.g1_normalize, oracle.g1_zero()) if g == 1 else (oracle.g2_add, oracle.g2_normalize, oracle.g2_zero())
    acc = zero
    for t in terms:
        acc = add(acc, t)
    return canon_infinity(norm(acc)[None])[0]


def test_group_wrappers(ran, inputs, oracle):
    a, b, P, Q = inputs["a"], inputs["b"], inputs["P"], inputs["Q"]
    k12, k8 = FC.rows(a[:12]), FC.rows(b[:8])
    t1, t2 = oracle.g1_mul_batch(P, k12), oracle.g2_mul_batch(Q, k8)
    _same(ran, "g1_msm_batch", np.stack([_sum(oracle, 1, t1[lo:hi]) for lo, hi in zip(G1_SEGMENTS, G1_SEGMENTS[1:])]))
    _same(ran, "g2_msm_batch", np.stack([_sum(oracle, 2, t2[lo:hi]) for lo, hi in zip(G2_SEGMENTS, G2_SEGMENTS[1:])]))
    _same(ran, "g1_msm", _sum(oracle, 1, t1))
    _same(ran, "g2_msm", _sum(oracle, 2, t2))
    _same(ran, "g1_mul_base", canon_infinity(oracle.g1_mul_batch(np.tile(P[1], (12, 1)), k12)))
    _same(ran, "g2_mul_base", canon_infinity(oracle.g2_mul_batch(np.tile(Q[1], (8, 1)), k8)))
    n1 = canon_infinity(np.stack([oracle.g1_normalize(p) for p in P]))
    n2 = canon_infinity(np.stack([oracle.g2_normalize(q) for q in Q]))
    _same(ran, "g1_normalize", n1)
    _same(ran, "g2_normalize", n2)
    _same(ran, "G1::normalize", n1[[0, 3, 11]])
    _same(ran, "G2::normalize", n2[[0, 2, 7]])
    e1 = [oracle.g1_eq(x, y) for x, y in zip(P, inputs["PO"])]
    e2 = [oracle.g2_eq(x, y) for x, y in zip(Q, inputs["QO"])]
    assert e1 == [i % 2 == 0 or i == 3 for i in range(N_G1)] and e2 == [i % 2 == 0 for i in range(N_G2)]          # 3: infinity on both sides
    _same(ran, "g1_eq", e1)
    _same(ran, "g2_eq", e2)
    _same(ran, "G1 operators", [e1[0], e1[1], not e1[0], not e1[1], True])
    _same(ran, "G2 operators", [e2[0], e2[1], not e2[0], not e2[1], True])
