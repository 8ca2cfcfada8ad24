"""The threading contract of include/bn254_hip.h, run for every family on an MI355X (run with -m gpu): the *_dev entry points on two streams
of ONE context - bytes under interleaving and the order the shared scratch imposes - and the host-buffer entry points from many threads.

ACTORS below holds one *_dev call per context-owned scratch buffer.  Its short form is the smallest shape that still uses the scratch (piece
lengths and fans from the library's hooks); its long form is the same call on the short inputs tiled `scale` times, issued `reps` times on
the one stream (the repetitions write into four output sets in turn).  Expected bytes: the integer models of tests/ for the Fr families, the oracle for
points and pairings; a tiled input has the tiled output (sumcheck: `scale` times the sums; the bucket sum: `scale` times the point), so every
byte of a long form is known as well.

Sizing (LONG below): each form alone, between two events on its stream after one warm-up call; the long form takes at least 5 ms and at
least ten times the short form of the actor behind it in the ring.  Kernel time on an MI355X, ms:

    actor                       short   long (scale, reps)    long   needed = max(5, 10 x the short form of the next)
    pairing_batch               1.023   (512, 8)            19.073   13.391
    pairing_product_batch       1.339   (64, 13)            20.935   15.746
    gt_pow                      1.575   (512, 7)            11.366    8.496
    g1_mul                      0.850   (512, 20)           16.530   11.050
    g1_msm_batch                1.105   (256, 14)           25.474   17.663
    g1_msm_bucket               1.766   (4096, 4)            8.306    5.000
    g1_mul_base_batch           0.192   (4096, 11)           7.456    5.000
    g1_normalize                0.130   (4096, 70)           8.021    5.380
    fr_inverse_batch            0.538   (4096, 16)           7.424    5.000
    fr_ntt_batch                0.041   (1024, 56)           6.996    5.000
    fr_dot_batch                0.042   (16384, 7)           6.609    5.000
    fr_scan_batch               0.265   (1024, 32)           9.279    6.494
    fr_sumcheck_round           0.649   (64, 24)            15.228   10.232

(medians of five and of three; the repetition counts leave a quarter and more above `needed`, because the short forms move by a tenth from
run to run.  g1_msm_bucket: one term, the smallest size of tests/test_gpu_msm_bucket.py at which every scope of the route runs; its long form
sums 4096 copies of the term.)  On that run the scratch-free control of the order test finished in front of the long call in 13 of 13 pairs.

Scratch buffers and the actor that covers each: ws and seg_plan with its pinned staging - pairing_product_batch_dev; exp_tbl -
pairing_batch_dev and pairing_product_batch_dev; pow_tbl - gt_pow_dev; mul_tbl - g1_mul_dev and g1_msm_batch_dev (with its term workspace and
work list in ws / seg_plan); msm_ws and msm_scal - g1_msm_dev on the bucket route; base_cache - g1_mul_base_batch_dev; norm_prefix -
g1_normalize_dev; fr_prefix - fr_inverse_batch_dev; ntt_tbl with its shift key and ntt_ws - fr_ntt_batch_dev; dot_ws (work list in seg_plan)
- fr_dot_batch_dev; scan_ws (work list in seg_plan) - fr_scan_batch_dev; mle_ws - fr_sumcheck_round_dev."""
import ctypes as C
import threading

import numpy as np
import pytest

import dot_cases as DC
import fr_cases as FC
import mle_cases as MC
import ntt_cases as NC
import scan_cases as SC
from conftest import canon_infinity

pytestmark = pytest.mark.gpu

R = FC.R
ACTORS = ["pairing_batch", "pairing_product_batch", "gt_pow", "g1_mul", "g1_msm_batch", "g1_msm_bucket", "g1_mul_base_batch", "g1_normalize",
          "fr_inverse_batch", "fr_ntt_batch", "fr_dot_batch", "fr_scan_batch", "fr_sumcheck_round"]
# the long form of every actor: (scale, reps), sized from the table in the module docstring
LONG = {
    "pairing_batch": (512, 8),
    "pairing_product_batch": (64, 13),
    "gt_pow": (512, 7),
    "g1_mul": (512, 20),
    "g1_msm_batch": (256, 14),
    "g1_msm_bucket": (4096, 4),
    "g1_mul_base_batch": (4096, 11),
    "g1_normalize": (4096, 70),
    "fr_inverse_batch": (4096, 16),
    "fr_ntt_batch": (1024, 56),
    "fr_dot_batch": (16384, 7),
    "fr_scan_batch": (1024, 32),
    "fr_sumcheck_round": (64, 24),
}
OUTPUT_SETS = 4                                        # the repetitions of a long form write into this many output sets in turn
MSM_SEGMENTS = [1, 5, 300]
PRODUCT_SEGMENTS = [2, 17]


def _load_lib():
    from bn_amd import _native
    l = _native.lib()
    for name in ("bn254_fr_dot_piece", "bn254_fr_dot_fan", "bn254_fr_scan_piece", "bn254_fr_scan_fan", "bn254_fr_sumcheck_piece", "bn254_fr_sumcheck_fan",
                 "bn254_ntt_tile_log"):
        getattr(l, name).argtypes = []; getattr(l, name).restype = C.c_uint
    return l


@pytest.fixture(scope="module")
def lib():
    return _load_lib()


@pytest.fixture(scope="module")
def eng():
    import bn_amd
    return bn_amd.Engine(0)


def _scalars(rng, n):
    return [int.from_bytes(rng.bytes(64), "little") % (R - 1) + 1 for _ in range(n)]


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _tiled_offsets(lens, scale):
    return _offsets(list(lens) * scale)


@pytest.fixture(scope="module")
def short(oracle, lib):
    """{actor: (inputs, expected outputs)} of the short forms as host arrays - computed once, never changed"""
    return _short_cases(oracle, lib)


def _short_cases(oracle, lib):
    rng = np.random.default_rng(4242)
    out = {}
    n_msm = sum(MSM_SEGMENTS)
    K = FC.rows(_scalars(rng, n_msm))
    P = oracle.g1_mul_batch_jacobian(np.tile(oracle.g1_one(), (n_msm, 1)), FC.rows(_scalars(rng, n_msm)))
    n_pairs = sum(PRODUCT_SEGMENTS)
    Q = oracle.g2_mul_batch_jacobian(np.tile(oracle.g2_one(), (n_pairs, 1)), FC.rows(_scalars(rng, n_pairs)))
    B = oracle.pairing_batch(P[:n_pairs], Q)
    out["pairing_batch"] = (dict(p=P[:8].copy(), q=Q[:8].copy()), dict(out=B[:8].copy()))
    folds = []
    for a, b in zip(_offsets(PRODUCT_SEGMENTS)[:-1], _offsets(PRODUCT_SEGMENTS)[1:]):
        acc = oracle.fq12_one()
        for i in range(int(a), int(b)):
            acc = oracle.fq12_mul(acc, B[i])
        folds.append(acc)
    out["pairing_product_batch"] = (dict(p=P[:n_pairs].copy(), q=Q.copy()), dict(out=np.stack(folds)))
    kp = K[:8].copy(); kp[0] = 0; kp[1] = FC.rows([1])[0]; kp[2] = FC.rows([R - 1])[0]
    out["gt_pow"] = (dict(a=B[:8].copy(), k=kp), dict(out=np.stack([oracle.gt_pow(B[i], kp[i]) for i in range(8)])))
    out["g1_mul"] = (dict(p=P[:70].copy(), k=K[:70].copy()), dict(out=oracle.g1_mul_batch(P[:70], K[:70])))
    terms = oracle.g1_mul_batch(P, K)
    sums = []
    for a, b in zip(_offsets(MSM_SEGMENTS)[:-1], _offsets(MSM_SEGMENTS)[1:]):
        acc = oracle.g1_zero()
        for t in terms[int(a):int(b)]:
            acc = oracle.g1_add(acc, t)
        sums.append(oracle.g1_normalize(acc))
    out["g1_msm_batch"] = (dict(p=P.copy(), k=K.copy()), dict(out=canon_infinity(np.stack(sums))))
    k1 = _scalars(rng, 1)[0]
    out["g1_msm_bucket"] = (dict(p=P[300:301].copy(), k=FC.rows([k1])), dict(k_int=k1))            # the sum of `scale` copies: (scale * k) P
    out["g1_mul_base_batch"] = (dict(base=P[7].copy(), k=K[100:170].copy()), dict(out=oracle.g1_mul_batch(np.tile(P[7], (70, 1)), K[100:170])))
    pn = P[200:270].copy(); pn[3] = oracle.g1_zero(); pn[69, 8:] = 0                               # two points at infinity, one with stale x, y
    out["g1_normalize"] = (dict(p=pn), dict(out=canon_infinity(np.stack([oracle.g1_normalize(p) for p in pn]))))
    inv = _scalars(rng, 70); inv[37] = 0; inv[5] = 1; inv[6] = R - 1
    rows, ok = FC.model_inverse(inv)
    out["fr_inverse_batch"] = (dict(a=FC.rows(inv)), dict(out=rows, ok=ok))
    log_n = int(lib.bn254_ntt_tile_log()) + 1
    vals = NC.batch(log_n, 1, seed=31)
    out["fr_ntt_batch"] = (dict(a=FC.rows(vals), log_n=log_n, shift=FC.rows([5])[0]), dict(out=FC.rows(NC.ntt(vals, False, 5))))
    L = 16 * int(lib.bn254_fr_dot_piece()) + 1
    coeff, xval = DC.terms(L, seed=32)
    out["fr_dot_batch"] = (dict(coeff=FC.rows(coeff), x=FC.rows(xval), L=L), dict(out=FC.rows(DC.model(coeff, xval, [0, L]))))
    L = int(lib.bn254_fr_scan_piece()) * int(lib.bn254_fr_scan_fan()) + 1
    a, b, init = SC.values(L, 33), SC.values(L, 34), [FC.rand(rng)]
    out["fr_scan_batch"] = (dict(a=FC.rows(a), b=FC.rows(b), init=FC.rows(init), L=L), dict(out=FC.rows(SC.model(a, b, [0, L], init))))
    h = int(lib.bn254_fr_sumcheck_piece()) * int(lib.bn254_fr_sumcheck_fan()) + 1
    name, k, degree, groups = MC.group_sets()[0]
    rws = MC.rows_of(2 * h, k, 35)
    out["fr_sumcheck_round"] = (dict(tables=MC.limbs(rws), h=h, k=k, degree=degree, groups=[(FC.rows([c])[0], m) for c, m in groups]),
                                dict(sums=MC.round_sums(rws, groups, degree)))
    return out


def _dev(arr):
    import torch
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr.view(np.int32 if arr.dtype == np.int32 else np.int64).copy()).to("cuda:0")


def _zeros(shape, dtype=None):
    import torch
    return torch.zeros(shape, dtype=dtype or torch.int64, device="cuda:0")


def _host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.int32 else a.view(np.uint64)


class Form:
    """one form of an actor on the device: its inputs (kept beside their host images), the output sets with the expected bytes, and
    issue(eng, stream) that enqueues the `reps` calls on the stream and returns without waiting"""

    def __init__(self, actor, oracle, short, scale=1, reps=1):
        self.actor, self.scale, self.reps = actor, scale, reps
        ins, want = short[actor]
        tile = lambda a: np.tile(a, (scale,) + (1,) * (a.ndim - 1))
        self.ins = {k: (_dev(tile(v)), tile(v)) for k, v in ins.items() if isinstance(v, np.ndarray) and k not in ("base", "shift", "groups", "tables")}
        self.host = ins
        self.want = {k: tile(v) for k, v in want.items() if isinstance(v, np.ndarray)}
        if actor == "g1_msm_bucket":
            point = oracle.g1_mul_batch(ins["p"], FC.rows([want["k_int"] * scale]))
            self.want = {"out": canon_infinity(point)}
        if actor == "fr_sumcheck_round":
            t, h = ins["tables"], ins["h"]
            tiled = np.concatenate([np.tile(t[:h], (scale, 1, 1)), np.tile(t[h:], (scale, 1, 1))])
            self.ins["tables"] = (_dev(tiled), tiled)
            self.want = {"out": FC.rows([v * scale for v in want["sums"]])}
        self.outs = [{k: _zeros(v.shape, _torch_dtype(v)) for k, v in self.want.items()} for _ in range(min(reps, OUTPUT_SETS))]

    def _call(self, eng, o, s):
        a, d, sc = self.actor, {k: v[0].data_ptr() for k, v in self.ins.items()}, self.scale
        out = o["out"].data_ptr()
        if a == "pairing_batch":
            eng.pairing_batch_dev(d["p"], d["q"], out, 8 * sc, s)
        elif a == "pairing_product_batch":
            eng.pairing_product_batch_dev(d["p"], d["q"], _tiled_offsets(PRODUCT_SEGMENTS, sc), out, s)
        elif a == "gt_pow":
            eng.gt_pow_dev(d["a"], d["k"], out, 8 * sc, s)
        elif a == "g1_mul":
            eng.g1_mul_dev(d["p"], d["k"], out, 70 * sc, s)
        elif a == "g1_msm_batch":
            eng.g1_msm_batch_dev(d["p"], d["k"], _tiled_offsets(MSM_SEGMENTS, sc), out, s)
        elif a == "g1_msm_bucket":
            eng.g1_msm_dev(d["p"], d["k"], sc, out, s)
        elif a == "g1_mul_base_batch":
            eng.g1_mul_base_batch_dev(self.host["base"], d["k"], out, 70 * sc, s)
        elif a == "g1_normalize":
            eng.g1_normalize_dev(d["p"], out, 70 * sc, s)
        elif a == "fr_inverse_batch":
            eng.fr_inverse_batch_dev(d["a"], out, o["ok"].data_ptr(), 70 * sc, s)
        elif a == "fr_ntt_batch":
            eng.fr_ntt_batch_dev(d["a"], out, self.host["log_n"], sc, False, self.host["shift"], s)
        elif a == "fr_dot_batch":
            eng.fr_dot_batch_dev(d["coeff"], None, d["x"], self.host["L"] * sc, _tiled_offsets([self.host["L"]], sc), sc, out, s)
        elif a == "fr_scan_batch":
            eng.fr_scan_batch_dev(d["a"], d["b"], d["init"], _tiled_offsets([self.host["L"]], sc), sc, out, stream=s)
        elif a == "fr_sumcheck_round":
            eng.fr_sumcheck_round_dev(d["tables"], 2 * self.host["h"] * sc, self.host["k"], self.host["groups"], out, self.host["degree"], s)
        else:
            raise KeyError(a)

    def issue(self, eng, stream):
        for r in range(self.reps):
            self._call(eng, self.outs[r % len(self.outs)], stream.cuda_stream)

    def clear(self):
        for o in self.outs:
            for t in o.values():
                t.zero_()

    def check(self, what):
        """every output of every repetition equals its expected bytes, every input is as it was"""
        for r, o in enumerate(self.outs):
            for k, t in o.items():
                got, want = _host(t).reshape(self.want[k].shape), self.want[k]
                assert got.tobytes() == want.tobytes(), (what, self.actor, self.scale, "output set %d, %d repetitions" % (r, self.reps), k,
                                                         np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0][:8])
        for k, (t, image) in self.ins.items():
            assert _host(t).tobytes() == image.tobytes(), (what, self.actor, "input", k)


def _torch_dtype(a):
    import torch
    return torch.int32 if a.dtype == np.int32 else torch.int64


def time_form(eng, form, stream):
    """milliseconds of one issue of the form alone on the stream, after one warm-up issue"""
    import torch
    form.issue(eng, stream); stream.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream); form.issue(eng, stream); b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def _fresh_engine():
    import bn_amd
    e = bn_amd.Engine(0)
    e.set_option("msm_bucket_min", 0)                  # g1_msm_dev takes the bucket route at every size (set before any concurrent use),
    e.set_option("msm_window_bits", 8)                 # with one window width: a call that changes the width waits for its stream
    return e


@pytest.fixture(scope="module")
def forms(oracle, short):
    """[{actor: (short form, long form)}] x 2 on the device, built once - a set per lap, so that no buffer has two writers that nothing
    orders; a test clears the outputs it is about to check"""
    return [{a: (Form(a, oracle, short), Form(a, oracle, short, *LONG[a])) for a in ACTORS} for _ in range(2)]


def _ring():
    return [(ACTORS[i], ACTORS[(i + 1) % len(ACTORS)]) for i in range(len(ACTORS))]


# ---- a. bytes under interleaving
def _growth_pairs(lib):
    """(family, lengths of the first call, lengths of the second), issued in this order on a context that starts with no scratch: the second
    call needs more than the first left.  Many one-piece segments need a long work list (seg_plan) and no partial sums (dot_ws) or maps
    (scan_ws); one long segment needs a short work list and many of those.  The sizes rise from pair to pair, because the buffers only grow"""
    out, many = [], 600
    for fam, P, F in (("dot", int(lib.bn254_fr_dot_piece()), int(lib.bn254_fr_dot_fan())), ("scan", int(lib.bn254_fr_scan_piece()), int(lib.bn254_fr_scan_fan()))):
        out += [(fam, [1] * many, [F * F * P + 1]), (fam, [2 * F * F * P + 1], [1] * (4 * many))]
        many *= 16
    return out


def _segmented_form(fam, lens, seed):
    """(issue(eng, stream), check(what)) of one dot or scan call over segments of these lengths, against the integer model"""
    n, m = sum(lens), len(lens)
    off = _offsets(lens)
    if fam == "dot":
        coeff, xval = DC.terms(n, seed)
        ins = [_dev(FC.rows(coeff)), _dev(FC.rows(xval))]
        images = [FC.rows(coeff), FC.rows(xval)]
        want = FC.rows(DC.model(coeff, xval, off))
        out = _zeros((m, 4))
        issue = lambda eng, s: eng.fr_dot_batch_dev(ins[0].data_ptr(), None, ins[1].data_ptr(), n, off, m, out.data_ptr(), s.cuda_stream)
    else:
        a, b = SC.values(n, seed), SC.values(n, seed + 1)
        ins = [_dev(FC.rows(a)), _dev(FC.rows(b))]
        images = [FC.rows(a), FC.rows(b)]
        want = FC.rows(SC.model(a, b, off))
        out = _zeros((n, 4))
        issue = lambda eng, s: eng.fr_scan_batch_dev(ins[0].data_ptr(), ins[1].data_ptr(), None, off, m, out.data_ptr(), stream=s.cuda_stream)

    def check(what):
        got = _host(out).reshape(want.shape)
        assert got.tobytes() == want.tobytes(), (what, fam, lens[:2], np.nonzero((got != want).any(axis=1))[0][:8])
        for t, image in zip(ins, images):
            assert _host(t).tobytes() == image.tobytes(), (what, fam, "input")
    return issue, check


def _ntt_pair_forms(short, count):
    """[(issue, check)] x 2: shift 5 forward, then shift 7 inverse, on `count` transforms - each call rebuilds the shift's table pair"""
    ins = short["fr_ntt_batch"][0]
    log_n = ins["log_n"]
    vals = NC.batch(log_n, 1, seed=31)
    image = np.tile(ins["a"], (count, 1))
    d_in = _dev(image)
    out = []
    for inverse, sh in ((False, 5), (True, 7)):
        want = np.tile(FC.rows(NC.ntt(vals, inverse, sh)), (count, 1))
        d_out = _zeros(want.shape)
        shift = FC.rows([sh])[0]
        issue = lambda eng, s, inverse=inverse, shift=shift, d_out=d_out: eng.fr_ntt_batch_dev(d_in.data_ptr(), d_out.data_ptr(), log_n, count, inverse, shift, s.cuda_stream)

        def check(what, want=want, d_out=d_out, sh=sh):
            got = _host(d_out).reshape(want.shape)
            assert got.tobytes() == want.tobytes(), (what, "ntt shift %d" % sh, np.nonzero((got != want).any(axis=1))[0][:8])
            assert _host(d_in).tobytes() == image.tobytes(), (what, "ntt input")
        out.append((issue, check))
    return out


def test_bytes_under_interleaving(oracle, lib, short, forms):
    """one fresh context, two streams, no synchronisation between the calls: the long form of every actor with the short form of the next
    behind it on the other stream, two laps with the streams swapped; four dot / scan pairs whose second call grows the scratch under the
    first; two NTT pairs whose calls alternate between two coset shifts.  Then every output, long and short, and every input is compared"""
    import torch
    e = _fresh_engine()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    growth = [(_segmented_form(fam, first, 50 + 2 * i), _segmented_form(fam, second, 70 + 2 * i)) for i, (fam, first, second) in enumerate(_growth_pairs(lib))]
    ntt = _ntt_pair_forms(short, 64) + _ntt_pair_forms(short, 1)
    for lap_forms in forms:
        for fs in lap_forms.values():
            for f in fs:
                f.clear()
    torch.cuda.synchronize()
    for (first, _), (second, _) in growth:             # first: the context has no scratch yet, and whatever these calls leave the ring outgrows
        first(e, s1); second(e, s2)
    for lap, (a, b) in enumerate(((s1, s2), (s2, s1))):
        for front, behind in _ring():
            forms[lap][front][1].issue(e, a)
            forms[lap][behind][0].issue(e, b)
        ntt[2 * lap][0](e, a); ntt[2 * lap + 1][0](e, b)
    torch.cuda.synchronize()
    for lap, lap_forms in enumerate(forms):
        for fs in lap_forms.values():
            for f in fs:
                f.check("ring, lap %d" % lap)
    for (_, c1), (_, c2) in growth:
        c1("growth, first call"); c2("growth, second call")
    for _, c in ntt:
        c("alternating shifts")
    e.close()


# ---- b. order
def test_a_call_on_the_second_stream_finishes_behind_the_call_that_holds_the_scratch(forms, short):
    """for every ring pair: e1 behind the long call on stream 1, e2 behind the short call on stream 2; once e2 has completed e1 must have,
    because the short call waited for the long call's scratch.  The control runs first: a scratch-free call (fr_mul_batch_dev on 64 elements)
    behind the same long calls MAY finish first, and unless it does so at least once the streams did not overlap and the order says nothing"""
    import torch
    e = _fresh_engine()
    forms = forms[0]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for fs in forms.values():                           # every buffer at its final size: no allocation (which waits for the device) below
        for f in fs:
            f.issue(e, s1)
    x = _dev(short["fr_inverse_batch"][0]["a"][:64]); y = _zeros((64, 4))
    e.fr_mul_batch_dev(x.data_ptr(), x.data_ptr(), y.data_ptr(), 64, s2.cuda_stream)
    torch.cuda.synchronize()
    overlapped = []
    for front in ACTORS:
        e1, e2 = torch.cuda.Event(), torch.cuda.Event()
        forms[front][1].issue(e, s1); e1.record(s1)
        e.fr_mul_batch_dev(x.data_ptr(), x.data_ptr(), y.data_ptr(), 64, s2.cuda_stream); e2.record(s2)
        e2.synchronize()
        if not e1.query():
            overlapped.append(front)
        torch.cuda.synchronize()
    print("control: the scratch-free call finished first behind %d of %d long calls: %s" % (len(overlapped), len(ACTORS), overlapped))
    if not overlapped:
        e.close()
        pytest.skip("the scratch-free control never finished in front of a long call: the two streams did not overlap in this process")
    late = []
    for front, behind in _ring():
        e1, e2 = torch.cuda.Event(), torch.cuda.Event()
        forms[front][1].issue(e, s1); e1.record(s1)
        forms[behind][0].issue(e, s2); e2.record(s2)
        e2.synchronize()
        if not e1.query():
            late.append((front, behind))
        torch.cuda.synchronize()
    e.close()
    assert not late, late


# ---- c. host threads
def _host_jobs(oracle, short, eng_of):
    """[(name, call() -> tuple of arrays, expected tuple)]: ten host-buffer calls, each with its short shape and one of a few thousand elements"""
    jobs = []

    def add(name, fn, want):
        jobs.append((name, fn, tuple(np.ascontiguousarray(w) for w in want)))
    ins, want = short["fr_ntt_batch"]
    vals = NC.batch(ins["log_n"], 1, seed=31)
    small = NC.batch(3, 5, seed=36)
    for sh in (5, 7):
        shift = FC.rows([sh])[0]
        add("fr_ntt_batch shift %d" % sh, lambda shift=shift: (eng_of().fr_ntt_batch(ins["a"], ins["log_n"], False, shift), eng_of().fr_ntt_batch(FC.rows(small), 3, True, shift)),
            (FC.rows(NC.ntt(vals, False, sh)), FC.rows(NC.ntt_batch(small, 3, True, sh))))
    d, dw = short["fr_dot_batch"]
    lens = [d["L"]] * 3 + [0, 7]
    coeff, xval = DC.terms(sum(lens), seed=37)
    add("fr_dot_batch", lambda: (eng_of().fr_dot_batch(d["coeff"], d["x"], [0, d["L"]]), eng_of().fr_dot_batch(FC.rows(coeff), FC.rows(xval), _offsets(lens))),
        (dw["out"], FC.rows(DC.model(coeff, xval, _offsets(lens)))))
    s, sw = short["fr_scan_batch"]
    lens2 = [s["L"]] * 3 + [0, 7]
    a, b = SC.values(sum(lens2), 38), SC.values(sum(lens2), 39)
    add("fr_scan_batch", lambda: (eng_of().fr_scan_batch(s["a"], s["b"], [0, s["L"]], s["init"]), eng_of().fr_scan_batch(FC.rows(a), FC.rows(b), _offsets(lens2))),
        (sw["out"], FC.rows(SC.model(a, b, _offsets(lens2)))))
    m, mw = short["fr_sumcheck_round"]
    t, h = m["tables"], m["h"]
    big = np.concatenate([np.tile(t[:h], (3, 1, 1)), np.tile(t[h:], (3, 1, 1))])
    add("fr_sumcheck_round", lambda: (eng_of().fr_sumcheck_round(t, m["groups"], m["degree"]), eng_of().fr_sumcheck_round(big, m["groups"], m["degree"])),
        (FC.rows(mw["sums"]), FC.rows([3 * v for v in mw["sums"]])))
    i, iw = short["fr_inverse_batch"]

    def inverse():
        r1, ok1 = eng_of().fr_inverse_batch(i["a"])
        r2, ok2 = eng_of().fr_inverse_batch(np.tile(i["a"], (50, 1)))
        return r1, ok1, r2, ok2
    add("fr_inverse_batch", inverse, (iw["out"], iw["ok"] != 0, np.tile(iw["out"], (50, 1)), np.tile(iw["ok"], 50) != 0))
    g, gw = short["g1_msm_batch"]
    add("g1_msm_batch", lambda: (eng_of().g1_msm_batch(g["p"], g["k"], _offsets(MSM_SEGMENTS)), eng_of().g1_msm_batch(np.tile(g["p"], (8, 1)), np.tile(g["k"], (8, 1)), _tiled_offsets(MSM_SEGMENTS, 8))),
        (gw["out"], np.tile(gw["out"], (8, 1))))
    p, pw = short["pairing_product_batch"]
    add("pairing_product_batch", lambda: (eng_of().pairing_product_batch(p["p"], p["q"], _offsets(PRODUCT_SEGMENTS)),
                                          eng_of().pairing_product_batch(np.tile(p["p"], (100, 1)), np.tile(p["q"], (100, 1)), _tiled_offsets(PRODUCT_SEGMENTS, 100))),
        (pw["out"], np.tile(pw["out"], (100, 1))))
    b8, bw = short["pairing_batch"]
    for j, tiles in enumerate((300, 500)):              # the slot-leasing path: no mutex, two callers side by side
        add("pairing_batch %d" % j, lambda tiles=tiles: (eng_of().pairing_batch(b8["p"], b8["q"]), eng_of().pairing_batch(np.tile(b8["p"], (tiles, 1)), np.tile(b8["q"], (tiles, 1)))),
            (bw["out"], np.tile(bw["out"], (tiles, 1))))
    return jobs


def _run_threads(jobs, iterations, timeout):
    errs = []
    start = threading.Barrier(len(jobs))

    def work(name, fn, want):
        try:
            start.wait(30)
            for it in range(iterations):
                got = fn()
                for j, (g, w) in enumerate(zip(got, want)):
                    if g.shape != w.shape or g.tobytes() != w.tobytes():
                        errs.append((name, "iteration %d" % it, "result %d differs" % j))
        except Exception as ex:                          # an error code of the library, a broken barrier
            errs.append((name, repr(ex)))
    th = [threading.Thread(target=work, args=job, daemon=True) for job in jobs]
    [t.start() for t in th]
    [t.join(timeout) for t in th]
    alive = [job[0] for job, t in zip(jobs, th) if t.is_alive()]
    assert not alive, ("still running", alive)
    assert not errs, errs


def test_ten_host_threads_on_one_context(oracle, short, eng):
    """eight threads in eight entry points that lock the context, two in bn254_pairing_batch, which leases a pipeline slot instead; four
    iterations each, every thread with inputs of its own; every result equals its expected bytes and no thread is left behind"""
    jobs = _host_jobs(oracle, short, lambda: eng)
    assert len(jobs) == 10
    _run_threads(jobs, 4, 120)


def test_three_fr_families_on_the_default_context(short, lib):
    """the C ABI with ctx == NULL - the process-wide default context the header's promise names - from three threads"""
    p = lambda a: C.c_void_p(a.ctypes.data)
    jobs = []
    ins, want = short["fr_ntt_batch"]
    a = np.ascontiguousarray(ins["a"]); shift = np.ascontiguousarray(ins["shift"])

    def ntt():
        out = np.zeros_like(a)
        assert lib.bn254_fr_ntt_batch(None, p(a), p(out), ins["log_n"], 1, 0, p(shift)) == 0
        return (out,)
    jobs.append(("fr_ntt_batch", ntt, (want["out"],)))
    d, dw = short["fr_dot_batch"]
    off = _offsets([d["L"]])

    def dot():
        out = np.zeros((1, 4), np.uint64)
        assert lib.bn254_fr_dot_batch(None, p(d["coeff"]), None, p(d["x"]), d["L"], p(off), 1, p(out)) == 0
        return (out,)
    jobs.append(("fr_dot_batch", dot, (dw["out"],)))
    s, sw = short["fr_scan_batch"]
    off2 = _offsets([s["L"]])

    def scan():
        out = np.zeros((s["L"], 4), np.uint64)
        assert lib.bn254_fr_scan_batch(None, p(s["a"]), p(s["b"]), p(s["init"]), p(off2), 1, 0, p(out)) == 0
        return (out,)
    jobs.append(("fr_scan_batch", scan, (sw["out"],)))
    _run_threads(jobs, 4, 120)
