"""Batch engine over the C ABI.  Arrays are numpy uint64 in the reference's #[repr(C)] layouts:
   Fr (n,4)  G1 (n,12)  G2 (n,24)  Gt (n,48)   - Montgomery limbs, little endian."""
import ctypes as C

import numpy as np

from . import _native

FR_BYTES, G1_WORDS, G2_WORDS, GT_WORDS = 32, 12, 24, 48


def _arr(a, width):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"expected shape (n,{width}) uint64, got {a.shape}")
    return a


def _p(a):
    return C.c_void_p(a.ctypes.data)


COMPRESSED_FORMATS = {"ark": 0, "gnark": 1}          # BN254_COMPRESSED_* of include/bn254_hip.h
G1_COMPRESSED_BYTES, G2_COMPRESSED_BYTES = 32, 64


def compressed_format(fmt):
    """"ark" / "gnark" -> the header's number (numbers pass through: the library rejects the unknown ones)"""
    if isinstance(fmt, str):
        if fmt not in COMPRESSED_FORMATS:
            raise ValueError(f"unknown compressed format {fmt!r}: {sorted(COMPRESSED_FORMATS)} are defined")
        return COMPRESSED_FORMATS[fmt]
    return int(fmt)


H2C_FIELD_BYTES, H2C_UNIFORM_BYTES, H2C_DST_MAX = 48, 96, 255       # BN254_H2C_* of include/bn254_hip.h
H2C_G2_FIELD_BYTES, H2C_G2_UNIFORM_BYTES = 96, 192                  # BN254_H2C_G2_*


def h2c_dst(dst):
    """the domain separation tag as bytes, 1 .. 255 of them (the RFC's rule for hashing longer tags is not built)"""
    dst = bytes(dst)
    if not 0 < len(dst) <= H2C_DST_MAX:
        raise ValueError(f"a domain separation tag has 1 .. {H2C_DST_MAX} bytes, got {len(dst)}")
    return dst


def _same_len(a, b):
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"operands differ in length: {a.shape[0]} vs {b.shape[0]}")


def _ntt_count(rows, log_n):
    """transforms in an array of `rows` elements"""
    if not 0 <= log_n <= 24:
        raise ValueError(f"log_n must be 0..24, got {log_n}")
    if rows % (1 << log_n):
        raise ValueError(f"{rows} elements are not whole transforms of 2^{log_n}")
    return rows >> log_n


def _group_ntt_count(rows, log_n):
    """transforms over G1 / G2 in an array of `rows` points"""
    if not 0 <= log_n <= 22:
        raise ValueError(f"log_n must be 0..22, got {log_n}")
    if rows % (1 << log_n):
        raise ValueError(f"{rows} points are not whole transforms of 2^{log_n}")
    return rows >> log_n


def _ntt_shift(shift):
    """the coset shift as one C-contiguous scalar of 4 uint64 words, or None (NULL).  The CALLER keeps the returned array alive for the length
    of the C call and takes its address there: a converted copy (a list, another dtype, a strided view) belongs to nobody else"""
    if shift is None:
        return None
    shift = np.ascontiguousarray(shift, dtype=np.uint64).reshape(-1)
    if shift.size != 4:
        raise ValueError(f"shift must be ONE scalar of 4 uint64 words, got {shift.size}")
    return shift


def _offsets(offsets):
    """CSR segment offsets as a C-contiguous size_t array (the C ABI checks their order and start)"""
    o = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if o.size == 0:
        raise ValueError("offsets needs m + 1 >= 1 entries")
    return o


def _dot_args(coeff, x, offsets, index):
    """the operands of fr_dot_batch, checked the way the C ABI checks them (it answers BN254_E_BAD_ARG; here the caller learns which one):
    (coeff, x, offsets, index or None) as C-contiguous arrays"""
    coeff = _arr(coeff, 4) if len(coeff) else np.zeros((0, 4), np.uint64)
    x = _arr(x, 4) if len(x) else np.zeros((0, 4), np.uint64)
    o = _offsets(offsets)
    n, nx = coeff.shape[0], x.shape[0]
    if int(o[0]) != 0 or (o.size > 1 and bool((o[1:] < o[:-1]).any())):
        raise ValueError("offsets must start at 0 and never decrease")
    if int(o[-1]) != n:
        raise ValueError(f"offsets[m] = {int(o[-1])} but {n} terms were given")
    if index is None:
        if nx != n:
            raise ValueError(f"without an index the terms meet x one to one: {n} terms vs {nx} elements of x")
        return coeff, x, o, None
    index = np.asarray(index)
    if index.ndim != 1 or index.shape[0] != n:
        raise ValueError(f"index holds {index.shape} entries but {n} terms were given")
    if n and (index.dtype.kind not in "iu" or int(index.min()) < 0 or int(index.max()) >= nx):
        raise ValueError(f"an index is out of range: x holds {nx} elements")
    return coeff, x, o, np.ascontiguousarray(index, dtype=np.uint64)


SCAN_REVERSE, SCAN_EXCLUSIVE, SCAN_A_PER_SEGMENT = 1, 2, 4           # BN254_SCAN_* of include/bn254_hip.h


def _scan_flags(reverse, exclusive, a_per_segment):
    return (SCAN_REVERSE if reverse else 0) | (SCAN_EXCLUSIVE if exclusive else 0) | (SCAN_A_PER_SEGMENT if a_per_segment else 0)


def _scan_args(a, b, offsets, init, a_per_segment):
    """the operands of fr_scan_batch, checked the way the C ABI checks them (it answers BN254_E_BAD_ARG; here the caller learns which one):
    (a or None, b or None, offsets, init or None) as C-contiguous arrays"""
    if a is None and b is None:
        raise ValueError("a and b are both None: the recurrence out[t] = a[t] * prev + b[t] needs one of them")
    rows = lambda v: None if v is None else (_arr(v, 4) if len(v) else np.zeros((0, 4), np.uint64))
    a, b, init = rows(a), rows(b), rows(init)
    o = _offsets(offsets)
    if int(o[0]) != 0 or (o.size > 1 and bool((o[1:] < o[:-1]).any())):
        raise ValueError("offsets must start at 0 and never decrease")
    m, n = o.size - 1, int(o[-1])
    if b is not None and b.shape[0] != n:
        raise ValueError(f"b holds {b.shape[0]} terms but offsets[m] = {n}")
    if a is not None and a.shape[0] != (m if a_per_segment else n):
        raise ValueError(f"a holds {a.shape[0]} records but " + (f"a_per_segment takes one for each of the {m} segments" if a_per_segment else f"offsets[m] = {n}"))
    if init is not None and init.shape[0] != m:
        raise ValueError(f"init holds {init.shape[0]} values but there are {m} segments")
    return a, b, o, init


MLE_VARS_MAX, SUMCHECK_DEGREE_MAX, SUMCHECK_TABLES_MAX, SUMCHECK_GROUPS_MAX = 30, 4, 16, 16       # BN254_MLE_* / BN254_SUMCHECK_* of include/bn254_hip.h


POSEIDON_ARITY_MAX, MERKLE_LOG_MAX = 4, 24                  # BN254_POSEIDON_ARITY_MAX / BN254_MERKLE_LOG_MAX of include/bn254_hip.h


def _poseidon_args(x, name, lo, hi, what):
    """rows of records as a C-contiguous (n, width, 4) array, lo <= width <= hi"""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    if x.ndim == 2 and x.shape[1] == 4:                            # one record per row
        x = x.reshape(x.shape[0], 1, 4)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError(f"{name} must have shape (n, {what}, 4) uint64, got {x.shape}")
    if not lo <= x.shape[1] <= hi:
        raise ValueError(f"{name} holds {x.shape[1]} records per row, {what} = {lo}..{hi} are supported")
    return x


def _merkle_args(leaves):
    """(leaves as a C-contiguous (n, 4) array, log2 n)"""
    x = _arr(leaves, 4) if len(leaves) else np.zeros((0, 4), np.uint64)
    n = x.shape[0]
    if n == 0 or n & (n - 1):
        raise ValueError(f"leaves holds {n} records: a tree needs a power of two, one at least")
    if n > 1 << MERKLE_LOG_MAX:
        raise ValueError(f"leaves holds {n} records, at most 2^{MERKLE_LOG_MAX} are supported")
    return x, n.bit_length() - 1


POSEIDON_EX_INPUTS_MAX = 16                                 # BN254_POSEIDON_EX_INPUTS_MAX of include/bn254_hip.h


def _poseidon_ex_args(x, init, n_outs, name="x"):
    """the operands of fr_poseidon_ex_batch, checked the way the C ABI checks them: (x as (n, n_inputs, 4), init as (n, 4) or None)"""
    x = _poseidon_args(x, name, 1, POSEIDON_EX_INPUTS_MAX, "n_inputs")
    if not 1 <= n_outs <= x.shape[1] + 1:
        raise ValueError(f"n_outs = {n_outs}: 1..{x.shape[1] + 1} for {x.shape[1]} inputs per row")
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.uint64).reshape(-1, 4)
        if init.shape[0] == 1 and x.shape[0] != 1:                 # one initial state for every row
            init = np.ascontiguousarray(np.broadcast_to(init, (x.shape[0], 4)))
        if init.shape[0] != x.shape[0]:
            raise ValueError(f"init holds {init.shape[0]} records but x has {x.shape[0]} rows")
    return x, init


def _poseidon_chain_args(x, offsets, rate):
    """the operands of fr_poseidon_chain_batch: (x as (n, 4), offsets as size_t words)"""
    if not 1 <= rate <= POSEIDON_EX_INPUTS_MAX:
        raise ValueError(f"rate = {rate}: 1..{POSEIDON_EX_INPUTS_MAX} are supported")
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
    o = _offsets(offsets)
    if int(o[0]) != 0 or (o.size > 1 and bool((o[1:] < o[:-1]).any())):
        raise ValueError("offsets must start at 0 and never decrease")
    if int(o[-1]) != x.shape[0]:
        raise ValueError(f"x holds {x.shape[0]} records but offsets[m] = {int(o[-1])}")
    return x, o


def _fr_point(v, name):
    """one field element (anything with .limbs, or four uint64 words) as a C-contiguous array of 4 words"""
    v = np.ascontiguousarray(getattr(v, "limbs", v), dtype=np.uint64).reshape(-1)
    if v.size != 4:
        raise ValueError(f"{name} must be ONE scalar of 4 uint64 words, got {v.size}")
    return v


def _mle_eq_args(z):
    z = _arr(z, 4) if len(z) else np.zeros((0, 4), np.uint64)
    if z.shape[0] > MLE_VARS_MAX:
        raise ValueError(f"z holds {z.shape[0]} variables, at most {MLE_VARS_MAX} are supported")
    return z


def _mle_fold_args(a, r):
    """(a as a C-contiguous (rows, .., 4) array, r): the fold pairs row i with row i + rows / 2, whatever lies between the first axis and the limbs"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim < 2 or a.shape[-1] != 4:
        raise ValueError(f"a must have shape (rows, .., 4) uint64, got {a.shape}")
    if a.shape[0] % 2:
        raise ValueError(f"a holds {a.shape[0]} rows: a fold needs an even number")
    return a, _fr_point(r, "r")


def _mle_quotients_args(a, z):
    """(a as a C-contiguous (2^nv, 4) array, z as (nv, 4)): the table of a multilinear polynomial and a point of as many variables"""
    z = _mle_eq_args(z)
    a = _arr(a, 4) if len(a) else np.zeros((0, 4), np.uint64)
    if a.shape[0] != 1 << z.shape[0]:
        raise ValueError(f"a holds {a.shape[0]} values but z has {z.shape[0]} variables: 2^{z.shape[0]} are needed")
    return a, z


def _sumcheck_args(tables, groups, degree):
    """the operands of fr_sumcheck_round, checked the way the C ABI checks them (it answers BN254_E_BAD_ARG; here the caller learns which one):
    (tables as (n, k, 4), group offsets, table numbers, coefficients as (g, 4), degree)"""
    t = np.ascontiguousarray(tables, dtype=np.uint64)
    if t.ndim == 2 and t.shape[1] == 4:                            # one table
        t = t.reshape(t.shape[0], 1, 4)
    if t.ndim != 3 or t.shape[2] != 4:
        raise ValueError(f"tables must have shape (n, k, 4) uint64, got {t.shape}")
    n, k = t.shape[0], t.shape[1]
    if n < 2 or n % 2:
        raise ValueError(f"tables hold {n} indices: a round needs an even number, 2 at least")
    if not 1 <= k <= SUMCHECK_TABLES_MAX:
        raise ValueError(f"tables hold {k} tables per index, 1..{SUMCHECK_TABLES_MAX} are supported")
    groups = list(groups)
    if not 1 <= len(groups) <= SUMCHECK_GROUPS_MAX:
        raise ValueError(f"groups holds {len(groups)} products, 1..{SUMCHECK_GROUPS_MAX} are supported")
    members = [[int(j) for j in g[1]] for g in groups]
    if degree is None:
        degree = max(len(m) for m in members)
    if not 1 <= degree <= SUMCHECK_DEGREE_MAX:
        raise ValueError(f"degree must be 1..{SUMCHECK_DEGREE_MAX}, got {degree}")
    for c, m in enumerate(members):
        if not 1 <= len(m) <= degree:
            raise ValueError(f"groups[{c}] holds {len(m)} tables, 1..{degree} (the degree) are allowed")
        if min(m) < 0 or max(m) >= k:
            raise ValueError(f"groups[{c}] names table {max(m) if max(m) >= k else min(m)} but tables holds {k}")
    coeff = np.stack([_fr_point(g[0], f"the coefficient of groups[{c}]") for c, g in enumerate(groups)])
    off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.uint64)
    return t, off, np.array([j for m in members for j in m], np.uint64), coeff, degree


def _fold_round_rows(n):
    """the fused fold-then-round call folds n rows to n / 2 and the round pairs those: whole quadruples of rows"""
    if n < 4 or n % 4:
        raise ValueError(f"tables hold {n} indices: a fold and a round need a multiple of 4")


def _segment_args(p, q, offsets):
    p = _arr(p, G1_WORDS) if len(p) else np.zeros((0, G1_WORDS), np.uint64)
    q = _arr(q, G2_WORDS) if len(q) else np.zeros((0, G2_WORDS), np.uint64)
    _same_len(p, q)
    o = _offsets(offsets)
    if int(o[-1]) != p.shape[0]:
        raise ValueError(f"offsets[m] = {int(o[-1])} but {p.shape[0]} pairs were given")
    return p, q, o, np.empty((o.size - 1, GT_WORDS), np.uint64)


def _msm_args(p, k, offsets, words):
    p = _arr(p, words) if len(p) else np.zeros((0, words), np.uint64)
    k = _arr(k, 4) if len(k) else np.zeros((0, 4), np.uint64)
    _same_len(p, k)
    o = _offsets(offsets)
    if int(o[-1]) != p.shape[0]:
        raise ValueError(f"offsets[m] = {int(o[-1])} but {p.shape[0]} terms were given")
    return p, k, o, np.empty((o.size - 1, words), np.uint64)


def _msm1_args(p, k, words):
    p = _arr(p, words) if len(p) else np.zeros((0, words), np.uint64)
    k = _arr(k, 4) if len(k) else np.zeros((0, 4), np.uint64)
    _same_len(p, k)
    return p, k, np.empty(words, np.uint64)


class Engine:
    """one context = one GPU (include/bn254_hip.h: bn254_ctx)"""

    def __init__(self, device=0):
        self._lib = _native.lib()
        if self._lib.bn254_device_count() <= 0:
            raise _native.Bn254Error("no HIP device: bn_amd has no CPU fallback")
        h = C.c_void_p()
        _native.check(self._lib.bn254_ctx_create(int(device), C.byref(h)))
        self._ctx = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.bn254_ctx_destroy(self._ctx)
            self._ctx = None

    # ---- tunables (include/bn254_hip.h BN254_OPT_*): names as in _native.OPTIONS; None / a negative value restores the default
    def set_option(self, name, value):
        _native.check(self._lib.bn254_ctx_set_option(self._h, _native.OPTIONS[name], -1 if value is None else int(value)))

    def get_option(self, name):
        v = C.c_long()
        _native.check(self._lib.bn254_ctx_get_option(self._h, _native.OPTIONS[name], C.byref(v)))
        return v.value

    def get_option_raw(self, name):
        """the explicitly set value of an option, or None while its default is in effect"""
        v = C.c_long()
        _native.check(self._lib.bn254_ctx_get_option_raw(self._h, _native.OPTIONS[name], C.byref(v)))
        return None if v.value < 0 else v.value

    def options(self, **kw):
        """context manager: set the given options, restore the previous RAW state (default or explicit) on exit"""
        eng = self

        class _Scope:
            def _restore(self_):
                for k, raw in self_.saved.items():
                    eng.set_option(k, raw)

            def __enter__(self_):
                self_.saved = {k: eng.get_option_raw(k) for k in kw}          # name -> None (default) or the explicit value: read, never written
                try:
                    for k, v in kw.items():
                        eng.set_option(k, v)
                except Exception:                  # a rejected value (BN254_E_BAD_ARG) must not leave the context half-configured
                    self_._restore()
                    raise
                return eng

            def __exit__(self_, *exc):
                self_._restore()
                return False
        return _Scope()

    @property
    def _h(self):
        """the context handle; a closed engine raises instead of silently falling back to the C ABI's NULL = default context"""
        if self._ctx is None:
            raise _native.Bn254Error("this Engine is closed")
        return self._ctx

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-buffer API
    def pairing_batch(self, p, q, out=None):
        """out: optional preallocated (n,48) uint64 array (a long-running caller reuses it; a fresh np.empty pays one page fault
        per 4 KB inside the D2H copy)"""
        p = _arr(p, G1_WORDS); q = _arr(q, G2_WORDS)
        if p.shape[0] != q.shape[0]:
            raise ValueError("p and q differ in length")
        if out is None:
            out = np.empty((p.shape[0], GT_WORDS), np.uint64)
        elif out.shape != (p.shape[0], GT_WORDS) or out.dtype != np.uint64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (n,48) uint64 array")
        _native.check(self._lib.bn254_pairing_batch(self._h, _p(p), _p(q), _p(out), p.shape[0]))
        return out

    def pairing_product(self, p, q):
        p = _arr(p, G1_WORDS) if len(p) else np.zeros((0, G1_WORDS), np.uint64)
        q = _arr(q, G2_WORDS) if len(q) else np.zeros((0, G2_WORDS), np.uint64)
        if p.shape[0] != q.shape[0]:
            raise ValueError("p and q differ in length")
        out = np.empty(GT_WORDS, np.uint64)
        _native.check(self._lib.bn254_pairing_product(self._h, _p(p), _p(q), p.shape[0], _p(out)))
        return out

    def pairing_product_batch(self, p, q, offsets):
        """out[j] = fold(Gt::one(), acc * pairing(p[i], q[i])) over i in [offsets[j], offsets[j+1]) -> (m, 48) uint64;
        ONE final exponentiation per segment (include/bn254_hip.h bn254_pairing_product_batch)"""
        p, q, o, out = _segment_args(p, q, offsets)
        _native.check(self._lib.bn254_pairing_product_batch(self._h, _p(p), _p(q), _p(o), o.size - 1, _p(out)))
        return out

    def g1_mul_batch(self, p, k):
        p = _arr(p, G1_WORDS); k = _arr(k, 4); _same_len(p, k)
        out = np.empty_like(p)
        _native.check(self._lib.bn254_g1_mul_batch(self._h, _p(p), _p(k), _p(out), p.shape[0]))
        return out

    def g2_mul_batch(self, p, k):
        p = _arr(p, G2_WORDS); k = _arr(k, 4); _same_len(p, k)
        out = np.empty_like(p)
        _native.check(self._lib.bn254_g2_mul_batch(self._h, _p(p), _p(k), _p(out), p.shape[0]))
        return out

    def _mul_base(self, fn, base, k, words):
        base = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
        if base.size != words:
            raise ValueError(f"base must be ONE point of {words} uint64 words, got {base.size}")
        k = _arr(k, 4) if len(k) else np.zeros((0, 4), np.uint64)
        out = np.empty((k.shape[0], words), np.uint64)
        _native.check(fn(self._h, _p(base), _p(k), _p(out), k.shape[0]))
        return out

    def g1_mul_base_batch(self, base, k):
        """out[i] = normalize(base * k[i]) for ONE G1 point `base` (12 words) -> (n, 12) uint64: the bytes of g1_mul_batch on the tiled base,
        by mixed additions over a per-base table the context caches (include/bn254_hip.h bn254_g1_mul_base_batch)"""
        return self._mul_base(self._lib.bn254_g1_mul_base_batch, base, k, G1_WORDS)

    def g2_mul_base_batch(self, base, k):
        """the same over G2 (base: 24 words) -> (n, 24) uint64"""
        return self._mul_base(self._lib.bn254_g2_mul_base_batch, base, k, G2_WORDS)

    def _normalize(self, fn, p, words):
        p = _arr(p, words) if len(p) else np.zeros((0, words), np.uint64)
        out = np.empty_like(p)
        _native.check(fn(self._h, _p(p), _p(out), p.shape[0]))
        return out

    def g1_normalize(self, p):
        """out[i] = (x/z^2, y/z^3, 1) of the G1 point p[i], infinity (z == 0) as (0, 1, 0) -> (n, 12) uint64: the bytes of g1_mul_batch by
        Fr::one(), with one field inversion per run of points (include/bn254_hip.h bn254_g1_normalize_batch)"""
        return self._normalize(self._lib.bn254_g1_normalize_batch, p, G1_WORDS)

    def g2_normalize(self, p):
        """the same over G2 -> (n, 24) uint64"""
        return self._normalize(self._lib.bn254_g2_normalize_batch, p, G2_WORDS)

    def _eq(self, fn, a, b, words):
        a = _arr(a, words) if len(a) else np.zeros((0, words), np.uint64)
        b = _arr(b, words) if len(b) else np.zeros((0, words), np.uint64)
        _same_len(a, b)
        out = np.empty(a.shape[0], np.int32)
        _native.check(fn(self._h, _p(a), _p(b), _p(out), a.shape[0]))
        return out != 0

    def g1_eq(self, a, b):
        """out[i] = (a[i] == b[i]) as group elements, whatever their Jacobian representations -> (n,) bool; no inversion
        (include/bn254_hip.h bn254_g1_eq_batch)"""
        return self._eq(self._lib.bn254_g1_eq_batch, a, b, G1_WORDS)

    def g2_eq(self, a, b):
        """the same over G2"""
        return self._eq(self._lib.bn254_g2_eq_batch, a, b, G2_WORDS)

    # ---- the scalar field on the device (include/bn254_hip.h bn254_fr_*_batch): (n,4) uint64 Montgomery images in, the same out
    def _fr2(self, fn, a, b, *tail):
        a = _arr(a, 4) if len(a) else np.zeros((0, 4), np.uint64)
        b = _arr(b, 4) if len(b) else np.zeros((0, 4), np.uint64)
        _same_len(a, b)
        out = np.empty_like(a)
        _native.check(fn(self._h, _p(a), _p(b), _p(out), a.shape[0], *tail))
        return out

    def fr_add_batch(self, a, b, negate_b=False):
        """out[i] = a[i] + b[i] (negate_b: a[i] - b[i]) mod r -> (n, 4) uint64"""
        return self._fr2(self._lib.bn254_fr_add_batch, a, b, 1 if negate_b else 0)

    def fr_mul_batch(self, a, b):
        """out[i] = a[i] * b[i] mod r -> (n, 4) uint64"""
        return self._fr2(self._lib.bn254_fr_mul_batch, a, b)

    def fr_pow_batch(self, a, e):
        """out[i] = a[i]^(the canonical integer of e[i]) -> (n, 4) uint64; 0^0 = 1"""
        return self._fr2(self._lib.bn254_fr_pow_batch, a, e)

    def fr_inverse_batch(self, a):
        """(out, ok): out[i] = a[i]^-1 and ok[i] True, or Fr::zero() and False where a[i] is zero -> (n, 4) uint64, (n,) bool; neighbouring
        elements share one exponentiation (include/bn254_hip.h bn254_fr_inverse_batch)"""
        a = _arr(a, 4) if len(a) else np.zeros((0, 4), np.uint64)
        out = np.empty_like(a); ok = np.empty(a.shape[0], np.int32)
        _native.check(self._lib.bn254_fr_inverse_batch(self._h, _p(a), _p(out), _p(ok), a.shape[0]))
        return out, ok != 0

    def fr_sqrt_batch(self, a):
        """(out, ok): out[i] = the square root of a[i] whose canonical integer is not above (r - 1) / 2 and ok[i] True, or Fr::zero() and False
        where a[i] is a non-residue -> (n, 4) uint64, (n,) bool (include/bn254_hip.h bn254_fr_sqrt_batch)"""
        a = _arr(a, 4) if len(a) else np.zeros((0, 4), np.uint64)
        out = np.empty_like(a); ok = np.empty(a.shape[0], np.int32)
        _native.check(self._lib.bn254_fr_sqrt_batch(self._h, _p(a), _p(out), _p(ok), a.shape[0]))
        return out, ok != 0

    def fr_interpret_batch(self, buf):
        """out[i] = the 64-byte record i of `buf` as a big-endian 512-bit integer, mod r (Fr::interpret, lib.rs:27-29) -> (n, 4) uint64"""
        b = np.ascontiguousarray(buf, np.uint8).reshape(-1, 64)
        out = np.empty((b.shape[0], 4), np.uint64)
        _native.check(self._lib.bn254_fr_interpret_batch(self._h, _p(b), _p(out), b.shape[0]))
        return out

    def fr_ntt_batch(self, a, log_n, inverse=False, shift=None):
        """len(a) / 2^log_n number-theoretic transforms of 2^log_n elements each, natural order in and out -> (len(a), 4) uint64.  Forward:
        the polynomial with coefficients a evaluated at shift * w^k; inverse: back to the coefficients.  shift: ONE scalar (4 uint64 words,
        non-zero) or None for 1 (include/bn254_hip.h bn254_fr_ntt_batch)"""
        a = _arr(a, 4) if len(a) else np.zeros((0, 4), np.uint64)
        count = _ntt_count(a.shape[0], log_n)
        out = np.empty_like(a)
        shift = _ntt_shift(shift)                                  # held here until the call has returned
        _native.check(self._lib.bn254_fr_ntt_batch(self._h, _p(a), _p(out), log_n, count, 1 if inverse else 0, None if shift is None else _p(shift)))
        return out

    def _group_ntt(self, fn, p, words, log_n, inverse, shift):
        p = _arr(p, words) if len(p) else np.zeros((0, words), np.uint64)
        count = _group_ntt_count(p.shape[0], log_n)
        out = np.empty_like(p)
        shift = _ntt_shift(shift)                                  # held here until the call has returned
        _native.check(fn(self._h, _p(p), _p(out), log_n, count, 1 if inverse else 0, None if shift is None else _p(shift)))
        return out

    def g1_ntt_batch(self, p, log_n, inverse=False, shift=None):
        """len(p) / 2^log_n transforms of 2^log_n G1 points each, natural order in and out -> (len(p), 12) uint64, normalised.  Forward:
        out[k] = sum_j [shift^j w^(j k)] p[j]; inverse: out[j] = [n^-1 shift^-j] sum_k [w^(-j k)] p[k].  shift: ONE scalar (4 uint64 words,
        non-zero) or None for 1 (include/bn254_hip.h bn254_g1_ntt_batch)"""
        return self._group_ntt(self._lib.bn254_g1_ntt_batch, p, G1_WORDS, log_n, inverse, shift)

    def g2_ntt_batch(self, p, log_n, inverse=False, shift=None):
        """the same over G2 -> (len(p), 24) uint64"""
        return self._group_ntt(self._lib.bn254_g2_ntt_batch, p, G2_WORDS, log_n, inverse, shift)

    def fr_dot_batch(self, coeff, x, offsets, index=None):
        """out[j] = sum of coeff[t] * x[index[t]] over t in [offsets[j], offsets[j+1]) -> (m, 4) uint64: a sparse matrix in CSR form times the
        vector x.  index None: x[t], a plain segmented inner product (len(x) == len(coeff)).  An empty segment gives zero
        (include/bn254_hip.h bn254_fr_dot_batch)"""
        coeff, x, o, index = _dot_args(coeff, x, offsets, index)
        out = np.empty((o.size - 1, 4), np.uint64)
        _native.check(self._lib.bn254_fr_dot_batch(self._h, _p(coeff), None if index is None else _p(index), _p(x), x.shape[0], _p(o), o.size - 1, _p(out)))
        return out

    def fr_scan_batch(self, a, b, offsets, init=None, reverse=False, exclusive=False, a_per_segment=False):
        """out[t] = a[t] * prev + b[t] over the terms of every segment [offsets[j], offsets[j+1]) in order, prev = out[t-1] or init[j] at the
        segment's first term -> (n, 4) uint64.  a None: prefix sums; b None: prefix products; init None: zero with b, one without.
        reverse: from each segment's last term to its first; exclusive: out[t] = prev; a_per_segment: a holds one factor per segment
        (include/bn254_hip.h bn254_fr_scan_batch)"""
        a, b, o, init = _scan_args(a, b, offsets, init, a_per_segment)
        out = np.empty((int(o[-1]), 4), np.uint64)
        opt = lambda v: None if v is None else _p(v)
        _native.check(self._lib.bn254_fr_scan_batch(self._h, opt(a), opt(b), opt(init), _p(o), o.size - 1, _scan_flags(reverse, exclusive, a_per_segment), _p(out)))
        return out

    def fr_mle_eq(self, z):
        """the table of eq(z, .) over the hypercube of nv = len(z) variables -> (2^nv, 4) uint64: out[i] = prod_j (bit j of i ? z[j] : 1 - z[j]);
        no variables give [one] (include/bn254_hip.h bn254_fr_mle_eq)"""
        z = _mle_eq_args(z)
        out = np.empty((1 << z.shape[0], 4), np.uint64)
        _native.check(self._lib.bn254_fr_mle_eq(self._h, _p(z), z.shape[0], _p(out)))
        return out

    def fr_mle_fold(self, a, r):
        """out[i] = a[i] + r * (a[i + rows/2] - a[i]) -> (rows/2, .., 4) uint64: binds the MOST significant variable of a multilinear table to r.
        a: (rows, 4), or (rows, k, 4) - k tables stored index-major, all folded at once; r: ONE scalar (an Fr or 4 uint64 words)
        (include/bn254_hip.h bn254_fr_mle_fold)"""
        a, r = _mle_fold_args(a, r)
        out = np.empty((a.shape[0] // 2,) + a.shape[1:], np.uint64)
        _native.check(self._lib.bn254_fr_mle_fold(self._h, _p(a), a.size // 4, _p(r), _p(out)))
        return out

    def fr_sumcheck_round(self, tables, groups, degree=None):
        """the round polynomial of sum_c coeff_c * prod_{j in group c} T_j at t = 0 .. degree -> (degree + 1, 4) uint64:
        out[t] = sum over i < n/2 and the groups of coeff_c * prod_j (T_j[i] + t * (T_j[i + n/2] - T_j[i])).  tables: (n, k, 4), table j at index i
        in tables[i, j]; groups: a list of (coeff, [table numbers]); degree: None for the longest group
        (include/bn254_hip.h bn254_fr_sumcheck_round)"""
        t, off, members, coeff, degree = _sumcheck_args(tables, groups, degree)
        out = np.empty((degree + 1, 4), np.uint64)
        _native.check(self._lib.bn254_fr_sumcheck_round(self._h, _p(t), t.shape[0], t.shape[1], _p(off), _p(members), _p(coeff), off.size - 1, degree, _p(out)))
        return out

    def fr_sumcheck_fold_round(self, tables, r, groups, degree=None):
        """fr_mle_fold of the (n, k, 4) tables by r and fr_sumcheck_round of the folded tables in ONE pass -> (folded, out): folded is (n/2, k, 4),
        folded[i] = tables[i] + r * (tables[i + n/2] - tables[i]); out is (degree + 1, 4), the round polynomial of the folded tables - the bytes of
        the two calls.  n must be a multiple of 4; every table is folded, also one no group names
        (include/bn254_hip.h bn254_fr_sumcheck_fold_round)"""
        t, off, members, coeff, degree = _sumcheck_args(tables, groups, degree)
        _fold_round_rows(t.shape[0])
        r = _fr_point(r, "r")
        folded = np.empty((t.shape[0] // 2,) + t.shape[1:], np.uint64)
        out = np.empty((degree + 1, 4), np.uint64)
        _native.check(self._lib.bn254_fr_sumcheck_fold_round(self._h, _p(t), t.shape[0], t.shape[1], _p(r), _p(off), _p(members), _p(coeff), off.size - 1, degree, _p(folded), _p(out)))
        return folded, out

    def fr_mle_quotients(self, a, z):
        """the quotients of the multilinear table a (2^nv records) at the point z (nv records) -> (2^nv, 4) uint64 in heap order: out[0] = f(z) and
        out[2^j + i] = q_j[i], where f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1}) - from t = a, for j = nv - 1 down to 0,
        q_j[i] = t[i + 2^j] - t[i] and t[i] += z[j] * q_j[i] (include/bn254_hip.h bn254_fr_mle_quotients)"""
        a, z = _mle_quotients_args(a, z)
        out = np.empty_like(a)
        _native.check(self._lib.bn254_fr_mle_quotients(self._h, _p(a), z.shape[0], _p(z), _p(out)))
        return out

    def fr_poseidon_batch(self, x):
        """out[i] = Poseidon(x[i, 0], .., x[i, arity - 1]) -> (n, 4) uint64: the circomlib / iden3 hash over Fr, element 0 of the permutation of
        [0, x[i, 0], ..].  x: (n, arity, 4), arity 1 .. 4 (include/bn254_hip.h bn254_fr_poseidon_batch)"""
        x = _poseidon_args(x, "x", 1, POSEIDON_ARITY_MAX, "arity")
        out = np.empty((x.shape[0], 4), np.uint64)
        _native.check(self._lib.bn254_fr_poseidon_batch(self._h, _p(x), x.shape[1], _p(out), x.shape[0]))
        return out

    def fr_poseidon_permute_batch(self, states):
        """out[i] = the Poseidon permutation of the state states[i] -> (n, t, 4) uint64.  states: (n, t, 4), t 2 .. 5
        (include/bn254_hip.h bn254_fr_poseidon_permute_batch)"""
        x = _poseidon_args(states, "states", 2, POSEIDON_ARITY_MAX + 1, "t")
        out = np.empty_like(x)
        _native.check(self._lib.bn254_fr_poseidon_permute_batch(self._h, _p(x), x.shape[1], _p(out), x.shape[0]))
        return out

    def fr_merkle_tree(self, leaves):
        """the n - 1 inner nodes of the binary Poseidon tree over n = 2^k leaves -> (n - 1, 4) uint64, level by level: the n / 2 parents of the
        leaves, the n / 4 parents of those, .. the root last; parent i of a level is hash(child[2 i], child[2 i + 1]).  One leaf gives no
        node (include/bn254_hip.h bn254_fr_merkle_tree)"""
        x, log_n = _merkle_args(leaves)
        out = np.empty((x.shape[0] - 1, 4), np.uint64)
        _native.check(self._lib.bn254_fr_merkle_tree(self._h, _p(x), log_n, _p(out) if log_n else None))
        return out

    def fr_poseidon_ex_batch(self, x, init=None, n_outs=1):
        """circomlib's PoseidonEx per row -> (n, n_outs, 4) uint64: out[i, j] = permute([init[i] or 0, x[i, 0], .., x[i, n_inputs - 1]])[j].
        x: (n, n_inputs, 4), n_inputs 1 .. 16; init: None, (n, 4), or one record for every row; 1 <= n_outs <= n_inputs + 1
        (include/bn254_hip.h bn254_fr_poseidon_ex_batch)"""
        x, init = _poseidon_ex_args(x, init, n_outs)
        out = np.empty((x.shape[0], n_outs, 4), np.uint64)
        _native.check(self._lib.bn254_fr_poseidon_ex_batch(self._h, _p(x), x.shape[1], _p(init) if init is not None else None, n_outs, _p(out), x.shape[0]))
        return out

    def fr_poseidon_chain_batch(self, x, offsets, rate=16):
        """one digest per variable-length record -> (m, 4) uint64: record j is x[offsets[j]:offsets[j + 1]]; c = len, then per block of `rate`
        elements (the last padded with zeros, an empty record is one block of zeros) c = permute([c, block..])[0].  This framing is this
        library's own (include/bn254_hip.h bn254_fr_poseidon_chain_batch)"""
        x, o = _poseidon_chain_args(x, offsets, rate)
        out = np.empty((o.size - 1, 4), np.uint64)
        _native.check(self._lib.bn254_fr_poseidon_chain_batch(self._h, _p(x) if x.shape[0] else None, _p(o), o.size - 1, rate, _p(out) if o.size > 1 else None))
        return out

    def g1_msm_batch(self, p, k, offsets):
        """out[j] = normalize(sum of p[i] * k[i] over i in [offsets[j], offsets[j+1])) -> (m, 12) uint64; an empty or cancelling
        segment gives G1::zero() = (0, 1, 0); ONE inversion per segment (include/bn254_hip.h bn254_g1_msm_batch)"""
        p, k, o, out = _msm_args(p, k, offsets, G1_WORDS)
        _native.check(self._lib.bn254_g1_msm_batch(self._h, _p(p), _p(k), _p(o), o.size - 1, _p(out)))
        return out

    def g2_msm_batch(self, p, k, offsets):
        """the same over G2 -> (m, 24) uint64"""
        p, k, o, out = _msm_args(p, k, offsets, G2_WORDS)
        _native.check(self._lib.bn254_g2_msm_batch(self._h, _p(p), _p(k), _p(o), o.size - 1, _p(out)))
        return out

    def g1_msm(self, p, k):
        """normalize(sum of p[i] * k[i] over ALL terms) -> (12,) uint64: one large multi-scalar multiplication, by the bucket method from
        the option msm_bucket_min terms on; the bytes of g1_msm_batch(p, k, [0, n])[0] (include/bn254_hip.h bn254_g1_msm)"""
        p, k, out = _msm1_args(p, k, G1_WORDS)
        _native.check(self._lib.bn254_g1_msm(self._h, _p(p), _p(k), p.shape[0], _p(out)))
        return out

    def g2_msm(self, p, k):
        """the same over G2 -> (24,) uint64"""
        p, k, out = _msm1_args(p, k, G2_WORDS)
        _native.check(self._lib.bn254_g2_msm(self._h, _p(p), _p(k), p.shape[0], _p(out)))
        return out

    # ---- multi-scalar multiplication against prepared bases (include/bn254_hip.h bn254_g1_msm_prepare ...)
    def _msm_prepare(self, g, points, window_bits):
        words = G1_WORDS if g == 1 else G2_WORDS
        p = _arr(points, words) if len(points) else np.zeros((0, words), np.uint64)
        h = C.c_void_p()
        fn = self._lib.bn254_g1_msm_prepare if g == 1 else self._lib.bn254_g2_msm_prepare
        _native.check(fn(self._h, _p(p) if p.shape[0] else None, p.shape[0], 0 if window_bits is None else int(window_bits), C.byref(h)))
        return PreparedMSM(self, h)

    def g1_msm_prepare(self, points, window_bits=None):
        """(n,12) raw G1 points (any z) -> PreparedMSM: the affine multiples 2^(c w) P_i of every window in device memory, for many
        g1_msm_prepared calls against the same points.  window_bits: None for the default of the size, or 3 .. 16"""
        return self._msm_prepare(1, points, window_bits)

    def g2_msm_prepare(self, points, window_bits=None):
        """the same over (n,24) G2 points"""
        return self._msm_prepare(2, points, window_bits)

    def _msm_prepared(self, g, prep, k, first):
        k = _arr(k, 4) if len(k) else np.zeros((0, 4), np.uint64)
        out = np.empty(G1_WORDS if g == 1 else G2_WORDS, np.uint64)
        fn = self._lib.bn254_g1_msm_prepared if g == 1 else self._lib.bn254_g2_msm_prepared
        _native.check(fn(self._h, prep._h, int(first), _p(k) if k.shape[0] else None, k.shape[0], _p(out)))
        return out

    def g1_msm_prepared(self, prep, k, first=0):
        """normalize(sum of P[first + i] * k[i]) over the points of `prep` -> (12,) uint64: the bytes of g1_msm on those points and scalars"""
        return self._msm_prepared(1, prep, k, first)

    def g2_msm_prepared(self, prep, k, first=0):
        """the same over a G2 handle -> (24,) uint64"""
        return self._msm_prepared(2, prep, k, first)

    def g1_add_batch(self, a, b, negate_b=False):
        """a + b (a - b): the reference's Jacobian limbs (groups/mod.rs:275-347)"""
        a = _arr(a, G1_WORDS); b = _arr(b, G1_WORDS); _same_len(a, b); out = np.empty_like(a)
        _native.check(self._lib.bn254_g1_add_batch(self._h, _p(a), _p(b), _p(out), a.shape[0], 1 if negate_b else 0)); return out

    def g2_add_batch(self, a, b, negate_b=False):
        a = _arr(a, G2_WORDS); b = _arr(b, G2_WORDS); _same_len(a, b); out = np.empty_like(a)
        _native.check(self._lib.bn254_g2_add_batch(self._h, _p(a), _p(b), _p(out), a.shape[0], 1 if negate_b else 0)); return out

    def g2_precompute(self, q):
        """(n,24) G2 -> (n,102,24) line coefficients [ell_0 | ell_vw | ell_vv] (groups/mod.rs:557-588)"""
        q = _arr(q, G2_WORDS)
        out = np.empty((q.shape[0], 102, 24), np.uint64)
        _native.check(self._lib.bn254_g2_precompute(self._h, _p(q), _p(out), q.shape[0]))
        return out

    def pairing_prepared_batch(self, p, coeffs):
        """coeffs (102,24): shared by all p;  (n,102,24): one prepared point per p"""
        p = _arr(p, G1_WORDS)
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
        shared = coeffs.ndim == 2
        if coeffs.shape[-2:] != (102, 24) or (not shared and coeffs.shape[0] != p.shape[0]):
            raise ValueError("coeffs must be (102,24) or (n,102,24)")
        out = np.empty((p.shape[0], GT_WORDS), np.uint64)
        _native.check(self._lib.bn254_pairing_prepared_batch(self._h, _p(p), _p(coeffs), 1 if shared else 0, _p(out), p.shape[0]))
        return out

    # ---- native prepared-G2 mode (include/bn254_hip.h bn254_g2_prepare ...)
    def g2_prepare(self, q):
        """(n,24) G2 points (or one (24,) point) -> PreparedG2: the device-resident native line tables (one point: shared by every P)"""
        q = _arr(q, G2_WORDS)
        h = C.c_void_p()
        _native.check(self._lib.bn254_g2_prepare(self._h, _p(q), q.shape[0], C.byref(h)))
        return PreparedG2(self, h)

    def g2_prepare_dev(self, d_q, n, stream=0):
        h = C.c_void_p()
        _native.check(self._lib.bn254_g2_prepare_dev(self._h, d_q, n, C.byref(h), stream))
        return PreparedG2(self, h)

    def pairing_prepared_native_batch(self, p, prepared, out=None):
        """out[i] = pairing(p[i], Q) for a one-point handle, pairing(p[i], Q[i]) otherwise"""
        p = _arr(p, G1_WORDS)
        if out is None:
            out = np.empty((p.shape[0], GT_WORDS), np.uint64)
        _native.check(self._lib.bn254_pairing_prepared_native_batch(self._h, _p(p), prepared._h, _p(out), p.shape[0]))
        return out

    def pairing_product_prepared_native(self, p, prepared):
        """fold(Gt::one(), acc * pairing(p[i], Q[i])) over prepared points (one-point handle: against that point) -> (48,) uint64"""
        p = _arr(p, G1_WORDS) if len(p) else np.zeros((0, G1_WORDS), np.uint64)
        out = np.empty(GT_WORDS, np.uint64)
        _native.check(self._lib.bn254_pairing_product_prepared_native(self._h, _p(p), prepared._h, p.shape[0], _p(out)))
        return out

    def pairing_product_batch_prepared_native(self, p, prepared, offsets, q_index=None):
        """out[j] = fold(Gt::one(), acc * pairing(p[i], point q_index[i] of `prepared`)) over i in [offsets[j], offsets[j+1]) -> (m, 48) uint64;
        ONE final exponentiation per segment (include/bn254_hip.h bn254_pairing_product_batch_prepared_native).  q_index None: pair i uses
        point i (every pair point 0 of a one-point handle)."""
        p = _arr(p, G1_WORDS) if len(p) else np.zeros((0, G1_WORDS), np.uint64)
        o = _offsets(offsets)
        if int(o[-1]) != p.shape[0]:
            raise ValueError(f"offsets[m] = {int(o[-1])} but {p.shape[0]} pairs were given")
        qi = None
        if q_index is not None:
            qi = np.ascontiguousarray(q_index, dtype=np.uint64).reshape(-1)
            if qi.size != p.shape[0]:
                raise ValueError(f"q_index has {qi.size} entries for {p.shape[0]} pairs")
        out = np.empty((o.size - 1, GT_WORDS), np.uint64)
        _native.check(self._lib.bn254_pairing_product_batch_prepared_native(self._h, _p(p), prepared._h, None if qi is None else _p(qi), _p(o), o.size - 1, _p(out)))
        return out

    def pairing_product_batch_prepared_native_dev(self, d_p, prepared, offsets, d_out, d_q_index=None, stream=0):
        """device pointers p, out (m values) and q_index (64-bit words, or None); `offsets` is a HOST sequence of m + 1 CSR offsets"""
        o = _offsets(offsets)
        _native.check(self._lib.bn254_pairing_product_batch_prepared_native_dev(self._h, d_p, prepared._h, d_q_index, _p(o), o.size - 1, d_out, stream))

    def miller_product_prepared_native_dev(self, d_p, prepared, n, d_partial, q_first=0, stream=0):
        _native.check(self._lib.bn254_miller_product_prepared_native_dev(self._h, d_p, prepared._h, q_first, n, d_partial, stream))

    def miller_prepared_native_dev(self, d_p, prepared, d_f, n, q_first=0, stream=0):
        _native.check(self._lib.bn254_miller_prepared_native_dev(self._h, d_p, prepared._h, q_first, d_f, n, stream))

    def pairing_prepared_native_dev(self, d_p, prepared, d_out, n, q_first=0, stream=0):
        _native.check(self._lib.bn254_pairing_prepared_native_batch_dev(self._h, d_p, prepared._h, q_first, d_out, n, stream))

    # ---- wire format (fixed-size records: G1 65 bytes, G2 129 bytes)
    def fr_encode_batch(self, k):
        k = _arr(k, 4); out = np.empty((k.shape[0], 32), np.uint8)
        _native.check(self._lib.bn254_fr_encode_batch(self._h, _p(k), _p(out), k.shape[0])); return out

    def fr_decode_batch(self, b):
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32); n = b.shape[0]
        out = np.empty((n, 4), np.uint64); st = np.empty(n, np.int32)
        _native.check(self._lib.bn254_fr_decode_batch(self._h, _p(b), _p(out), _p(st), n)); return out, st

    def g1_encode_batch(self, p):
        p = _arr(p, G1_WORDS); out = np.empty((p.shape[0], 65), np.uint8)
        _native.check(self._lib.bn254_g1_encode_batch(self._h, _p(p), _p(out), p.shape[0])); return out

    def g2_encode_batch(self, p):
        p = _arr(p, G2_WORDS); out = np.empty((p.shape[0], 129), np.uint8)
        _native.check(self._lib.bn254_g2_encode_batch(self._h, _p(p), _p(out), p.shape[0])); return out

    def g1_decode_batch(self, b):
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 65); n = b.shape[0]
        out = np.empty((n, G1_WORDS), np.uint64); st = np.empty(n, np.int32)
        _native.check(self._lib.bn254_g1_decode_batch(self._h, _p(b), _p(out), _p(st), n)); return out, st

    def g2_decode_batch(self, b):
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 129); n = b.shape[0]
        out = np.empty((n, G2_WORDS), np.uint64); st = np.empty(n, np.int32)
        _native.check(self._lib.bn254_g2_decode_batch(self._h, _p(b), _p(out), _p(st), n)); return out, st

    # ---- compressed encodings (x and a sign bit: G1 32 bytes, G2 64 bytes; format "ark" or "gnark")
    def _compress(self, fn, p, words, rec, fmt):
        p = _arr(p, words); out = np.empty((p.shape[0], rec), np.uint8)
        _native.check(fn(self._h, _p(p), compressed_format(fmt), _p(out), p.shape[0])); return out

    def _decompress(self, fn, b, words, rec, fmt):
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, rec); n = b.shape[0]
        out = np.empty((n, words), np.uint64); st = np.empty(n, np.int32)
        _native.check(fn(self._h, _p(b), compressed_format(fmt), _p(out), _p(st), n)); return out, st

    def g1_compress_batch(self, p, format="ark"):
        """(n,12) uint64 points (any Jacobian form) -> (n,32) uint8 canonical records"""
        return self._compress(self._lib.bn254_g1_compress_batch, p, G1_WORDS, G1_COMPRESSED_BYTES, format)

    def g2_compress_batch(self, p, format="ark"):
        return self._compress(self._lib.bn254_g2_compress_batch, p, G2_WORDS, G2_COMPRESSED_BYTES, format)

    def g1_decompress_batch(self, b, format="ark"):
        """records -> (points (x, y, 1), int32 status: 0 ok, 3 flags, 1 range, 4 no such point, 5 not in the subgroup); rejected -> G::zero()"""
        return self._decompress(self._lib.bn254_g1_decompress_batch, b, G1_WORDS, G1_COMPRESSED_BYTES, format)

    def g2_decompress_batch(self, b, format="ark"):
        return self._decompress(self._lib.bn254_g2_decompress_batch, b, G2_WORDS, G2_COMPRESSED_BYTES, format)

    def g1_compress_batch_dev(self, d_p, d_out, n, format="ark", stream=0):
        _native.check(self._lib.bn254_g1_compress_batch_dev(self._h, d_p, compressed_format(format), d_out, n, stream))

    def g2_compress_batch_dev(self, d_p, d_out, n, format="ark", stream=0):
        _native.check(self._lib.bn254_g2_compress_batch_dev(self._h, d_p, compressed_format(format), d_out, n, stream))

    def g1_decompress_batch_dev(self, d_in, d_out, d_status, n, format="ark", stream=0):
        """device pointers: records, points and n int32 statuses"""
        _native.check(self._lib.bn254_g1_decompress_batch_dev(self._h, d_in, compressed_format(format), d_out, d_status, n, stream))

    def g2_decompress_batch_dev(self, d_in, d_out, d_status, n, format="ark", stream=0):
        _native.check(self._lib.bn254_g2_decompress_batch_dev(self._h, d_in, compressed_format(format), d_out, d_status, n, stream))

    # ---- hash to G1 (RFC 9380: the SvdW map, hash_to_curve from uniform bytes, and behind SHA-256 XMD on the device)
    def g1_map_to_curve_batch(self, u):
        """(n,48) uint8 big-endian integers (taken mod q) -> (n,12) uint64 points (x, y, 1)"""
        u = np.ascontiguousarray(u, np.uint8).reshape(-1, H2C_FIELD_BYTES); out = np.empty((u.shape[0], G1_WORDS), np.uint64)
        _native.check(self._lib.bn254_g1_map_to_curve_batch(self._h, _p(u), _p(out), u.shape[0])); return out

    def g1_hash_to_curve_uniform_batch(self, uniform):
        """(n,96) uint8 uniform bytes -> (n,12) uint64: map(u0) + map(u1), normalised"""
        b = np.ascontiguousarray(uniform, np.uint8).reshape(-1, H2C_UNIFORM_BYTES); out = np.empty((b.shape[0], G1_WORDS), np.uint64)
        _native.check(self._lib.bn254_g1_hash_to_curve_uniform_batch(self._h, _p(b), _p(out), b.shape[0])); return out

    def g1_hash_to_curve_batch(self, msgs, dst):
        """(n,msg_len) uint8 messages of one length and a tag of 1 .. 255 bytes -> (n,12) uint64: hash_to_curve with SHA-256 XMD on the device"""
        msgs = np.ascontiguousarray(msgs, np.uint8)
        if msgs.ndim != 2:
            raise ValueError(f"msgs must be an (n, msg_len) uint8 array, got shape {msgs.shape}")
        dst = h2c_dst(dst); n, ml = msgs.shape
        out = np.empty((n, G1_WORDS), np.uint64)
        _native.check(self._lib.bn254_g1_hash_to_curve_batch(self._h, _p(msgs) if msgs.size else None, ml, dst, len(dst), _p(out), n)); return out

    def g1_map_to_curve_batch_dev(self, d_u, d_out, n, stream=0):
        _native.check(self._lib.bn254_g1_map_to_curve_batch_dev(self._h, d_u, d_out, n, stream))

    def g1_hash_to_curve_uniform_batch_dev(self, d_uniform, d_out, n, stream=0):
        _native.check(self._lib.bn254_g1_hash_to_curve_uniform_batch_dev(self._h, d_uniform, d_out, n, stream))

    def g1_hash_to_curve_batch_dev(self, d_msgs, msg_len, dst, d_out, n, stream=0):
        """device pointers for messages and points; `dst` is host bytes (it travels as a kernel argument)"""
        dst = h2c_dst(dst)
        _native.check(self._lib.bn254_g1_hash_to_curve_batch_dev(self._h, d_msgs, msg_len, dst, len(dst), d_out, n, stream))

    # ---- hash to G2 (RFC 9380 over Fq2 and the cofactor clearing [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P); neither the constants nor the
    # outputs are checked against gnark-crypto or any other library)
    def g2_map_to_curve_batch(self, u):
        """(n,96) uint8: c0 then c1, big-endian integers (taken mod q) -> (n,24) uint64 points (x, y, 1) of the twist, NOT in G2"""
        u = np.ascontiguousarray(u, np.uint8).reshape(-1, H2C_G2_FIELD_BYTES); out = np.empty((u.shape[0], G2_WORDS), np.uint64)
        _native.check(self._lib.bn254_g2_map_to_curve_batch(self._h, _p(u), _p(out), u.shape[0])); return out

    def g2_clear_cofactor_batch(self, p):
        """(n,24) uint64 Jacobian points of the twist (on the curve: the caller's responsibility) -> (n,24) uint64 points of G2, normalised"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, G2_WORDS); out = np.empty_like(p)
        _native.check(self._lib.bn254_g2_clear_cofactor_batch(self._h, _p(p), _p(out), p.shape[0])); return out

    def g2_hash_to_curve_uniform_batch(self, uniform):
        """(n,192) uint8 uniform bytes u0.c0 | u0.c1 | u1.c0 | u1.c1 -> (n,24) uint64: clear(map(u0) + map(u1)), normalised"""
        b = np.ascontiguousarray(uniform, np.uint8).reshape(-1, H2C_G2_UNIFORM_BYTES); out = np.empty((b.shape[0], G2_WORDS), np.uint64)
        _native.check(self._lib.bn254_g2_hash_to_curve_uniform_batch(self._h, _p(b), _p(out), b.shape[0])); return out

    def g2_hash_to_curve_batch(self, msgs, dst):
        """(n,msg_len) uint8 messages of one length and a tag of 1 .. 255 bytes -> (n,24) uint64: hash_to_curve with SHA-256 XMD on the device"""
        msgs = np.ascontiguousarray(msgs, np.uint8)
        if msgs.ndim != 2:
            raise ValueError(f"msgs must be an (n, msg_len) uint8 array, got shape {msgs.shape}")
        dst = h2c_dst(dst); n, ml = msgs.shape
        out = np.empty((n, G2_WORDS), np.uint64)
        _native.check(self._lib.bn254_g2_hash_to_curve_batch(self._h, _p(msgs) if msgs.size else None, ml, dst, len(dst), _p(out), n)); return out

    def g2_map_to_curve_batch_dev(self, d_u, d_out, n, stream=0):
        _native.check(self._lib.bn254_g2_map_to_curve_batch_dev(self._h, d_u, d_out, n, stream))

    def g2_clear_cofactor_batch_dev(self, d_p, d_out, n, stream=0):
        """d_out may be exactly d_p"""
        _native.check(self._lib.bn254_g2_clear_cofactor_batch_dev(self._h, d_p, d_out, n, stream))

    def g2_hash_to_curve_uniform_batch_dev(self, d_uniform, d_out, n, stream=0):
        _native.check(self._lib.bn254_g2_hash_to_curve_uniform_batch_dev(self._h, d_uniform, d_out, n, stream))

    def g2_hash_to_curve_batch_dev(self, d_msgs, msg_len, dst, d_out, n, stream=0):
        """device pointers for messages and points; `dst` is host bytes (it travels as a kernel argument)"""
        dst = h2c_dst(dst)
        _native.check(self._lib.bn254_g2_hash_to_curve_batch_dev(self._h, d_msgs, msg_len, dst, len(dst), d_out, n, stream))

    # ---- validation of raw points: what every other call trusts its caller to have done
    def g1_validate_batch(self, p):
        """(n,12) uint64 raw records (x, y, z), any z -> (n,) int32 status: 0 valid (infinity, z == 0, included), 1 a coordinate is not below q,
        4 not on the curve"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, G1_WORDS); st = np.empty(p.shape[0], np.int32)
        _native.check(self._lib.bn254_g1_validate_batch(self._h, _p(p), _p(st), p.shape[0])); return st

    def g2_validate_batch(self, p):
        """(n,24) uint64 raw records -> (n,) int32 status: as for G1, and 5 for a point of the twist outside the order-r subgroup (the
        endomorphism subgroup test [u + 1]P + psi([u]P) + psi^2([u]P) == psi^3([2u]P))"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, G2_WORDS); st = np.empty(p.shape[0], np.int32)
        _native.check(self._lib.bn254_g2_validate_batch(self._h, _p(p), _p(st), p.shape[0])); return st

    def g1_validate_batch_dev(self, d_p, d_status, n, stream=0):
        """device pointers: records and n int32 statuses"""
        _native.check(self._lib.bn254_g1_validate_batch_dev(self._h, d_p, d_status, n, stream))

    def g2_validate_batch_dev(self, d_p, d_status, n, stream=0):
        _native.check(self._lib.bn254_g2_validate_batch_dev(self._h, d_p, d_status, n, stream))

    # ---- Baby Jubjub (the twisted Edwards curve over Fr; a point is two Fr, x then y, affine) and EdDSA-Poseidon on it
    def bjj_validate_batch(self, p):
        """(n,2,4) uint64 raw records -> (n,) int32 status: 0 valid (O included), 1 a coordinate's words are not below r, 4 not on the curve,
        5 on the curve but [l]P != O"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); st = np.empty(p.shape[0], np.int32)
        _native.check(self._lib.bn254_bjj_validate_batch(self._h, _p(p), _p(st), p.shape[0])); return st

    def bjj_add_batch(self, p, q):
        """(n,2,4) + (n,2,4) uint64 points of the curve -> (n,2,4): the complete affine sum"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); q = np.ascontiguousarray(q, np.uint64).reshape(-1, 2, 4)
        if p.shape != q.shape:
            raise ValueError(f"{p.shape[0]} points, {q.shape[0]} points")
        out = np.empty_like(p)
        _native.check(self._lib.bn254_bjj_add_batch(self._h, _p(p), _p(q), _p(out), p.shape[0])); return out

    def bjj_mul_batch(self, p, k):
        """(n,2,4) uint64 points of the curve, (n,4) uint64 Fr -> (n,2,4): [canonical integer of k] p, affine"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); k = np.ascontiguousarray(k, np.uint64).reshape(-1, 4)
        if p.shape[0] != k.shape[0]:
            raise ValueError(f"{p.shape[0]} points, {k.shape[0]} scalars")
        out = np.empty_like(p)
        _native.check(self._lib.bn254_bjj_mul_batch(self._h, _p(p), _p(k), _p(out), p.shape[0])); return out

    def eddsa_poseidon_challenge_batch(self, a, r8, msg):
        """(n,2,4) keys, (n,2,4) points R8, (n,4) messages -> (n,4) uint64: Poseidon5(r8.x, r8.y, a.x, a.y, msg), no curve check"""
        a = np.ascontiguousarray(a, np.uint64).reshape(-1, 2, 4); r8 = np.ascontiguousarray(r8, np.uint64).reshape(-1, 2, 4)
        msg = np.ascontiguousarray(msg, np.uint64).reshape(-1, 4)
        if not a.shape[0] == r8.shape[0] == msg.shape[0]:
            raise ValueError(f"{a.shape[0]} keys, {r8.shape[0]} points, {msg.shape[0]} messages")
        out = np.empty_like(msg)
        _native.check(self._lib.bn254_eddsa_poseidon_challenge_batch(self._h, _p(a), _p(r8), _p(msg), _p(out), a.shape[0])); return out

    def eddsa_poseidon_verify_batch(self, a, r8, s, msg):
        """keys, points R8, scalars S, messages -> (n,) int32 status: 1 a word array is not below r or S >= l, 4 R8 or A is not on the curve,
        6 [S]B8 != R8 + [8 hm]A, 0 valid"""
        a = np.ascontiguousarray(a, np.uint64).reshape(-1, 2, 4); r8 = np.ascontiguousarray(r8, np.uint64).reshape(-1, 2, 4)
        s = np.ascontiguousarray(s, np.uint64).reshape(-1, 4); msg = np.ascontiguousarray(msg, np.uint64).reshape(-1, 4)
        if not a.shape[0] == r8.shape[0] == s.shape[0] == msg.shape[0]:
            raise ValueError(f"{a.shape[0]} keys, {r8.shape[0]} points, {s.shape[0]} scalars, {msg.shape[0]} messages")
        st = np.empty(a.shape[0], np.int32)
        _native.check(self._lib.bn254_eddsa_poseidon_verify_batch(self._h, _p(a), _p(r8), _p(s), _p(msg), _p(st), a.shape[0])); return st

    def bjj_pack_batch(self, p):
        """(n,2,4) uint64 points -> (n,32) uint8: y little endian, bit 7 of byte 31 set iff the integer of x is above (r - 1) / 2; no validation"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); out = np.empty((p.shape[0], 32), np.uint8)
        _native.check(self._lib.bn254_bjj_pack_batch(self._h, _p(p), _p(out), p.shape[0])); return out

    def bjj_unpack_batch(self, in32):
        """(n,32) uint8 -> ((n,2,4) uint64 points, (n,) int32 status): 1 y is not below r, 4 no point has this y, 3 x == 0 with the sign bit
        set, 0 otherwise; a rejected record gives O = (0, 1).  No subgroup check"""
        b = np.ascontiguousarray(in32, np.uint8).reshape(-1, 32)
        out = np.empty((b.shape[0], 2, 4), np.uint64); st = np.empty(b.shape[0], np.int32)
        _native.check(self._lib.bn254_bjj_unpack_batch(self._h, _p(b), _p(out), _p(st), b.shape[0])); return out, st

    def eddsa_poseidon_verify_packed_batch(self, a32, sig64, msg):
        """(n,32) uint8 packed keys, (n,64) uint8 packed signatures, (n,4) messages -> (n,) int32 status: 1 a y, S or msg is out of range, 4 a
        point has no x, 3 a non-canonical sign, 6 [S]B8 != R8 + [8 hm]A, 0 valid.  One launch: a lane unpacks its two points and verifies"""
        a32 = np.ascontiguousarray(a32, np.uint8).reshape(-1, 32); sig64 = np.ascontiguousarray(sig64, np.uint8).reshape(-1, 64)
        msg = np.ascontiguousarray(msg, np.uint64).reshape(-1, 4)
        if not a32.shape[0] == sig64.shape[0] == msg.shape[0]:
            raise ValueError(f"{a32.shape[0]} keys, {sig64.shape[0]} signatures, {msg.shape[0]} messages")
        st = np.empty(msg.shape[0], np.int32)
        _native.check(self._lib.bn254_eddsa_poseidon_verify_packed_batch(self._h, _p(a32), _p(sig64), _p(msg), _p(st), msg.shape[0])); return st

    def bjj_pack_batch_dev(self, d_p, d_out32, n, stream=0):
        """device pointers: n points and 32 n bytes"""
        _native.check(self._lib.bn254_bjj_pack_batch_dev(self._h, d_p, d_out32, n, stream))

    def bjj_unpack_batch_dev(self, d_in32, d_out, d_status, n, stream=0):
        """device pointers: 32 n bytes, n points and n int32 statuses"""
        _native.check(self._lib.bn254_bjj_unpack_batch_dev(self._h, d_in32, d_out, d_status, n, stream))

    def eddsa_poseidon_verify_packed_batch_dev(self, d_a32, d_sig64, d_msg, d_status, n, stream=0):
        _native.check(self._lib.bn254_eddsa_poseidon_verify_packed_batch_dev(self._h, d_a32, d_sig64, d_msg, d_status, n, stream))

    def bjj_validate_batch_dev(self, d_p, d_status, n, stream=0):
        """device pointers: records and n int32 statuses"""
        _native.check(self._lib.bn254_bjj_validate_batch_dev(self._h, d_p, d_status, n, stream))

    def bjj_add_batch_dev(self, d_p, d_q, d_out, n, stream=0):
        """d_out may be exactly d_p or d_q"""
        _native.check(self._lib.bn254_bjj_add_batch_dev(self._h, d_p, d_q, d_out, n, stream))

    def bjj_mul_batch_dev(self, d_p, d_k, d_out, n, stream=0):
        """d_out may be exactly d_p"""
        _native.check(self._lib.bn254_bjj_mul_batch_dev(self._h, d_p, d_k, d_out, n, stream))

    def eddsa_poseidon_challenge_batch_dev(self, d_a, d_r8, d_msg, d_out, n, stream=0):
        _native.check(self._lib.bn254_eddsa_poseidon_challenge_batch_dev(self._h, d_a, d_r8, d_msg, d_out, n, stream))

    def eddsa_poseidon_verify_batch_dev(self, d_a, d_r8, d_s, d_msg, d_status, n, stream=0):
        _native.check(self._lib.bn254_eddsa_poseidon_verify_batch_dev(self._h, d_a, d_r8, d_s, d_msg, d_status, n, stream))

    # ---- Grumpkin (y^2 = x^3 - 17 over Fr, of prime order q; a point is two Fr, x then y, affine, O = (0, 0); a scalar is 32 little-endian bytes)
    def grumpkin_validate_batch(self, p):
        """(n,2,4) uint64 raw records -> (n,) int32 status: 0 a point of the curve (O = (0, 0) included), 1 a coordinate's words are not below r,
        4 not on the curve"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); st = np.empty(p.shape[0], np.int32)
        _native.check(self._lib.bn254_grumpkin_validate_batch(self._h, _p(p), _p(st), p.shape[0])); return st

    def grumpkin_add_batch(self, p, q):
        """(n,2,4) + (n,2,4) uint64 points of the curve -> (n,2,4): the complete sum, affine"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); q = np.ascontiguousarray(q, np.uint64).reshape(-1, 2, 4)
        if p.shape != q.shape:
            raise ValueError(f"{p.shape[0]} points, {q.shape[0]} points")
        out = np.empty_like(p)
        _native.check(self._lib.bn254_grumpkin_add_batch(self._h, _p(p), _p(q), _p(out), p.shape[0])); return out

    def grumpkin_mul_batch(self, p, k):
        """(n,2,4) uint64 points of the curve, (n,4) uint64 plain 256-bit integers (not Montgomery images) -> (n,2,4): [k] p, affine"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); k = np.ascontiguousarray(k, np.uint64).reshape(-1, 4)
        if p.shape[0] != k.shape[0]:
            raise ValueError(f"{p.shape[0]} points, {k.shape[0]} scalars")
        out = np.empty_like(p)
        _native.check(self._lib.bn254_grumpkin_mul_batch(self._h, _p(p), _p(k), _p(out), p.shape[0])); return out

    def grumpkin_msm_batch(self, p, k, offsets):
        """out[j] = sum of [k[t]] p[t] over t in [offsets[j], offsets[j+1]) -> (m,2,4) uint64; an empty or cancelling segment gives O = (0, 0)
        (include/bn254_hip.h bn254_grumpkin_msm_batch)"""
        p = np.ascontiguousarray(p, np.uint64).reshape(-1, 2, 4); k = np.ascontiguousarray(k, np.uint64).reshape(-1, 4)
        if p.shape[0] != k.shape[0]:
            raise ValueError(f"{p.shape[0]} points, {k.shape[0]} scalars")
        o = _offsets(offsets)
        if int(o[-1]) != p.shape[0]:
            raise ValueError(f"offsets[m] = {int(o[-1])} but {p.shape[0]} terms were given")
        out = np.empty((o.size - 1, 2, 4), np.uint64)
        _native.check(self._lib.bn254_grumpkin_msm_batch(self._h, _p(p), _p(k), _p(o), o.size - 1, _p(out))); return out

    def grumpkin_validate_batch_dev(self, d_p, d_status, n, stream=0):
        """device pointers: records and n int32 statuses"""
        _native.check(self._lib.bn254_grumpkin_validate_batch_dev(self._h, d_p, d_status, n, stream))

    def grumpkin_add_batch_dev(self, d_p, d_q, d_out, n, stream=0):
        """d_out may be exactly d_p or d_q"""
        _native.check(self._lib.bn254_grumpkin_add_batch_dev(self._h, d_p, d_q, d_out, n, stream))

    def grumpkin_mul_batch_dev(self, d_p, d_k, d_out, n, stream=0):
        """d_out may be exactly d_p"""
        _native.check(self._lib.bn254_grumpkin_mul_batch_dev(self._h, d_p, d_k, d_out, n, stream))

    def grumpkin_msm_batch_dev(self, d_p, d_k, offsets, m, d_out, stream=0):
        """device pointers p (offsets[m] points), k (as many 32-byte scalars) and out (m points; must not overlap the inputs), ordered on
        `stream`; `offsets` is a HOST sequence of m + 1 CSR offsets, read before the call returns"""
        o = _offsets(offsets)
        if o.size != m + 1:
            raise ValueError(f"{m} segments need {m + 1} offsets, got {o.size}")
        _native.check(self._lib.bn254_grumpkin_msm_batch_dev(self._h, d_p, d_k, _p(o), m, d_out, stream))

    # ---- the crate's variable-length byte stream (infinity = the lone byte 0)
    def _encode_stream(self, fn, p, rec):
        out = np.empty(p.shape[0] * rec, np.uint8); w = C.c_size_t()
        _native.check(fn(self._h, _p(p), p.shape[0], _p(out), out.size, C.byref(w)))
        return out[:w.value].copy()

    def g1_encode_stream(self, p):
        return self._encode_stream(self._lib.bn254_g1_encode_stream, _arr(p, G1_WORDS), 65)

    def g2_encode_stream(self, p):
        return self._encode_stream(self._lib.bn254_g2_encode_stream, _arr(p, G2_WORDS), 129)

    def _decode_stream(self, fn, b, words, max_points):
        b = np.ascontiguousarray(b, np.uint8).reshape(-1)
        cap = b.size if max_points is None else int(max_points)
        out = np.zeros((max(cap, 1), words), np.uint64); st = np.zeros(max(cap, 1), np.int32); cnt = C.c_size_t(); used = C.c_size_t()
        _native.check(fn(self._h, _p(b), b.size, _p(out), _p(st), cap, C.byref(cnt), C.byref(used)))
        return out[:cnt.value], st[:cnt.value], used.value

    def g1_decode_stream(self, b, max_points=None):
        """bytes -> (points, status, bytes consumed)"""
        return self._decode_stream(self._lib.bn254_g1_decode_stream, b, G1_WORDS, max_points)

    def g2_decode_stream(self, b, max_points=None):
        return self._decode_stream(self._lib.bn254_g2_decode_stream, b, G2_WORDS, max_points)

    def gt_mul_batch(self, a, b):
        a = _arr(a, GT_WORDS); b = _arr(b, GT_WORDS); _same_len(a, b)
        out = np.empty_like(a)
        _native.check(self._lib.bn254_gt_mul_batch(self._h, _p(a), _p(b), _p(out), a.shape[0]))
        return out

    def gt_pow_batch(self, a, k):
        a = _arr(a, GT_WORDS); k = _arr(k, 4); _same_len(a, k)
        out = np.empty_like(a)
        _native.check(self._lib.bn254_gt_pow_batch(self._h, _p(a), _p(k), _p(out), a.shape[0]))
        return out

    def gt_inverse_batch(self, a):
        """Gt::inverse (lib.rs:172)"""
        a = _arr(a, GT_WORDS)
        out = np.empty_like(a)
        _native.check(self._lib.bn254_gt_inverse_batch(self._h, _p(a), _p(out), a.shape[0]))
        return out

    # ---- device-resident API: raw device pointers (ints) + hipStream_t (int or 0)
    def pairing_batch_dev(self, d_p, d_q, d_out, n, stream=0):
        _native.check(self._lib.bn254_pairing_batch_dev(self._h, d_p, d_q, d_out, n, stream))

    def miller_batch_dev(self, d_p, d_q, d_f, n, stream=0):
        _native.check(self._lib.bn254_miller_batch_dev(self._h, d_p, d_q, d_f, n, stream))

    def final_exp_batch_dev(self, d_f, d_out, n, stream=0):
        _native.check(self._lib.bn254_final_exp_batch_dev(self._h, d_f, d_out, n, stream))

    def gt_product_dev(self, d_in, n, d_out, stream=0):
        _native.check(self._lib.bn254_gt_product_dev(self._h, d_in, n, d_out, stream))

    def gt_product_final_exp_dev(self, d_in, m, d_out, stream=0):
        _native.check(self._lib.bn254_gt_product_final_exp_dev(self._h, d_in, m, d_out, stream))

    def miller_product_dev(self, d_p, d_q, n, d_partial, stream=0):
        _native.check(self._lib.bn254_miller_product_dev(self._h, d_p, d_q, n, d_partial, stream))

    def pairing_product_batch_dev(self, d_p, d_q, offsets, d_out, stream=0):
        """device pointers p, q, out (m values); `offsets` is a HOST sequence of m + 1 CSR offsets"""
        o = _offsets(offsets)
        _native.check(self._lib.bn254_pairing_product_batch_dev(self._h, d_p, d_q, _p(o), o.size - 1, d_out, stream))

    def g2_precompute_dev(self, d_q, d_coeffs, n, stream=0):
        _native.check(self._lib.bn254_g2_precompute_dev(self._h, d_q, d_coeffs, n, stream))

    def miller_prepared_dev(self, d_p, d_coeffs, shared, d_f, n, stream=0):
        _native.check(self._lib.bn254_miller_prepared_dev(self._h, d_p, d_coeffs, 1 if shared else 0, d_f, n, stream))

    def g1_mul_dev(self, d_p, d_k, d_out, n, stream=0, normalize=True):
        f = self._lib.bn254_g1_mul_batch_dev if normalize else self._lib.bn254_g1_mul_jacobian_dev
        _native.check(f(self._h, d_p, d_k, d_out, n, stream))

    def g2_mul_dev(self, d_p, d_k, d_out, n, stream=0, normalize=True):
        f = self._lib.bn254_g2_mul_batch_dev if normalize else self._lib.bn254_g2_mul_jacobian_dev
        _native.check(f(self._h, d_p, d_k, d_out, n, stream))

    def g1_normalize_dev(self, d_p, d_out, n, stream=0):
        """device pointers p, out (n points; out may be p), ordered on `stream`"""
        _native.check(self._lib.bn254_g1_normalize_batch_dev(self._h, d_p, d_out, n, stream))

    def g2_normalize_dev(self, d_p, d_out, n, stream=0):
        _native.check(self._lib.bn254_g2_normalize_batch_dev(self._h, d_p, d_out, n, stream))

    def g1_eq_dev(self, d_a, d_b, d_out, n, stream=0):
        """device pointers a, b (n points) and out (n int32: 1 or 0), ordered on `stream`"""
        _native.check(self._lib.bn254_g1_eq_batch_dev(self._h, d_a, d_b, d_out, n, stream))

    def g2_eq_dev(self, d_a, d_b, d_out, n, stream=0):
        _native.check(self._lib.bn254_g2_eq_batch_dev(self._h, d_a, d_b, d_out, n, stream))

    def fr_add_batch_dev(self, d_a, d_b, d_out, n, negate_b=False, stream=0):
        """device pointers a, b, out (n records of 32 bytes; out may be a or b), ordered on `stream`"""
        _native.check(self._lib.bn254_fr_add_batch_dev(self._h, d_a, d_b, d_out, n, 1 if negate_b else 0, stream))

    def fr_mul_batch_dev(self, d_a, d_b, d_out, n, stream=0):
        _native.check(self._lib.bn254_fr_mul_batch_dev(self._h, d_a, d_b, d_out, n, stream))

    def fr_pow_batch_dev(self, d_a, d_e, d_out, n, stream=0):
        _native.check(self._lib.bn254_fr_pow_batch_dev(self._h, d_a, d_e, d_out, n, stream))

    def fr_inverse_batch_dev(self, d_a, d_out, d_ok, n, stream=0):
        """d_ok: n int32 (1 / 0), or None"""
        _native.check(self._lib.bn254_fr_inverse_batch_dev(self._h, d_a, d_out, d_ok, n, stream))

    def fr_sqrt_batch_dev(self, d_a, d_out, d_ok, n, stream=0):
        """d_ok: n int32 (1 / 0), or None; d_out may be exactly d_a"""
        _native.check(self._lib.bn254_fr_sqrt_batch_dev(self._h, d_a, d_out, d_ok, n, stream))

    def fr_interpret_batch_dev(self, d_in, d_out, n, stream=0):
        """d_in: 64 n bytes, d_out: n records"""
        _native.check(self._lib.bn254_fr_interpret_batch_dev(self._h, d_in, d_out, n, stream))

    def fr_ntt_batch_dev(self, d_in, d_out, log_n, count, inverse=False, shift=None, stream=0):
        """device pointers in, out (count * 2^log_n records of 32 bytes; out may be in), ordered on `stream`; `shift` is a HOST scalar (4 uint64
        words) or None, read before the call returns"""
        shift = _ntt_shift(shift)                                  # held here until the call has returned (it reads the shift before it does)
        _native.check(self._lib.bn254_fr_ntt_batch_dev(self._h, d_in, d_out, log_n, count, 1 if inverse else 0, None if shift is None else _p(shift), stream))

    def g1_ntt_batch_dev(self, d_in, d_out, log_n, count, inverse=False, shift=None, stream=0):
        """device pointers in, out (count * 2^log_n records of 96 bytes; out may be in), ordered on `stream`; `shift` is a HOST scalar (4 uint64
        words) or None, read before the call returns"""
        shift = _ntt_shift(shift)                                  # held here until the call has returned (it reads the shift before it does)
        _native.check(self._lib.bn254_g1_ntt_batch_dev(self._h, d_in, d_out, log_n, count, 1 if inverse else 0, None if shift is None else _p(shift), stream))

    def g2_ntt_batch_dev(self, d_in, d_out, log_n, count, inverse=False, shift=None, stream=0):
        """the same over G2: records of 192 bytes"""
        shift = _ntt_shift(shift)                                  # held here until the call has returned (it reads the shift before it does)
        _native.check(self._lib.bn254_g2_ntt_batch_dev(self._h, d_in, d_out, log_n, count, 1 if inverse else 0, None if shift is None else _p(shift), stream))

    def fr_dot_batch_dev(self, d_coeff, d_index, d_x, nx, offsets, m, d_out, stream=0):
        """device pointers coeff (offsets[m] records of 32 bytes), index (as many 64-bit words, or None), x (nx records), out (m records),
        ordered on `stream`; `offsets` is a HOST sequence of m + 1 CSR offsets, read before the call returns.  The index is not checked here:
        an entry >= nx contributes zero"""
        o = _offsets(offsets)
        if o.size != m + 1:
            raise ValueError(f"{m} segments need {m + 1} offsets, got {o.size}")
        _native.check(self._lib.bn254_fr_dot_batch_dev(self._h, d_coeff, d_index, d_x, nx, _p(o), m, d_out, stream))

    def fr_scan_batch_dev(self, d_a, d_b, d_init, offsets, m, d_out, reverse=False, exclusive=False, a_per_segment=False, stream=0):
        """device pointers a, b (offsets[m] records of 32 bytes; a_per_segment: a has m; either may be None), init (m records, or None) and
        out (offsets[m] records; may be d_a or d_b), ordered on `stream`; `offsets` is a HOST sequence of m + 1 CSR offsets, read before the
        call returns"""
        o = _offsets(offsets)
        if o.size != m + 1:
            raise ValueError(f"{m} segments need {m + 1} offsets, got {o.size}")
        _native.check(self._lib.bn254_fr_scan_batch_dev(self._h, d_a, d_b, d_init, _p(o), m, _scan_flags(reverse, exclusive, a_per_segment), d_out, stream))

    def fr_mle_eq_dev(self, d_z, nv, d_out, stream=0):
        """device pointers z (nv records of 32 bytes) and out (2^nv records), ordered on `stream`"""
        _native.check(self._lib.bn254_fr_mle_eq_dev(self._h, d_z, nv, d_out, stream))

    def fr_mle_fold_dev(self, d_in, length, r, d_out, stream=0):
        """device pointers in (`length` records of 32 bytes) and out (length / 2 records; may be d_in: the upper half is then left as it was),
        ordered on `stream`; `r` is a HOST scalar (an Fr or 4 uint64 words), read before the call returns"""
        r = _fr_point(r, "r")                                      # held here until the call has returned
        _native.check(self._lib.bn254_fr_mle_fold_dev(self._h, d_in, length, _p(r), d_out, stream))

    def fr_sumcheck_round_dev(self, d_tables, n, k, groups, d_out, degree=None, stream=0):
        """device pointers tables (n * k records of 32 bytes, table j at index i in record i * k + j) and out (degree + 1 records), ordered on
        `stream`; `groups` is a HOST list of (coeff, [table numbers]), read before the call returns.  Returns the degree it ran with"""
        members = [[int(j) for j in g[1]] for g in groups]
        if degree is None:
            degree = max((len(m) for m in members), default=0)
        coeff = np.stack([_fr_point(g[0], f"the coefficient of groups[{c}]") for c, g in enumerate(groups)]) if members else np.zeros((0, 4), np.uint64)
        off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.uint64)
        flat = np.array([j for m in members for j in m] or [0], np.uint64)
        _native.check(self._lib.bn254_fr_sumcheck_round_dev(self._h, d_tables, n, k, _p(off), _p(flat), _p(coeff), len(members), degree, d_out, stream))
        return degree

    def fr_sumcheck_fold_round_dev(self, d_tables, n, k, r, groups, d_folded, d_out, degree=None, stream=0):
        """device pointers tables (n * k records of 32 bytes, table j at index i in record i * k + j; n a multiple of 4), folded (n / 2 * k records;
        may be d_tables: the call then runs in place and rows [n/2, n) are left as they were) and out (degree + 1 records), ordered on `stream`;
        `r` (an Fr or 4 uint64 words) and `groups`, a list of (coeff, [table numbers]), are HOST values, read before the call returns.  Returns
        the degree it ran with"""
        members = [[int(j) for j in g[1]] for g in groups]
        if degree is None:
            degree = max((len(m) for m in members), default=0)
        r = _fr_point(r, "r")                                      # held here until the call has returned
        coeff = np.stack([_fr_point(g[0], f"the coefficient of groups[{c}]") for c, g in enumerate(groups)]) if members else np.zeros((0, 4), np.uint64)
        off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.uint64)
        flat = np.array([j for m in members for j in m] or [0], np.uint64)
        _native.check(self._lib.bn254_fr_sumcheck_fold_round_dev(self._h, d_tables, n, k, _p(r), _p(off), _p(flat), _p(coeff), len(members), degree, d_folded, d_out, stream))
        return degree

    def fr_mle_quotients_dev(self, d_a, z, d_out, stream=0):
        """device pointers a and out (2^nv records of 32 bytes each; out must not overlap a, which is never written), ordered on `stream`; `z`
        is a HOST array of nv scalars, read before the call returns"""
        z = _mle_eq_args(z)                                        # held here until the call has returned
        _native.check(self._lib.bn254_fr_mle_quotients_dev(self._h, d_a, z.shape[0], _p(z), d_out, stream))

    def fr_poseidon_batch_dev(self, d_in, arity, d_out, n, stream=0):
        """device pointers in (n * arity records of 32 bytes, row-major) and out (n records; must not overlap in), ordered on `stream`"""
        _native.check(self._lib.bn254_fr_poseidon_batch_dev(self._h, d_in, arity, d_out, n, stream))

    def fr_poseidon_permute_batch_dev(self, d_in, t, d_out, n, stream=0):
        """device pointers in and out (n states of t records of 32 bytes each; out may be exactly in), ordered on `stream`"""
        _native.check(self._lib.bn254_fr_poseidon_permute_batch_dev(self._h, d_in, t, d_out, n, stream))

    def fr_merkle_tree_dev(self, d_leaves, log_n, d_nodes, stream=0):
        """device pointers leaves (2^log_n records of 32 bytes) and nodes (2^log_n - 1 records, level by level, the root last; must not overlap
        leaves), ordered on `stream`: one launch per level"""
        _native.check(self._lib.bn254_fr_merkle_tree_dev(self._h, d_leaves, log_n, d_nodes, stream))

    def fr_poseidon_ex_batch_dev(self, d_in, n_inputs, d_init, n_outs, d_out, n, stream=0):
        """device pointers in (n * n_inputs records of 32 bytes, row-major), init (n records, or None / 0 for zeros) and out (n * n_outs records;
        must overlap no input), ordered on `stream`.  The first call of a width on the engine blocks while its constants go to the device"""
        _native.check(self._lib.bn254_fr_poseidon_ex_batch_dev(self._h, d_in, n_inputs, d_init or None, n_outs, d_out, n, stream))

    def fr_poseidon_chain_batch_dev(self, d_in, offsets, rate, d_out, stream=0):
        """device pointers in (offsets[m] records of 32 bytes) and out (m records; must not overlap in), ordered on `stream`; `offsets` is a HOST
        array of m + 1 entries, read before the call returns"""
        o = _offsets(offsets)                                      # held here until the call has returned
        _native.check(self._lib.bn254_fr_poseidon_chain_batch_dev(self._h, d_in, _p(o), o.size - 1, rate, d_out, stream))

    def g1_mul_base_batch_dev(self, base, d_k, d_out, n, stream=0):
        """`base` is a HOST point (12 uint64 words), read before the call returns; d_k, d_out device pointers (n records), ordered on `stream`"""
        base = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
        if base.size != G1_WORDS:
            raise ValueError(f"base must be ONE point of {G1_WORDS} uint64 words, got {base.size}")
        _native.check(self._lib.bn254_g1_mul_base_batch_dev(self._h, _p(base), d_k, d_out, n, stream))

    def g2_mul_base_batch_dev(self, base, d_k, d_out, n, stream=0):
        base = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
        if base.size != G2_WORDS:
            raise ValueError(f"base must be ONE point of {G2_WORDS} uint64 words, got {base.size}")
        _native.check(self._lib.bn254_g2_mul_base_batch_dev(self._h, _p(base), d_k, d_out, n, stream))

    def g1_msm_batch_dev(self, d_p, d_k, offsets, d_out, stream=0):
        """device pointers p, k, out (m points); `offsets` is a HOST sequence of m + 1 CSR offsets"""
        o = _offsets(offsets)
        _native.check(self._lib.bn254_g1_msm_batch_dev(self._h, d_p, d_k, _p(o), o.size - 1, d_out, stream))

    def g2_msm_batch_dev(self, d_p, d_k, offsets, d_out, stream=0):
        o = _offsets(offsets)
        _native.check(self._lib.bn254_g2_msm_batch_dev(self._h, d_p, d_k, _p(o), o.size - 1, d_out, stream))

    def g1_msm_dev(self, d_p, d_k, n, d_out, stream=0):
        """device pointers p, k (n terms) and out (ONE point), ordered on `stream`"""
        _native.check(self._lib.bn254_g1_msm_dev(self._h, d_p, d_k, n, d_out, stream))

    def g2_msm_dev(self, d_p, d_k, n, d_out, stream=0):
        _native.check(self._lib.bn254_g2_msm_dev(self._h, d_p, d_k, n, d_out, stream))

    def g1_msm_prepare_dev(self, d_p, n, window_bits=None, stream=0):
        """device pointer to n raw G1 points -> PreparedMSM; the build is ordered on `stream`"""
        h = C.c_void_p()
        _native.check(self._lib.bn254_g1_msm_prepare_dev(self._h, d_p, n, 0 if window_bits is None else int(window_bits), C.byref(h), stream))
        return PreparedMSM(self, h)

    def g2_msm_prepare_dev(self, d_p, n, window_bits=None, stream=0):
        h = C.c_void_p()
        _native.check(self._lib.bn254_g2_msm_prepare_dev(self._h, d_p, n, 0 if window_bits is None else int(window_bits), C.byref(h), stream))
        return PreparedMSM(self, h)

    def g1_msm_prepared_dev(self, prep, first, d_k, n, d_out, stream=0):
        """device pointers k (n scalars) and out (ONE point) against points [first, first + n) of `prep`, ordered on `stream`"""
        _native.check(self._lib.bn254_g1_msm_prepared_dev(self._h, prep._h, int(first), d_k, n, d_out, stream))

    def g2_msm_prepared_dev(self, prep, first, d_k, n, d_out, stream=0):
        _native.check(self._lib.bn254_g2_msm_prepared_dev(self._h, prep._h, int(first), d_k, n, d_out, stream))

    def gt_mul_dev(self, d_a, d_b, d_out, n, stream=0):
        _native.check(self._lib.bn254_gt_mul_batch_dev(self._h, d_a, d_b, d_out, n, stream))

    def gt_pow_dev(self, d_a, d_k, d_out, n, stream=0):
        _native.check(self._lib.bn254_gt_pow_batch_dev(self._h, d_a, d_k, d_out, n, stream))

    def exp_by_neg_z_dev(self, d_in, d_out, n, stream=0):
        """Fq12::exp_by_neg_z as the reference writes it (fq12.rs:229-246), any Fq12 in"""
        _native.check(self._lib.bn254_exp_by_neg_z_dev(self._h, d_in, d_out, n, stream))

    def synthetic_scalars_dev(self, seed, lo, n, which, d_out, stream=0):
        _native.check(self._lib.bn254_synthetic_scalars_dev(self._h, seed, lo, n, which, d_out, stream))

    def tile_dev(self, d_record, record_bytes, n, d_out, stream=0):
        _native.check(self._lib.bn254_tile_dev(self._h, d_record, record_bytes, n, d_out, stream))

    # ---- measurement
    def ubench_mac32(self, waves_per_simd=8, iters=1 << 15, operand_bits=32):
        """(G lane-MAC32 per second of a pure v_mad_u64_u32 stream, kernel ms) - the same-run `roofline.peak` of bench.py;
        operand_bits = 29: on the engine's own limbs (the multiplier's rate depends on its data)"""
        g = C.c_double(); ms = C.c_double()
        _native.check(self._lib.bn254_ubench_mac32_ex(self._h, int(waves_per_simd), int(iters), int(operand_bits), C.byref(g), C.byref(ms)))
        return g.value, ms.value

    def wave_ubench(self, which, iters=200):
        """microseconds per run of one program of the wave-cooperative machine on a single wave"""
        ms = C.c_double()
        _native.check(self._lib.bn254_wave_ubench(self._h, int(which), int(iters), C.byref(ms)))
        return ms.value * 1e3 / iters

    def profile(self, on=True):
        _native.check(self._lib.bn254_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        _native.check(self._lib.bn254_profile_reset(self._h))

    def kernel_stats(self, kernel):
        ms = C.c_double(); cnt = C.c_uint64()
        _native.check(self._lib.bn254_kernel_stats(self._h, kernel.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value


class PreparedG2:
    """opaque handle of bn254_g2_prepare: the native line tables of `count` G2 points in device memory (33 792 B each)"""

    def __init__(self, engine, handle):
        self._eng = engine
        self._p = handle

    @property
    def _h(self):
        if self._p is None:
            raise _native.Bn254Error("this PreparedG2 is closed")
        return self._p

    @property
    def count(self):
        return int(self._eng._lib.bn254_g2_prepared_count(self._h))

    @property
    def device_bytes(self):
        return int(self._eng._lib.bn254_g2_prepared_bytes(self._h))

    def export(self):
        """the table as (88 lines, 12 groups, 2 x count columns, 4) uint32 - for tests"""
        n = self.count
        out = np.empty((88, 12, 2 * n, 4), np.uint32)
        _native.check(self._eng._lib.bn254_g2_prepared_export(self._eng._h, self._h, _p(out), out.nbytes))
        return out

    def close(self):
        if getattr(self, "_p", None) and getattr(self._eng, "_ctx", None):
            self._eng._lib.bn254_g2_prepared_destroy(self._p)
        self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedMSM:
    """opaque handle of bn254_g{1,2}_msm_prepare: the affine multiples 2^(c w) P_i of `count` points of G1 or G2 in device memory"""

    def __init__(self, engine, handle):
        self._eng = engine
        self._p = handle

    @property
    def _h(self):
        if self._p is None:
            raise _native.Bn254Error("this PreparedMSM is closed")
        return self._p

    @property
    def count(self):
        h = self._h
        return int(self._eng._lib.bn254_msm_prepared_count(h))

    @property
    def group(self):
        h = self._h
        return int(self._eng._lib.bn254_msm_prepared_group(h))

    @property
    def window_bits(self):
        h = self._h
        return int(self._eng._lib.bn254_msm_prepared_window_bits(h))

    @property
    def windows(self):
        c = self.window_bits
        return (254 + c - 1) // c

    @property
    def device_bytes(self):
        h = self._h
        return int(self._eng._lib.bn254_msm_prepared_bytes(h))

    def export(self):
        """the table as (windows, count, group, 20) uint32: entry (w, i) is one 80-byte record per component - 9 + 9 limbs of (x, y), the
        flag word (not zero: the point at infinity), a zero word - for tests"""
        out = np.empty((self.windows, self.count, self.group, 20), np.uint32)
        _native.check(self._eng._lib.bn254_msm_prepared_export(self._eng._h, self._h, _p(out) if out.size else None, out.nbytes))
        return out

    def msm(self, scalars, first=0):
        """normalize(sum of P[first + i] * scalars[i]) -> G1 or G2; scalars: a sequence of Fr or an (n,4) uint64 array"""
        from . import api
        k = api._scalar_array(scalars)
        if self.group == 1:
            return api.G1(self._eng.g1_msm_prepared(self, k, first))
        return api.G2(self._eng.g2_msm_prepared(self, k, first))

    def close(self):
        if getattr(self, "_p", None) and getattr(self._eng, "_ctx", None):
            self._eng._lib.bn254_msm_prepared_destroy(self._p)
        self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiEngine:
    """several GPUs of one node behind ONE host process (include/bn254_hip.h: bn254_multi): contiguous shards of independent
    pairings, and the multi-pairing product with its single 384-byte-per-rank exchange (RCCL all-gather when every rank has
    its own GPU, peer copies when a device is listed twice)."""

    def __init__(self, devices, exchange="auto"):
        """exchange: "auto" (RCCL when every rank has its own GPU and RCCL loads, else peer copies), "peer", "rccl" (fail instead of
        falling back)"""
        self._lib = _native.lib()
        if self._lib.bn254_device_count() <= 0:
            raise _native.Bn254Error("no HIP device: bn_amd has no CPU fallback")
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        _native.check(self._lib.bn254_multi_create_ex(devs, len(devices), _native.EXCHANGE[exchange], C.byref(h)))
        self._m = h
        self.devices = list(devices)

    def set_option(self, name, value):
        _native.check(self._lib.bn254_multi_set_option(self._h, _native.OPTIONS[name], -1 if value is None else int(value)))

    @property
    def _h(self):
        if self._m is None:
            raise _native.Bn254Error("this MultiEngine is closed")
        return self._m

    @property
    def exchange(self):
        return {0: "peer", 1: "rccl"}[self._lib.bn254_multi_exchange_kind(self._h)]

    @property
    def numa_nodes(self):
        """per rank: the NUMA node its host thread is pinned to during a call, -1 = not pinned"""
        return [self._lib.bn254_multi_rank_numa_node(self._h, g) for g in range(len(self.devices))]

    def close(self):
        if getattr(self, "_m", None):
            self._lib.bn254_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pairing_batch(self, p, q, out=None):
        p = _arr(p, G1_WORDS); q = _arr(q, G2_WORDS); _same_len(p, q)
        if out is None:
            out = np.empty((p.shape[0], GT_WORDS), np.uint64)
        elif out.shape != (p.shape[0], GT_WORDS) or out.dtype != np.uint64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (n,48) uint64 array")
        _native.check(self._lib.bn254_pairing_batch_multi(self._h, _p(p), _p(q), _p(out), p.shape[0]))
        return out

    def pairing_product(self, p, q):
        p = _arr(p, G1_WORDS) if len(p) else np.zeros((0, G1_WORDS), np.uint64)
        q = _arr(q, G2_WORDS) if len(q) else np.zeros((0, G2_WORDS), np.uint64)
        _same_len(p, q)
        out = np.empty(GT_WORDS, np.uint64)
        _native.check(self._lib.bn254_pairing_product_multi(self._h, _p(p), _p(q), p.shape[0], _p(out)))
        return out

    def pairing_product_batch(self, p, q, offsets):
        """Engine.pairing_product_batch with the segments sharded over the ranks (segment j on the rank whose pair shard holds offsets[j])"""
        p, q, o, out = _segment_args(p, q, offsets)
        _native.check(self._lib.bn254_pairing_product_batch_multi(self._h, _p(p), _p(q), _p(o), o.size - 1, _p(out)))
        return out

    def g1_msm_batch(self, p, k, offsets):
        """Engine.g1_msm_batch with the segments sharded over the ranks (segment j on the rank whose term shard holds offsets[j])"""
        p, k, o, out = _msm_args(p, k, offsets, G1_WORDS)
        _native.check(self._lib.bn254_g1_msm_batch_multi(self._h, _p(p), _p(k), _p(o), o.size - 1, _p(out)))
        return out

    def g2_msm_batch(self, p, k, offsets):
        p, k, o, out = _msm_args(p, k, offsets, G2_WORDS)
        _native.check(self._lib.bn254_g2_msm_batch_multi(self._h, _p(p), _p(k), _p(o), o.size - 1, _p(out)))
        return out

    def g1_msm(self, p, k):
        """Engine.g1_msm with the terms sharded over the ranks; rank 0 adds the partial sums"""
        p, k, out = _msm1_args(p, k, G1_WORDS)
        _native.check(self._lib.bn254_g1_msm_multi(self._h, _p(p), _p(k), p.shape[0], _p(out)))
        return out

    def g2_msm(self, p, k):
        p, k, out = _msm1_args(p, k, G2_WORDS)
        _native.check(self._lib.bn254_g2_msm_multi(self._h, _p(p), _p(k), p.shape[0], _p(out)))
        return out

    def g2_prepare(self, q):
        """one point: prepared on every rank's GPU; n points: sharded over the ranks (then paired with exactly n points p)"""
        q = _arr(q, G2_WORDS)
        h = C.c_void_p()
        _native.check(self._lib.bn254_g2_prepare_multi(self._h, _p(q), q.shape[0], C.byref(h)))
        return MultiPreparedG2(self, h)

    def pairing_prepared_native_batch(self, p, prepared, out=None):
        p = _arr(p, G1_WORDS)
        if out is None:
            out = np.empty((p.shape[0], GT_WORDS), np.uint64)
        _native.check(self._lib.bn254_pairing_prepared_native_batch_multi(self._h, _p(p), prepared._h, _p(out), p.shape[0]))
        return out

    def pairing_product_prepared_native(self, p, prepared):
        """the multi-pairing over the prepared points, sharded: one 384-byte exchange, ONE final exponentiation"""
        p = _arr(p, G1_WORDS) if len(p) else np.zeros((0, G1_WORDS), np.uint64)
        out = np.empty(GT_WORDS, np.uint64)
        _native.check(self._lib.bn254_pairing_product_prepared_native_multi(self._h, _p(p), prepared._h, p.shape[0], _p(out)))
        return out


class MultiPreparedG2:
    """handle of bn254_g2_prepare_multi: per-rank native tables"""

    def __init__(self, multi, handle):
        self._m = multi
        self._p = handle

    @property
    def _h(self):
        if self._p is None:
            raise _native.Bn254Error("this MultiPreparedG2 is closed")
        return self._p

    @property
    def count(self):
        return int(self._m._lib.bn254_multi_prepared_count(self._h))

    def close(self):
        if getattr(self, "_p", None) and getattr(self._m, "_m", None):
            self._m._lib.bn254_multi_prepared_destroy(self._p)
        self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
