"""Host-side mirror of the reference crate's public API (src/lib.rs): Fr, G1, G2, Gt, pairing - plus the batch entry points
the GPU engine adds (pairing_batch / pairing_product; the reference only has the fold of shootout/main.rs:11-16).

Values are immutable wrappers around the reference's memory images (Montgomery u64 limbs).  Group and pairing arithmetic
runs on the GPU through the C ABI; the operators of a single scalar Fr (lib.rs:15-53, "host-side convenience" in SURVEY.md) are plain
Python integer arithmetic, ARRAYS of scalars have the batch functions fr_*_batch, which run on the GPU like everything else.  No CPU
fallback for anything that touches a curve point or a Gt."""
import numpy as np

from .engine import Engine, G1_WORDS, G2_WORDS, GT_WORDS

_U = 4965661367192848881
Q_MOD = 36 * _U**4 + 36 * _U**3 + 24 * _U**2 + 6 * _U + 1
R_MOD = 36 * _U**4 + 36 * _U**3 + 18 * _U**2 + 6 * _U + 1
_MONT = 1 << 256
_M64 = (1 << 64) - 1

_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


def _limbs(v):
    return np.array([(v >> (64 * i)) & _M64 for i in range(4)], np.uint64)


def _mont(v, mod):
    return _limbs(v % mod * _MONT % mod)


class Fr:
    """scalar field element (lib.rs:15-53); `limbs` is the reference's Montgomery image"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = int(v) % R_MOD

    @staticmethod
    def zero(): return Fr(0)
    @staticmethod
    def one(): return Fr(1)
    @staticmethod
    def from_str(s):                      # lib.rs:24 -> fields/fp.rs:39-59: ASCII decimal digits only; "" is zero; anything else None
        if not all(c in "0123456789" for c in s):
            return None
        return Fr(int(s)) if s else Fr(0)
    @staticmethod
    def random(rng):                      # uniform mod r from 512 bits, like arith.rs:195-198
        return Fr(int.from_bytes(rng.bytes(64), "little"))
    @staticmethod
    def interpret(buf):                   # lib.rs:27-29 -> arith.rs:90-97: 64 bytes as a big-endian 512-bit integer, mod r
        buf = bytes(buf)
        if len(buf) != 64:
            raise ValueError("Fr.interpret takes exactly 64 bytes")
        return Fr(int.from_bytes(buf, "big"))
    @staticmethod
    def root_of_unity(log_n):             # w_n for n = 2^log_n: w_28^(2^(28 - log_n)), w_28 = 5^((r-1)/2^28) - ark-bn254's root; the domains nest
        if not 0 <= log_n <= 28:
            raise ValueError("r - 1 is divisible by 2^28 and no higher power of two")
        return Fr(pow(5, (R_MOD - 1) >> log_n, R_MOD))
    @staticmethod
    def from_limbs(l):
        return Fr(sum(int(x) << (64 * i) for i, x in enumerate(l)) * pow(_MONT, -1, R_MOD))
    @property
    def limbs(self): return _mont(self.v, R_MOD)
    def inverse(self): return None if self.v == 0 else Fr(pow(self.v, -1, R_MOD))
    def sqrt(self):
        """the square root whose integer is not above (r - 1) / 2, None for a non-residue (on the GPU: fr_sqrt_batch)"""
        return fr_sqrt_batch([self])[0]
    def is_zero(self): return self.v == 0
    def pow(self, e): return Fr(pow(self.v, e.v, R_MOD))
    def __add__(self, o): return Fr(self.v + o.v)
    def __sub__(self, o): return Fr(self.v - o.v)
    def __mul__(self, o): return Fr(self.v * o.v)
    def __neg__(self): return Fr(-self.v)
    def __eq__(self, o): return isinstance(o, Fr) and self.v == o.v
    def __hash__(self): return hash(self.v)
    def __repr__(self): return f"Fr({self.v})"


def _one_fq(): return _mont(1, Q_MOD)


class _Point:
    WORDS = 0
    __slots__ = ("limbs",)

    def __init__(self, limbs):
        self.limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(self.WORDS)

    def is_zero(self):                    # groups/mod.rs:224-226: z == 0
        return not self.limbs[2 * self.WORDS // 3:].any()

    def __eq__(self, o):                  # projective equality (groups/mod.rs:83-109): one comparison on the GPU, nothing normalized
        return type(o) is type(self) and bool(self._eq(default_engine())(self.limbs, o.limbs)[0])

    def normalize(self):                  # lib.rs:88-95 / 131-138: (x/z^2, y/z^3, 1) on the GPU
        return type(self)(self._normalize(default_engine())(self.limbs)[0])


class G1(_Point):
    WORDS = G1_WORDS

    @staticmethod
    def one():                            # groups/mod.rs:355-361: (1, 2, 1)
        return G1(np.concatenate([_one_fq(), _mont(2, Q_MOD), _one_fq()]))
    @staticmethod
    def zero():                           # groups/mod.rs:208-214: (0, 1, 0)
        return G1(np.concatenate([np.zeros(4, np.uint64), _one_fq(), np.zeros(4, np.uint64)]))
    @staticmethod
    def random(rng): return G1.one() * Fr.random(rng)        # groups/mod.rs:220-222
    _eq = staticmethod(lambda e: e.g1_eq)
    _normalize = staticmethod(lambda e: e.g1_normalize)
    def __mul__(self, k):                 # lib.rs:116-120 (result returned normalized)
        return G1(default_engine().g1_mul_batch(self.limbs, k.limbs)[0])
    def __add__(self, o):                 # lib.rs:103-106 (the reference's Jacobian limbs)
        return G1(default_engine().g1_add_batch(self.limbs, o.limbs)[0])
    def __sub__(self, o):                 # lib.rs:108-111
        return G1(default_engine().g1_add_batch(self.limbs, o.limbs, negate_b=True)[0])
    def __neg__(self):                    # lib.rs:113-114
        return G1(default_engine().g1_add_batch(G1.zero().limbs, self.limbs, negate_b=True)[0])
    @staticmethod
    def msm(points, scalars):             # normalize(sum points[i] * scalars[i]) in one call
        return g1_msm(points, scalars)
    def mul_base(self, scalars):          # [self * k for k in scalars] over ONE cached table of self
        return g1_mul_base(self, scalars)
    @staticmethod
    def hash(msg, dst):                   # hash_to_curve of RFC 9380 (SvdW, SHA-256 XMD) under the tag dst
        return g1_hash_to_curve_batch([msg], dst)[0]
    def is_valid(self):                   # the limbs are below q and on the curve (or z == 0): one check on the GPU
        return int(g1_validate_batch([self])[0]) == 0
    def to_compressed(self, format="ark"):    # 32 bytes: x and the sign of y
        return g1_compress_batch([self], format)[0]
    @staticmethod
    def from_compressed(b, format="ark"):     # DecodeError for a record that is rejected
        return _one_decompressed(g1_decompress_batch, b, format)


_G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
            11559732032986387107991004021392285783925812861821192530917403151452391805634),
           (8495653923123431417604973247489272438418190587263600148770280649306958101930,
            4082367875863433681332203403145435568316851327593401208105741076214120093531))


class G2(_Point):
    WORDS = G2_WORDS

    @staticmethod
    def one():                            # groups/mod.rs:377-390
        (x0, x1), (y0, y1) = _G2_GEN
        return G2(np.concatenate([_mont(x0, Q_MOD), _mont(x1, Q_MOD), _mont(y0, Q_MOD), _mont(y1, Q_MOD), _one_fq(), np.zeros(4, np.uint64)]))
    @staticmethod
    def zero():
        z = np.zeros(8, np.uint64)
        return G2(np.concatenate([z, _one_fq(), np.zeros(4, np.uint64), z]))
    @staticmethod
    def random(rng): return G2.one() * Fr.random(rng)
    _eq = staticmethod(lambda e: e.g2_eq)
    _normalize = staticmethod(lambda e: e.g2_normalize)
    def __mul__(self, k):
        return G2(default_engine().g2_mul_batch(self.limbs, k.limbs)[0])
    def __add__(self, o):                 # lib.rs:146-149
        return G2(default_engine().g2_add_batch(self.limbs, o.limbs)[0])
    def __sub__(self, o):
        return G2(default_engine().g2_add_batch(self.limbs, o.limbs, negate_b=True)[0])
    def __neg__(self):
        return G2(default_engine().g2_add_batch(G2.zero().limbs, self.limbs, negate_b=True)[0])
    @staticmethod
    def msm(points, scalars):
        return g2_msm(points, scalars)
    def mul_base(self, scalars):
        return g2_mul_base(self, scalars)
    @staticmethod
    def hash(msg, dst):                   # hash_to_curve of RFC 9380 over Fq2 (SvdW, SHA-256 XMD) and the psi-based cofactor clearing
        return g2_hash_to_curve_batch([msg], dst)[0]
    def is_valid(self):                   # below q, on the twist AND in the order-r subgroup (or z == 0): one check on the GPU
        return int(g2_validate_batch([self])[0]) == 0
    def to_compressed(self, format="ark"):    # 64 bytes
        return g2_compress_batch([self], format)[0]
    @staticmethod
    def from_compressed(b, format="ark"):
        return _one_decompressed(g2_decompress_batch, b, format)


class Gt:
    """target group element (lib.rs:165-179)"""
    __slots__ = ("limbs",)

    def __init__(self, limbs):
        self.limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(GT_WORDS)

    @staticmethod
    def one():
        l = np.zeros(GT_WORDS, np.uint64); l[:4] = _one_fq()
        return Gt(l)
    def __mul__(self, o):                 # lib.rs:175-179
        return Gt(default_engine().gt_mul_batch(self.limbs, o.limbs)[0])
    def pow(self, k):                     # lib.rs:171
        return Gt(default_engine().gt_pow_batch(self.limbs, k.limbs)[0])
    def inverse(self):                    # lib.rs:172
        return Gt(default_engine().gt_inverse_batch(self.limbs)[0])
    def __eq__(self, o): return isinstance(o, Gt) and np.array_equal(self.limbs, o.limbs)   # canonical limbs: memcmp
    def __repr__(self): return "Gt(%s...)" % hex(int(self.limbs[0]))


def pairing(p, q):
    """lib.rs:181-183"""
    return Gt(default_engine().pairing_batch(p.limbs, q.limbs)[0])


def pairing_batch(ps, qs, engine=None):
    """out[i] = pairing(ps[i], qs[i]); ps/qs: sequences of G1/G2 or (n,12)/(n,24) uint64 arrays"""
    e = engine or default_engine()
    P = np.stack([p.limbs for p in ps]) if not isinstance(ps, np.ndarray) else ps
    Q = np.stack([q.limbs for q in qs]) if not isinstance(qs, np.ndarray) else qs
    return e.pairing_batch(P, Q)


def pairing_product(ps, qs, engine=None):
    """fold(Gt::one(), acc * pairing(p, q)) (shootout/main.rs:11-16) with ONE final exponentiation"""
    e = engine or default_engine()
    P = np.stack([p.limbs for p in ps]) if not isinstance(ps, np.ndarray) else ps
    Q = np.stack([q.limbs for q in qs]) if not isinstance(qs, np.ndarray) else qs
    return Gt(e.pairing_product(P, Q))


def _segment_arrays(segments, qs, offsets):
    if offsets is not None:                   # (n,12) / (n,24) arrays + CSR offsets
        return np.asarray(segments, np.uint64).reshape(-1, G1_WORDS), np.asarray(qs, np.uint64).reshape(-1, G2_WORDS), np.asarray(offsets, np.uint64)
    if qs is not None:
        raise ValueError("qs is only taken together with offsets")
    segments = [list(s) for s in segments]
    offs = np.zeros(len(segments) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in segments], dtype=np.uint64) if segments else []
    pairs = [pq for s in segments for pq in s]
    P = np.stack([p.limbs for p, _ in pairs]) if pairs else np.zeros((0, G1_WORDS), np.uint64)
    Q = np.stack([q.limbs for _, q in pairs]) if pairs else np.zeros((0, G2_WORDS), np.uint64)
    return P, Q, offs


def _product_batch_limbs(segments, qs, offsets, engine):
    P, Q, offs = _segment_arrays(segments, qs, offsets)
    return (engine or default_engine()).pairing_product_batch(P, Q, offs)


def pairing_product_batch(segments, qs=None, offsets=None, engine=None):
    """[fold(Gt::one(), acc * pairing(p, q)) over the pairs of each segment] (shootout/main.rs:11-16 per segment) with ONE final
    exponentiation per segment.  segments: a sequence of sequences of (G1, G2) - an empty one gives Gt::one() -, or (n,12) / (n,24) uint64
    arrays as `segments` / `qs` plus CSR `offsets` (m + 1 entries)."""
    return [Gt(r) for r in _product_batch_limbs(segments, qs, offsets, engine)]


def pairing_check_batch(segments, qs=None, offsets=None, engine=None):
    """numpy bool array: product of segment j == Gt::one(), compared as canonical limbs - the predicate of a Groth16 / EIP-197-style check"""
    return (_product_batch_limbs(segments, qs, offsets, engine) == Gt.one().limbs).all(axis=1)


def _msm_arrays(group, segments, ks, offsets):
    if offsets is not None:                   # (n, WORDS) points and (n,4) scalars + CSR offsets
        return np.asarray(segments, np.uint64).reshape(-1, group.WORDS), np.asarray(ks, np.uint64).reshape(-1, 4), np.asarray(offsets, np.uint64)
    if ks is not None:
        raise ValueError("ks is only taken together with offsets")
    segments = [list(s) for s in segments]
    offs = np.zeros(len(segments) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in segments], dtype=np.uint64) if segments else []
    terms = [pk for s in segments for pk in s]
    P = np.stack([p.limbs for p, _ in terms]) if terms else np.zeros((0, group.WORDS), np.uint64)
    K = np.stack([k.limbs for _, k in terms]) if terms else np.zeros((0, 4), np.uint64)
    return P, K, offs


def g1_msm_batch(segments, ks=None, offsets=None, engine=None):
    """[normalize(sum of p * k over the terms of each segment)] (lib.rs:103-120,88-95 folded per segment): many independent multi-scalar
    multiplications in one call, ONE inversion per segment.  segments: a sequence of sequences of (G1, Fr) - an empty one gives G1.zero() -,
    or (n,12) / (n,4) uint64 arrays as `segments` / `ks` plus CSR `offsets` (m + 1 entries)."""
    P, K, offs = _msm_arrays(G1, segments, ks, offsets)
    return [G1(r) for r in (engine or default_engine()).g1_msm_batch(P, K, offs)]


def g2_msm_batch(segments, ks=None, offsets=None, engine=None):
    """the same over G2: (G2, Fr) terms, or (n,24) / (n,4) arrays plus offsets"""
    P, K, offs = _msm_arrays(G2, segments, ks, offsets)
    return [G2(r) for r in (engine or default_engine()).g2_msm_batch(P, K, offs)]


def _msm1_arrays(group, points, scalars):
    if isinstance(points, np.ndarray) or isinstance(scalars, np.ndarray):          # (n, WORDS) points and (n, 4) scalars
        return np.asarray(points, np.uint64).reshape(-1, group.WORDS), np.asarray(scalars, np.uint64).reshape(-1, 4)
    points, scalars = list(points), list(scalars)
    if len(points) != len(scalars):
        raise ValueError("as many scalars as points")
    P = np.stack([p.limbs for p in points]) if points else np.zeros((0, group.WORDS), np.uint64)
    K = np.stack([k.limbs for k in scalars]) if scalars else np.zeros((0, 4), np.uint64)
    return P, K


def g1_msm(points, scalars, engine=None):
    """normalize(sum of points[i] * scalars[i]): ONE large multi-scalar multiplication (bucket method from the option msm_bucket_min terms
    on; the same bytes as the one-segment g1_msm_batch).  Sequences of G1 / Fr, or (n,12) / (n,4) uint64 arrays; no terms give G1.zero()."""
    P, K = _msm1_arrays(G1, points, scalars)
    return G1((engine or default_engine()).g1_msm(P, K))


def g2_msm(points, scalars, engine=None):
    """the same over G2: sequences of G2 / Fr, or (n,24) / (n,4) arrays"""
    P, K = _msm1_arrays(G2, points, scalars)
    return G2((engine or default_engine()).g2_msm(P, K))


def _point_array(group, points):
    if isinstance(points, np.ndarray):
        return np.asarray(points, np.uint64).reshape(-1, group.WORDS)
    points = list(points)
    return np.stack([p.limbs for p in points]) if points else np.zeros((0, group.WORDS), np.uint64)


def g1_msm_prepare(points, window_bits=None, engine=None):
    """PreparedMSM of the G1 points: prepare once what g1_msm redoes per call against the same points (a proving key, an SRS), then
    `.msm(scalars, first=0)` == g1_msm(points[first:first + len(scalars)], scalars), the same bytes.  points: a sequence of G1 or an (n,12)
    uint64 array, raw (any z); window_bits: None for the default of the size, or 3 .. 16."""
    return (engine or default_engine()).g1_msm_prepare(_point_array(G1, points), window_bits)


def g2_msm_prepare(points, window_bits=None, engine=None):
    """the same over G2: a sequence of G2 or an (n,24) uint64 array"""
    return (engine or default_engine()).g2_msm_prepare(_point_array(G2, points), window_bits)


def _scalar_array(scalars):
    if isinstance(scalars, np.ndarray):
        return np.asarray(scalars, np.uint64).reshape(-1, 4)
    scalars = list(scalars)
    return np.stack([k.limbs for k in scalars]) if scalars else np.zeros((0, 4), np.uint64)


def g1_mul_base(base, scalars, engine=None):
    """[base * k for k in scalars], normalized like `base * k`: fixed-base scalar multiplication - key / SRS generation, many scalars against
    one generator.  The engine builds a table of multiples of `base` once and keeps it (four bases per group); every product is then at most
    22 mixed additions.  base: a G1 (or 12 uint64 words); scalars: a sequence of Fr or an (n,4) uint64 array."""
    b = base.limbs if isinstance(base, G1) else base
    return [G1(r) for r in (engine or default_engine()).g1_mul_base_batch(b, _scalar_array(scalars))]


def g2_mul_base(base, scalars, engine=None):
    """the same over G2: base a G2 (or 24 uint64 words)"""
    b = base.limbs if isinstance(base, G2) else base
    return [G2(r) for r in (engine or default_engine()).g2_mul_base_batch(b, _scalar_array(scalars))]


def _point_array(cls, points):
    if isinstance(points, np.ndarray):
        return np.asarray(points, np.uint64).reshape(-1, cls.WORDS)
    points = list(points)
    return np.stack([p.limbs for p in points]) if points else np.zeros((0, cls.WORDS), np.uint64)


DECODE_STATUS = {0: "ok", 1: "a coordinate is not below the field modulus", 2: "an Fq2 coordinate is not below the squared modulus", 3: "invalid flags or leading byte",
                 4: "no point of the curve has this x", 5: "the point is not in the subgroup"}


class DecodeError(ValueError):
    """a record the decoder rejected; .status is the decoder's number (DECODE_STATUS)"""
    def __init__(self, status):
        self.status = int(status)
        super().__init__(f"decode status {self.status}: {DECODE_STATUS.get(self.status, 'unknown')}")


def _records(b, size):
    """bytes (one record or many), a sequence of bytes objects or a uint8 array -> (n, size) uint8"""
    if isinstance(b, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(b), np.uint8)
    elif isinstance(b, np.ndarray):
        a = np.ascontiguousarray(b, np.uint8).reshape(-1)
    else:
        a = np.frombuffer(b"".join(bytes(r) for r in b), np.uint8)
    if a.size % size:
        raise ValueError(f"{a.size} bytes are not whole records of {size}")
    return a.reshape(-1, size)


def _one_decompressed(fn, b, format):
    points, status = fn(b, format)
    if len(points) != 1:
        raise ValueError(f"one record is expected, got {len(points)}")
    if status[0]:
        raise DecodeError(status[0])
    return points[0]


def g1_compress_batch(points, format="ark", engine=None):
    """[32 bytes per point]: x and the sign of y in the layout `format` ("ark": little endian, flags in the last byte; "gnark": big endian,
    flags in the first).  points: a sequence of G1 (any Jacobian form) or an (n,12) uint64 array."""
    return [r.tobytes() for r in (engine or default_engine()).g1_compress_batch(_point_array(G1, points), format)]


def g2_compress_batch(points, format="ark", engine=None):
    """the same over G2: 64 bytes per point"""
    return [r.tobytes() for r in (engine or default_engine()).g2_compress_batch(_point_array(G2, points), format)]


def g1_decompress_batch(b, format="ark", engine=None):
    """(points, status): b is bytes of whole 32-byte records, a sequence of records or a uint8 array.  status[i] (int32): 0 ok, 3 invalid
    flags, 1 x not below q, 4 no point has this x; a rejected record is G1.zero()."""
    rec = _records(b, 32)
    p, st = (engine or default_engine()).g1_decompress_batch(rec, format)
    return [G1(r) for r in p], st


def g2_decompress_batch(b, format="ark", engine=None):
    """the same over G2: 64-byte records; status 5 for a point of the twist outside the subgroup"""
    rec = _records(b, 64)
    p, st = (engine or default_engine()).g2_decompress_batch(rec, format)
    return [G2(r) for r in p], st


def g1_map_to_curve_batch(us, engine=None):
    """[map_to_curve(u) for u in us], the Shallue-van de Woestijne map of RFC 9380: never the point at infinity.  us: a sequence of integers
    below 2^384 (taken mod q) or an (n,48) uint8 array of big-endian integers."""
    if not isinstance(us, np.ndarray):
        us = list(us)
        us = np.stack([np.frombuffer(int(u).to_bytes(48, "big"), np.uint8) for u in us]) if us else np.zeros((0, 48), np.uint8)
    return [G1(r) for r in (engine or default_engine()).g1_map_to_curve_batch(us)]


def _hash_to_curve_limbs(msgs, dst, engine):
    """(n,12) uint64: messages of one length take the device's SHA-256, mixed lengths are expanded with hashlib and take the uniform call"""
    from . import hash_to_curve as h2c
    dst = h2c.h2c_dst(dst)
    if not isinstance(msgs, np.ndarray):
        msgs = [bytes(m) for m in msgs]
    e = engine or default_engine()
    arr = h2c.message_array(msgs)
    if arr is not None:
        return e.g1_hash_to_curve_batch(arr, dst)
    return e.g1_hash_to_curve_uniform_batch(h2c.uniform_bytes(msgs, dst))


def g1_hash_to_curve_batch(msgs, dst, engine=None):
    """[hash_to_curve(m) for m in msgs] (RFC 9380, random-oracle variant: SHA-256 XMD, two SvdW maps, one sum) under the domain separation
    tag dst (1 .. 255 bytes).  msgs: a sequence of bytes or an (n, msg_len) uint8 array."""
    return [G1(r) for r in _hash_to_curve_limbs(msgs, dst, engine)]


def g2_map_to_curve_batch(us, engine=None):
    """[map_to_curve(u) for u in us] over Fq2: points (x, y, 1) of the twist, never at infinity and NOT in G2 (g2_clear_cofactor_batch takes
    them there).  us: a sequence of (c0, c1) pairs of integers below 2^384 (taken mod q) or an (n,96) uint8 array, c0 then c1, big endian."""
    if not isinstance(us, np.ndarray):
        us = list(us)
        us = np.stack([np.frombuffer(int(c0).to_bytes(48, "big") + int(c1).to_bytes(48, "big"), np.uint8) for c0, c1 in us]) if us else np.zeros((0, 96), np.uint8)
    return [G2(r) for r in (engine or default_engine()).g2_map_to_curve_batch(us)]


def g2_clear_cofactor_batch(points, engine=None):
    """[clear(p) for p in points], clear(P) = [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P), normalised: a point of G2 for every point of the twist
    (being on the curve is the caller's responsibility).  Not [2q - r]P; on G2 it is a fixed scalar.  Neither the constants nor the outputs are checked against gnark-crypto or any other
    library."""
    return [G2(r) for r in (engine or default_engine()).g2_clear_cofactor_batch(_point_array(G2, points))]


def _g2_hash_to_curve_limbs(msgs, dst, engine):
    """(n,24) uint64: messages of one length take the device's SHA-256, mixed lengths are expanded with hashlib and take the uniform call"""
    from . import hash_to_curve as h2c
    dst = h2c.h2c_dst(dst)
    if not isinstance(msgs, np.ndarray):
        msgs = [bytes(m) for m in msgs]
    e = engine or default_engine()
    arr = h2c.message_array(msgs)
    if arr is not None:
        return e.g2_hash_to_curve_batch(arr, dst)
    return e.g2_hash_to_curve_uniform_batch(h2c.uniform_bytes_g2(msgs, dst))


def g2_hash_to_curve_batch(msgs, dst, engine=None):
    """[hash_to_curve(m) for m in msgs] into G2 (RFC 9380, random-oracle variant over Fq2: SHA-256 XMD to 192 bytes, two SvdW maps, one sum,
    the cofactor clearing) under the domain separation tag dst (1 .. 255 bytes).  msgs: a sequence of bytes or an (n, msg_len) uint8 array."""
    return [G2(r) for r in _g2_hash_to_curve_limbs(msgs, dst, engine)]


def g1_validate_batch(points, engine=None):
    """int32 status per point, for raw limbs from anywhere: 0 valid (the point at infinity, z == 0, included), 1 a coordinate is not below q,
    4 not on the curve y^2 = x^3 + 3 (in Jacobian form, any z).  G1 has cofactor 1.  points: a sequence of G1 or an (n,12) uint64 array."""
    return (engine or default_engine()).g1_validate_batch(_point_array(G1, points))


def g2_validate_batch(points, engine=None):
    """the same over G2, and 5 for a point of the twist outside the order-r subgroup: the twist has the 254-bit cofactor 2q - r, and every
    pairing, multiplication and verifier of this package trusts its G2 inputs to be in the subgroup.  The test is the endomorphism subgroup
    test [u + 1]P + psi([u]P) + psi^2([u]P) == psi^3([2u]P), exact on the twist."""
    return (engine or default_engine()).g2_validate_batch(_point_array(G2, points))


def _valid_rows(engine, g1, g2, keys):
    """bool per row of a signature batch (bn_amd.bls, bn_amd.bls_minpk with validate=True): the G1 and the G2 point of the row are valid - one
    validation call per group - and the public key (`keys`: whichever of the two arrays holds them) is not the point at infinity"""
    ok = (np.asarray(engine.g1_validate_batch(g1)) == 0) & (np.asarray(engine.g2_validate_batch(g2)) == 0)
    return ok & keys[:, 2 * keys.shape[1] // 3:].any(axis=1)


def g1_normalize_batch(points, engine=None):
    """[p.normalize() for p in points] in one call: (x/z^2, y/z^3, 1), infinity as G1.zero(); neighbouring points share one field
    inversion.  points: a sequence of G1 or an (n,12) uint64 array."""
    return [G1(r) for r in (engine or default_engine()).g1_normalize(_point_array(G1, points))]


def g2_normalize_batch(points, engine=None):
    """the same over G2: a sequence of G2 or an (n,24) uint64 array"""
    return [G2(r) for r in (engine or default_engine()).g2_normalize(_point_array(G2, points))]


def g1_eq_batch(a, b, engine=None):
    """[x == y for x, y in zip(a, b)] in one call, as group elements (any Jacobian representations; nothing is normalized) -> list of bool"""
    return [bool(r) for r in (engine or default_engine()).g1_eq(_point_array(G1, a), _point_array(G1, b))]


def g2_eq_batch(a, b, engine=None):
    """the same over G2"""
    return [bool(r) for r in (engine or default_engine()).g2_eq(_point_array(G2, a), _point_array(G2, b))]


def fr_add_batch(a, b, engine=None):
    """[x + y for x, y in zip(a, b)] on the GPU in one call.  Here and below: sequences of Fr, or (n,4) uint64 arrays of Montgomery limbs."""
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_add_batch(_scalar_array(a), _scalar_array(b))]


def fr_sub_batch(a, b, engine=None):
    """[x - y for x, y in zip(a, b)]"""
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_add_batch(_scalar_array(a), _scalar_array(b), negate_b=True)]


def fr_neg_batch(a, engine=None):
    """[-x for x in a]: 0 - x (lib.rs:43-47)"""
    A = _scalar_array(a)
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_add_batch(np.zeros_like(A), A, negate_b=True)]


def fr_mul_batch(a, b, engine=None):
    """[x * y for x, y in zip(a, b)]"""
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_mul_batch(_scalar_array(a), _scalar_array(b))]


def fr_pow_batch(a, e, engine=None):
    """[x.pow(y) for x, y in zip(a, e)] (lib.rs:23); 0^0 is one"""
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_pow_batch(_scalar_array(a), _scalar_array(e))]


def fr_inverse_batch(a, engine=None):
    """[x.inverse() for x in a] (lib.rs:25): a list of Fr, None where x is zero; neighbouring elements share one exponentiation"""
    out, ok = (engine or default_engine()).fr_inverse_batch(_scalar_array(a))
    return [Fr.from_limbs(r) if k else None for r, k in zip(out, ok)]


def fr_sqrt_batch(a, engine=None):
    """[x.sqrt() for x in a]: a list of Fr, None where x is a non-residue.  Of the two roots the one whose canonical integer is not above
    (r - 1) / 2 comes out; 0 has the root 0.  No counterpart in the reference crate"""
    out, ok = (engine or default_engine()).fr_sqrt_batch(_scalar_array(a))
    return [Fr.from_limbs(r) if k else None for r, k in zip(out, ok)]


def fr_interpret_batch(bufs, engine=None):
    """[Fr.interpret(b) for b in bufs] (lib.rs:27-29): a sequence of 64-byte buffers, or an (n,64) uint8 array"""
    if not isinstance(bufs, np.ndarray):
        bufs = [bytes(b) for b in bufs]
        if any(len(b) != 64 for b in bufs):
            raise ValueError("Fr.interpret takes exactly 64 bytes")
        bufs = np.frombuffer(b"".join(bufs), np.uint8).reshape(-1, 64)
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_interpret_batch(bufs)]


def fr_dot_batch(coeff, x, offsets, index=None, engine=None):
    """[sum(coeff[t] * x[index[t]] for t in range(offsets[j], offsets[j + 1])) for j in range(m)] -> list of Fr: a sparse matrix in CSR form
    (offsets, index, coeff) times the vector x, all rows in ONE call.  index None: x[t], a plain segmented inner product.  coeff and x are
    sequences of Fr or (n,4) uint64 arrays; an empty segment gives zero.  ValueError for offsets that do not start at 0, decrease or end
    elsewhere than at len(coeff), for an index of another length or with an entry >= len(x), and for len(x) != len(coeff) without an index."""
    from .engine import _dot_args
    args = _dot_args(_scalar_array(coeff), _scalar_array(x), offsets, index)
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_dot_batch(args[0], args[1], args[2], args[3])]


def fr_scan_batch(a, b, offsets, init=None, reverse=False, exclusive=False, a_per_segment=False, engine=None):
    """The first-order linear recurrence over every segment, all segments in ONE call -> list of len(terms) Fr:
        out[t] = a[t] * prev + b[t],   prev = out[t-1], or init[j] at the first term of segment j = [offsets[j], offsets[j+1])
    a None: every a[t] is one (segmented prefix sums); b None: every b[t] is zero (segmented prefix products); init None: zero with b, one
    without.  reverse: each segment from its last term to its first; exclusive: out[t] = prev (the first term gets init[j], the total is
    not written); a_per_segment: a holds one factor per segment (powers, Horner's rule).  a, b, init are sequences of Fr or (n,4) uint64
    arrays.  ValueError, before any device call, naming the operand: a and b both None, offsets that do not start at 0 or decrease, a, b or
    init of the wrong length."""
    from .engine import _scan_args
    rows = lambda v: None if v is None else _scalar_array(v)
    args = _scan_args(rows(a), rows(b), offsets, rows(init), a_per_segment)
    out = (engine or default_engine()).fr_scan_batch(args[0], args[1], args[2], args[3], reverse=reverse, exclusive=exclusive, a_per_segment=a_per_segment)
    return [Fr.from_limbs(r) for r in out]


def fr_mle_eq(z, engine=None):
    """The table of eq(z, .) over the hypercube of nv = len(z) variables -> list of 2^nv Fr: out[i] = prod_j (z[j] if bit j of i else 1 - z[j]), the
    multilinear polynomial that is one at the point z of the hypercube and zero at every other.  z: a sequence of Fr or an (nv,4) uint64
    array; no variables give [Fr.one()].  ValueError for more than 30 variables."""
    from .engine import _mle_eq_args
    Z = _mle_eq_args(_scalar_array(z))
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_mle_eq(Z)]


def fr_mle_fold(a, r, engine=None):
    """[a[i] + r * (a[i + len(a) // 2] - a[i]) for i in range(len(a) // 2)] -> list of Fr: the multilinear table a with its MOST significant
    variable bound to r.  a: a sequence of Fr or an (n,4) uint64 array, n even; r: an Fr.  ValueError for an odd length."""
    from .engine import _mle_fold_args
    A, rr = _mle_fold_args(_scalar_array(a), r)
    return [Fr.from_limbs(x) for x in (engine or default_engine()).fr_mle_fold(A, rr)]


def fr_sumcheck_round(tables, groups, degree=None, engine=None):
    """The round polynomial of a sumcheck over sum_c coeff_c * prod_{j in group c} T_j, at t = 0 .. degree -> list of degree + 1 Fr:
        out[t] = sum over i < n / 2 and the groups c of coeff_c * prod_j (T_j[i] + t * (T_j[i + n / 2] - T_j[i]))
    - the most significant variable is the one the round binds, and out[0] + out[1] is the sum over all n indices.  tables: a sequence of k
    tables of n Fr each, or an (n, k, 4) uint64 array with table j at index i in [i, j]; groups: a list of (coeff, [table numbers]), a table
    may repeat within a group; degree: None for the longest group.  ValueError, before any device call, naming the operand: an odd n or
    n < 2, more than 16 tables or groups, a group that is empty, longer than the degree or names a table that is not there."""
    from .engine import _sumcheck_args
    if not isinstance(tables, np.ndarray):
        cols = [_scalar_array(t) for t in tables]
        if len({c.shape[0] for c in cols}) > 1:
            raise ValueError(f"tables differ in length: {[c.shape[0] for c in cols]}")
        tables = np.stack(cols, axis=1) if cols else np.zeros((0, 0, 4), np.uint64)
    t, _, _, _, degree = _sumcheck_args(tables, groups, degree)
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_sumcheck_round(t, groups, degree)]


def fr_sumcheck_fold_round(tables, r, groups, degree=None, engine=None):
    """fr_mle_fold of every table by r, then fr_sumcheck_round of the folded tables, in ONE pass over them -> (folded, out): folded is the
    (n / 2, k, 4) uint64 array of the tables with their most significant variable bound to r, out the list of degree + 1 Fr of the round
    polynomial over the folded tables - what a sumcheck prover does between two challenges.  tables, groups and degree as in
    fr_sumcheck_round; r: an Fr.  ValueError, before any device call, for what fr_sumcheck_round rejects and for an n that is no multiple of 4."""
    from .engine import _fold_round_rows, _fr_point, _sumcheck_args
    if not isinstance(tables, np.ndarray):
        cols = [_scalar_array(t) for t in tables]
        if len({c.shape[0] for c in cols}) > 1:
            raise ValueError(f"tables differ in length: {[c.shape[0] for c in cols]}")
        tables = np.stack(cols, axis=1) if cols else np.zeros((0, 0, 4), np.uint64)
    t, _, _, _, degree = _sumcheck_args(tables, groups, degree)
    _fold_round_rows(t.shape[0])
    rr = _fr_point(r, "r")
    folded, out = (engine or default_engine()).fr_sumcheck_fold_round(t, rr, groups, degree)
    return folded, [Fr.from_limbs(x) for x in out]


def fr_mle_quotients(a, z, engine=None):
    """The quotients of the multilinear table a at the point z -> list of len(a) Fr in heap order: out[0] = f(z) and out[2^j + i] = q_j[i] for
    j < nv, i < 2^j, with f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1}): from t = a, for j = nv - 1 down to 0, q_j[i] = t[i + 2^j] - t[i] and
    t[i] += z[j] * q_j[i].  a: a sequence of 2^nv Fr or an (n,4) uint64 array; z: nv Fr.  ValueError unless len(a) == 2^len(z) <= 2^30."""
    from .engine import _mle_quotients_args
    A, Z = _mle_quotients_args(_scalar_array(a), _scalar_array(z))
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_mle_quotients(A, Z)]


def _poseidon_rows(rows):
    """rows of Fr (a sequence of equally long sequences) or an (n, width, 4) uint64 array -> the array"""
    if isinstance(rows, np.ndarray):
        return rows
    rows = [_scalar_array(r) for r in rows]
    if len({r.shape[0] for r in rows}) > 1:
        raise ValueError(f"rows differ in length: {sorted({r.shape[0] for r in rows})}")
    return np.stack(rows) if rows else np.zeros((0, 1, 4), np.uint64)


def fr_poseidon_batch(inputs, engine=None):
    """[Poseidon(*row) for row in inputs] -> list of Fr: the circomlib / iden3 hash over Fr (x^5, t = arity + 1, R_F = 8, R_P = 56 / 57 / 56 / 60),
    element 0 of the permutation of [0, *row]; one GPU lane per hash.  inputs: rows of 1 .. 4 Fr each, all of one length, or an
    (n, arity, 4) uint64 array.  ValueError for another arity."""
    from .engine import _poseidon_args, POSEIDON_ARITY_MAX
    x = _poseidon_args(_poseidon_rows(inputs), "inputs", 1, POSEIDON_ARITY_MAX, "arity")
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_poseidon_batch(x)]


def fr_poseidon_permute_batch(states, engine=None):
    """[permute(state) for state in states] -> list of lists of Fr: the Poseidon permutation itself on states of t = 2 .. 5 Fr each (or an
    (n, t, 4) uint64 array).  ValueError for another width."""
    from .engine import _poseidon_args, POSEIDON_ARITY_MAX
    x = _poseidon_args(_poseidon_rows(states), "states", 2, POSEIDON_ARITY_MAX + 1, "t")
    return [[Fr.from_limbs(r) for r in st] for st in (engine or default_engine()).fr_poseidon_permute_batch(x)]


def fr_poseidon_ex_batch(inputs, init=None, n_outs=1, engine=None):
    """[PoseidonEx(*row)] -> list of lists of n_outs Fr: circomlib's PoseidonEx(n_inputs, n_outs), the first n_outs elements of the permutation
    of [init_i, *row] at width n_inputs + 1; several GPU lanes share one permutation.  inputs: rows of 1 .. 16 Fr each, all of one length, or
    an (n, n_inputs, 4) uint64 array; init: None (zeros), one Fr for every row, or a sequence of one Fr per row; 1 <= n_outs <= n_inputs + 1.
    fr_poseidon_ex_batch(rows)[i][0] is fr_poseidon_batch(rows)[i] for 1 .. 4 inputs.  ValueError for another shape."""
    from .engine import _poseidon_ex_args
    if isinstance(init, Fr):
        init = [init]
    x, init = _poseidon_ex_args(_poseidon_rows(inputs), None if init is None else _scalar_array(init), n_outs, "inputs")
    return [[Fr.from_limbs(r) for r in row] for row in (engine or default_engine()).fr_poseidon_ex_batch(x, init, n_outs)]


def fr_poseidon_chain_batch(records, rate=16, engine=None):
    """[hash_chain(record)] -> list of Fr, one digest per record of any length (bn_amd.poseidon.hash_chain_host): c = len(record); the record is cut
    into max(1, ceil(len / rate)) blocks of `rate` Fr, the last padded with zeros; per block c = permute([c, *block])[0] at width rate + 1.  The
    framing is this package's own - not an additive sponge, not another library's format.  records: a list of sequences of Fr of any lengths,
    or a pair (flat, offsets) of a sequence of Fr (or an (n, 4) uint64 array) and m + 1 CSR offsets.  ValueError for rate outside 1 .. 16."""
    from .engine import _poseidon_chain_args
    if isinstance(records, tuple) and len(records) == 2:
        flat, offsets = _scalar_array(records[0]), records[1]
    else:
        rows = [_scalar_array(r) for r in records]
        offsets = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.uint64)
        flat = np.concatenate(rows) if rows else np.zeros((0, 4), np.uint64)
    x, o = _poseidon_chain_args(flat, offsets, rate)
    if o.size == 1:
        return []
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_poseidon_chain_batch(x, o, rate)]


def fr_merkle_tree(leaves, engine=None):
    """the n - 1 inner nodes of the binary Poseidon tree over n = 2^k leaves -> list of Fr, level by level: the n / 2 parents of the leaves
    first, the root last; parent i of a level is hash(child[2 i], child[2 i + 1]).  One call, one launch per level.  leaves: a sequence of Fr
    or an (n, 4) uint64 array.  ValueError unless n is a power of two (one leaf gives [])."""
    from .engine import _merkle_args
    x, _ = _merkle_args(_scalar_array(leaves))
    return [Fr.from_limbs(r) for r in (engine or default_engine()).fr_merkle_tree(x)]


def _shift_limbs(shift):
    if shift is None:
        return None
    shift = shift if isinstance(shift, Fr) else Fr(shift)
    if shift.is_zero():
        raise ValueError("the coset shift must be non-zero")
    return shift.limbs


def fr_ntt_batch(rows, inverse=False, shift=None, engine=None):
    """one transform per row, all in ONE call: rows is a sequence of equally long sequences of Fr (length n a power of two) or a (count, n, 4)
    uint64 array.  See fr_ntt."""
    if isinstance(rows, np.ndarray):
        if rows.ndim != 3 or rows.shape[2] != 4:
            raise ValueError("an array of transforms is (count, n, 4) uint64")
        count, n = rows.shape[0], rows.shape[1]
        flat = np.asarray(rows, np.uint64).reshape(-1, 4)
    else:
        rows = [r if isinstance(r, np.ndarray) else list(r) for r in rows]
        count, n = len(rows), (len(rows[0]) if rows else 1)
        if any(len(r) != n for r in rows):
            raise ValueError("every transform of a batch has the same length")
        flat = np.concatenate([_scalar_array(r) for r in rows]) if rows else np.zeros((0, 4), np.uint64)
    if n < 1 or n & (n - 1):
        raise ValueError(f"the length of a transform must be a power of two, got {n}")
    sh = _shift_limbs(shift)
    if count == 0:
        return []
    out = (engine or default_engine()).fr_ntt_batch(flat, n.bit_length() - 1, inverse, sh)
    return [[Fr.from_limbs(r) for r in out[t * n:(t + 1) * n]] for t in range(count)]


def fr_ntt(values, inverse=False, shift=None, engine=None):
    """The number-theoretic transform of `values` (a sequence of Fr or an (n,4) uint64 array; n = 2^log_n, else ValueError) over the subgroup
    generated by w = Fr.root_of_unity(log_n), natural order in and out -> list of Fr.  Forward: out[k] = sum_j values[j] (shift w^k)^j, the
    polynomial with these coefficients evaluated on the coset shift * H; inverse: out[j] = shift^-j n^-1 sum_k values[k] w^(-j k), the
    coefficients back from such evaluations.  shift: an Fr or an integer, None for 1."""
    A = _scalar_array(values)
    return fr_ntt_batch(A.reshape(1, -1, 4), inverse, shift, engine)[0]


def _group_ntt_batch(cls, method, points, log_n, inverse, shift, engine):
    A = _point_array(cls, points)
    if not 0 <= log_n <= 22:
        raise ValueError(f"log_n must be 0..22, got {log_n}")
    if A.shape[0] % (1 << log_n):
        raise ValueError(f"{A.shape[0]} points are not whole transforms of 2^{log_n}")
    sh = _shift_limbs(shift)
    if A.shape[0] == 0:
        return []
    return [cls(r) for r in getattr(engine or default_engine(), method)(A, log_n, inverse, sh)]


def _group_ntt_log(n):
    if n < 1 or n & (n - 1):
        raise ValueError(f"the length of a transform must be a power of two, got {n}")
    return n.bit_length() - 1


def g1_ntt_batch(points, log_n, inverse=False, shift=None, engine=None):
    """len(points) / 2^log_n transforms over G1 in ONE call, transform t in points [t n, (t + 1) n): see g1_ntt.  points: a sequence of G1 or
    an (N, 12) uint64 array; N a multiple of n = 2^log_n, else ValueError."""
    return _group_ntt_batch(G1, "g1_ntt_batch", points, log_n, inverse, shift, engine)


def g2_ntt_batch(points, log_n, inverse=False, shift=None, engine=None):
    """the same over G2: a sequence of G2 or an (N, 24) uint64 array"""
    return _group_ntt_batch(G2, "g2_ntt_batch", points, log_n, inverse, shift, engine)


def g1_ntt(points, inverse=False, shift=None, engine=None):
    """The transform of fr_ntt with G1 points for data (n = 2^log_n of them, else ValueError) and scalar multiplication for the product,
    natural order in and out -> list of normalised G1.  Forward: out[k] = sum_j [shift^j w^(j k)] points[j] with w = Fr.root_of_unity(log_n);
    inverse: out[j] = [n^-1 shift^-j] sum_k [w^(-j k)] points[k].  The inverse transform of the powers tau^i G of a reference string gives
    its Lagrange points (bn_amd.kzg.lagrange_srs).  shift: an Fr or an integer, None for 1."""
    A = _point_array(G1, points)
    return g1_ntt_batch(A, _group_ntt_log(A.shape[0]), inverse, shift, engine)


def g2_ntt(points, inverse=False, shift=None, engine=None):
    """the same over G2"""
    A = _point_array(G2, points)
    return g2_ntt_batch(A, _group_ntt_log(A.shape[0]), inverse, shift, engine)


def _bjj_points(points):
    from . import babyjub
    return babyjub._point_array(points)


def bjj_validate_batch(points, engine=None):
    """(n,) int32 per Baby Jubjub point (bn_amd.babyjub): 0 a valid point ([l]P == O; O itself included), 1 a coordinate's words are not below
    r, 4 not on the curve, 5 on the curve but [l]P != O.  points: a sequence of babyjub.Point or (x, y) integer pairs, or an (n, 2, 4) uint64
    array of raw records"""
    return (engine or default_engine()).bjj_validate_batch(_bjj_points(points))


def bjj_add_batch(p, q, engine=None):
    """[p_i + q_i] -> list of babyjub.Point: the complete sum, for points of the curve (not checked)"""
    from .babyjub import Point
    P, Q = _bjj_points(p), _bjj_points(q)
    if P.shape != Q.shape:
        raise ValueError(f"{P.shape[0]} points, {Q.shape[0]} points")
    return [Point.from_limbs(r) for r in (engine or default_engine()).bjj_add_batch(P, Q)]


def bjj_mul_batch(p, k, engine=None):
    """[[k_i] p_i] -> list of babyjub.Point, for any point of the curve (cofactor components included; not checked) and any Fr k: the scalar is
    the canonical integer of the element"""
    from .babyjub import Point
    P, K = _bjj_points(p), _scalar_array(k)
    if P.shape[0] != K.shape[0]:
        raise ValueError(f"{P.shape[0]} points, {K.shape[0]} scalars")
    return [Point.from_limbs(r) for r in (engine or default_engine()).bjj_mul_batch(P, K)]


def eddsa_poseidon_challenge_batch(a, r8, msg, engine=None):
    """[Poseidon5(r8.x, r8.y, a.x, a.y, msg)] -> list of Fr: the challenge of EdDSA-Poseidon (circomlib's Poseidon at width 6), plain field
    elements in, no curve check.  a, r8: points as for bjj_add_batch; msg: a sequence of Fr or an (n,4) uint64 array"""
    A, R8, M = _bjj_points(a), _bjj_points(r8), _scalar_array(msg)
    if not A.shape[0] == R8.shape[0] == M.shape[0]:
        raise ValueError(f"{A.shape[0]} keys, {R8.shape[0]} points, {M.shape[0]} messages")
    return [Fr.from_limbs(r) for r in (engine or default_engine()).eddsa_poseidon_challenge_batch(A, R8, M)]


def eddsa_poseidon_verify_batch(a, r8, s, msg, engine=None):
    """(n,) int32 per signature (R8, S) on msg under the key A, circomlib's verifyPoseidon: 1 a word array of a, r8, s or msg is not below r or the
    integer of s is not below l, 4 R8 or A is not on the curve, 6 [S]B8 != R8 + [8 hm]A, 0 valid - checked in that order, every row on its own.
    There is no subgroup check: A = O with R8 = [S]B8 verifies, as it does in circomlib"""
    A, R8, S, M = _bjj_points(a), _bjj_points(r8), _scalar_array(s), _scalar_array(msg)
    if not A.shape[0] == R8.shape[0] == S.shape[0] == M.shape[0]:
        raise ValueError(f"{A.shape[0]} keys, {R8.shape[0]} points, {S.shape[0]} scalars, {M.shape[0]} messages")
    return (engine or default_engine()).eddsa_poseidon_verify_batch(A, R8, S, M)


def _byte_records(records, size):
    if isinstance(records, np.ndarray):
        return np.ascontiguousarray(records, np.uint8).reshape(-1, size)
    records = [bytes(b) for b in records]
    if any(len(b) != size for b in records):
        raise ValueError(f"every record is {size} bytes")
    return np.frombuffer(b"".join(records), np.uint8).reshape(-1, size)


def bjj_pack_batch(points, engine=None):
    """[32 bytes per Baby Jubjub point] (circomlib's packPoint as bn_amd.babyjub describes it): y little endian, bit 7 of the last byte set iff
    the integer of x is above (r - 1) / 2.  No validation.  points as for bjj_add_batch"""
    return [r.tobytes() for r in (engine or default_engine()).bjj_pack_batch(_bjj_points(points))]


def bjj_unpack_batch(records, engine=None):
    """(list of babyjub.Point, (n,) int32 status) per 32-byte record: 1 y is not below r, 4 no point has this y, 3 x == 0 with the sign bit set
    (this project's choice), 0 otherwise; a rejected record gives the identity.  No subgroup check, as in circomlib: bjj_validate_batch is there
    for that.  records: a sequence of 32-byte strings or an (n,32) uint8 array"""
    from .babyjub import Point
    out, st = (engine or default_engine()).bjj_unpack_batch(_byte_records(records, 32))
    return [Point.from_limbs(r) for r in out], st


def eddsa_poseidon_verify_packed_batch(a32, sig64, msg, engine=None):
    """(n,) int32 per packed signature (64 bytes: the packed R8, then S little endian) on msg under the packed key (32 bytes): 1 a y, S or msg is
    out of range, 4 a point has no x, 3 a non-canonical sign, 6 [S]B8 != R8 + [8 hm]A, 0 valid - checked in that order, every row on its own,
    in one launch.  No subgroup check"""
    A, S, M = _byte_records(a32, 32), _byte_records(sig64, 64), _scalar_array(msg)
    if not A.shape[0] == S.shape[0] == M.shape[0]:
        raise ValueError(f"{A.shape[0]} keys, {S.shape[0]} signatures, {M.shape[0]} messages")
    return (engine or default_engine()).eddsa_poseidon_verify_packed_batch(A, S, M)


def _grumpkin_points(points):
    from . import grumpkin
    return grumpkin._point_array(points)


def _grumpkin_scalars(scalars):
    from . import grumpkin
    return grumpkin._scalar_array(scalars)


def grumpkin_validate_batch(points, engine=None):
    """(n,) int32 per Grumpkin point (bn_amd.grumpkin): 0 a point of the curve (O = (0, 0) included), 1 a coordinate's words are not below r,
    4 not on the curve.  The cofactor is 1: there is no subgroup status.  points: a sequence of grumpkin.Point or (x, y) integer pairs, or an
    (n, 2, 4) uint64 array of raw records"""
    return (engine or default_engine()).grumpkin_validate_batch(_grumpkin_points(points))


def grumpkin_add_batch(p, q, engine=None):
    """[p_i + q_i] -> list of grumpkin.Point: the complete sum, for points of the curve (not checked)"""
    from .grumpkin import Point
    P, Q = _grumpkin_points(p), _grumpkin_points(q)
    if P.shape != Q.shape:
        raise ValueError(f"{P.shape[0]} points, {Q.shape[0]} points")
    return [Point.from_limbs(r) for r in (engine or default_engine()).grumpkin_add_batch(P, Q)]


def grumpkin_mul_batch(p, k, engine=None):
    """[[k_i] p_i] -> list of grumpkin.Point, for points of the curve (not checked).  k: a sequence of integers in [0, 2^256) (an Fr counts as
    its canonical integer), or an (n, 4) uint64 array of plain little-endian words - NOT Montgomery images; the result is [k mod q]p"""
    from .grumpkin import Point
    P, K = _grumpkin_points(p), _grumpkin_scalars(k)
    if P.shape[0] != K.shape[0]:
        raise ValueError(f"{P.shape[0]} points, {K.shape[0]} scalars")
    return [Point.from_limbs(r) for r in (engine or default_engine()).grumpkin_mul_batch(P, K)]


def grumpkin_msm_batch(p, k, offsets, engine=None):
    """[sum of [k_t] p_t over t in [offsets[j], offsets[j+1])] -> list of grumpkin.Point: many independent multi-scalar multiplications in
    one call; an empty or cancelling segment gives O.  p, k as for grumpkin_mul_batch; offsets: m + 1 CSR offsets"""
    from .grumpkin import Point
    P, K = _grumpkin_points(p), _grumpkin_scalars(k)
    if P.shape[0] != K.shape[0]:
        raise ValueError(f"{P.shape[0]} points, {K.shape[0]} scalars")
    return [Point.from_limbs(r) for r in (engine or default_engine()).grumpkin_msm_batch(P, K, offsets)]


class PreparedG2:
    """G2 points prepared once for many pairings (the crate's internal G2Precomp, groups/mod.rs:472-483,557-588, as a device-resident
    native table: Engine.g2_prepare).  One point: shared by every P; several: point i is paired with ps[i]."""

    def __init__(self, qs, engine=None):
        e = engine or default_engine()
        Q = qs.limbs if isinstance(qs, G2) else (np.stack([q.limbs for q in qs]) if not isinstance(qs, np.ndarray) else qs)
        self._e = e
        self._h = e.g2_prepare(Q)

    def __len__(self):
        return self._h.count

    def pairing(self, p):
        """== pairing(p, q) for a one-point handle"""
        return Gt(self._e.pairing_prepared_native_batch(p.limbs, self._h)[0])

    def pairing_batch(self, ps):
        P = np.stack([p.limbs for p in ps]) if not isinstance(ps, np.ndarray) else ps
        return self._e.pairing_prepared_native_batch(P, self._h)

    def pairing_product(self, ps):
        """== fold(Gt::one(), acc * pairing(ps[i], q[i])) (shootout/main.rs:11-16) with ONE final exponentiation"""
        P = np.stack([p.limbs for p in ps]) if not isinstance(ps, np.ndarray) else ps
        return Gt(self._e.pairing_product_prepared_native(P, self._h))

    def _product_batch_limbs(self, segments, q_index, offsets):
        if offsets is not None:                   # (n,12) array + per-pair indices (or None) + CSR offsets
            P = np.asarray(segments, np.uint64).reshape(-1, G1_WORDS)
            return self._e.pairing_product_batch_prepared_native(P, self._h, np.asarray(offsets, np.uint64), q_index)
        if q_index is not None:
            raise ValueError("q_index is only taken together with offsets (segments carry their indices: (G1, index))")
        segments = [list(s) for s in segments]
        offs = np.zeros(len(segments) + 1, np.uint64)
        offs[1:] = np.cumsum([len(s) for s in segments], dtype=np.uint64) if segments else []
        pairs = [pi for s in segments for pi in s]
        n = len(self)
        for _, i in pairs:
            if not 0 <= int(i) < n:
                raise ValueError(f"index {i} names no point of this handle ({n} points)")
        P = np.stack([p.limbs for p, _ in pairs]) if pairs else np.zeros((0, G1_WORDS), np.uint64)
        return self._e.pairing_product_batch_prepared_native(P, self._h, offs, np.array([int(i) for _, i in pairs], np.uint64))

    def pairing_product_batch(self, segments, q_index=None, offsets=None):
        """[fold(Gt::one(), acc * pairing(p, point i of this handle)) over the (p, i) of each segment] with ONE final exponentiation per segment -
        pairing_product_batch with the G2 side prepared.  segments: a sequence of sequences of (G1, index) - an empty one gives Gt::one() -, or an
        (n,12) uint64 array as `segments` plus CSR `offsets` (m + 1 entries) and `q_index` (n indices; None: pair i uses point i, every pair
        point 0 of a one-point handle)."""
        return [Gt(r) for r in self._product_batch_limbs(segments, q_index, offsets)]

    def pairing_check_batch(self, segments, q_index=None, offsets=None):
        """numpy bool array: product of segment j == Gt::one() - a block of Groth16 / EIP-197-style checks against prepared points"""
        return (self._product_batch_limbs(segments, q_index, offsets) == Gt.one().limbs).all(axis=1)

    def close(self):
        self._h.close()
