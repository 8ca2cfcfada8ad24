// bn254.hpp - header-only C++ facade over the C ABI (bn254_hip.h), mirroring the public API of the reference crate
// zcash-hackworks/bn (src/lib.rs): same names, argument meaning and error behaviour, so code written against the crate reads
// the same here.  Values are the crate's #[repr(C)] memory images; all curve/pairing arithmetic runs on the GPU.
//
//   reference (Rust)                              here (C++)
//   bn::pairing(p, q) -> Gt        lib.rs:181     bn::pairing(p, q)
//   G1::one() / zero() / is_zero   lib.rs:83-87   bn::G1::one() / zero() / is_zero()
//   g * fr                         lib.rs:116     g * fr                  (returned normalized, lib.rs:88-95)
//   Gt::one(), a == b              lib.rs:169     bn::Gt::one(), a == b   (canonical limbs: memcmp)
//   (fold of shootout/main.rs)                    bn::pairing_batch(...), bn::pairing_product(...)
#pragma once
#include <array>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bn254_hip.h"

namespace bn {

struct Error : std::runtime_error {
    int code;
    explicit Error(int c) : std::runtime_error(std::string("bn254_hip: ") + bn254_error_string(c)), code(c) {}
};
inline void check(int rc) { if (rc != 0) throw Error(rc); }

// R mod q, the Montgomery image of 1 (fp.rs:170-177)
static const uint64_t FQ_ONE[4] = {0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full};
static const uint64_t FQ_TWO[4] = {0xa6ba871b8b1e1b3aull, 0x14f1d651eb8e167bull, 0xccdd46def0f28c58ull, 0x1c14ef83340fbe5eull};
static const uint64_t FR_ONE[4] = {0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full};

struct Fr {
    bn_fr v;
    static Fr one() { Fr r; std::memcpy(r.v.l, FR_ONE, 32); return r; }     // lib.rs:21
    static Fr zero() { Fr r; std::memset(&r.v, 0, 32); return r; }          // lib.rs:20
};
struct G1 {
    bn_g1 v;
    static G1 one() {                                                        // groups/mod.rs:355-361
        G1 r; std::memcpy(r.v.x, FQ_ONE, 32); std::memcpy(r.v.y, FQ_TWO, 32); std::memcpy(r.v.z, FQ_ONE, 32); return r;
    }
    static G1 zero() { G1 r; std::memset(&r.v, 0, sizeof r.v); std::memcpy(r.v.y, FQ_ONE, 32); return r; }   // (0,1,0)
    bool is_zero() const { return (v.z[0] | v.z[1] | v.z[2] | v.z[3]) == 0; }
    G1 operator*(const Fr &k) const { G1 r; check(bn254_g1_mul_batch(nullptr, &v, &k.v, &r.v, 1)); return r; }
    G1 operator+(const G1 &o) const { G1 r; check(bn254_g1_add_batch(nullptr, &v, &o.v, &r.v, 1, 0)); return r; }     // lib.rs:103-106
    G1 operator-(const G1 &o) const { G1 r; check(bn254_g1_add_batch(nullptr, &v, &o.v, &r.v, 1, 1)); return r; }     // lib.rs:108-111
    G1 operator-() const { return zero() - *this; }                                                                  // lib.rs:113-114
    void normalize() { check(bn254_g1_normalize_batch(nullptr, &v, &v, 1)); }                                        // lib.rs:88-95 (in place)
    bool operator==(const G1 &o) const { int32_t r = 0; check(bn254_g1_eq_batch(nullptr, &v, &o.v, &r, 1)); return r != 0; }   // groups/mod.rs:83-109
    bool operator!=(const G1 &o) const { return !(*this == o); }
};
struct G2 {
    bn_g2 v;
    static G2 one() {                                                        // groups/mod.rs:377-390
        static const uint64_t X[8] = {0x8e83b5d102bc2026ull, 0xdceb1935497b0172ull, 0xfbb8264797811adfull, 0x19573841af96503bull,
                                      0xafb4737da84c6140ull, 0x6043dd5a5802d8c4ull, 0x09e950fc52a02f86ull, 0x14fef0833aea7b6bull};
        static const uint64_t Y[8] = {0x619dfa9d886be9f6ull, 0xfe7fd297f59e9b78ull, 0xff9e1a62231b7dfeull, 0x28fd7eebae9e4206ull,
                                      0x64095b56c71856eeull, 0xdc57f922327d3cbbull, 0x55f935be33351076ull, 0x0da4a0e693fd6482ull};
        G2 r; std::memcpy(r.v.x, X, 64); std::memcpy(r.v.y, Y, 64); std::memset(r.v.z, 0, 64); std::memcpy(r.v.z, FQ_ONE, 32); return r;
    }
    static G2 zero() { G2 r; std::memset(&r.v, 0, sizeof r.v); std::memcpy(r.v.y, FQ_ONE, 32); return r; }
    bool is_zero() const { uint64_t o = 0; for (int i = 0; i < 8; ++i) o |= v.z[i]; return o == 0; }
    G2 operator*(const Fr &k) const { G2 r; check(bn254_g2_mul_batch(nullptr, &v, &k.v, &r.v, 1)); return r; }
    G2 operator+(const G2 &o) const { G2 r; check(bn254_g2_add_batch(nullptr, &v, &o.v, &r.v, 1, 0)); return r; }
    G2 operator-(const G2 &o) const { G2 r; check(bn254_g2_add_batch(nullptr, &v, &o.v, &r.v, 1, 1)); return r; }
    G2 operator-() const { return zero() - *this; }
    void normalize() { check(bn254_g2_normalize_batch(nullptr, &v, &v, 1)); }                                        // lib.rs:131-138 (in place)
    bool operator==(const G2 &o) const { int32_t r = 0; check(bn254_g2_eq_batch(nullptr, &v, &o.v, &r, 1)); return r != 0; }
    bool operator!=(const G2 &o) const { return !(*this == o); }
};
struct Gt {
    bn_gt v;
    static Gt one() { Gt r; std::memset(&r.v, 0, sizeof r.v); std::memcpy(r.v.c, FQ_ONE, 32); return r; }     // lib.rs:169
    Gt operator*(const Gt &o) const { Gt r; check(bn254_gt_mul_batch(nullptr, &v, &o.v, &r.v, 1)); return r; }      // lib.rs:175-179
    Gt pow(const Fr &k) const { Gt r; check(bn254_gt_pow_batch(nullptr, &v, &k.v, &r.v, 1)); return r; }            // lib.rs:171
    Gt inverse() const { Gt r; check(bn254_gt_inverse_batch(nullptr, &v, &r.v, 1)); return r; }                     // lib.rs:172
    bool operator==(const Gt &o) const { return std::memcmp(&v, &o.v, sizeof v) == 0; }
    bool operator!=(const Gt &o) const { return !(*this == o); }
};
static_assert(sizeof(Fr) == 32 && sizeof(G1) == 96 && sizeof(G2) == 192 && sizeof(Gt) == 384, "layouts must equal the crate's #[repr(C)] types");

// lib.rs:181-183
inline Gt pairing(const G1 &p, const G2 &q) { Gt r; check(bn254_pairing_batch(nullptr, &p.v, &q.v, &r.v, 1)); return r; }
// out[i] = pairing(p[i], q[i])
inline std::vector<Gt> pairing_batch(const std::vector<G1> &p, const std::vector<G2> &q) {
    if (p.size() != q.size()) throw std::invalid_argument("pairing_batch: length mismatch");
    std::vector<Gt> out(p.size());
    check(bn254_pairing_batch(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_g2 *>(q.data()),
                              reinterpret_cast<bn_gt *>(out.data()), p.size()));
    return out;
}
// fold(Gt::one(), acc * pairing(p, q))   (shootout/main.rs:11-16)
inline Gt pairing_product(const std::vector<G1> &p, const std::vector<G2> &q) {
    if (p.size() != q.size()) throw std::invalid_argument("pairing_product: length mismatch");
    Gt r;
    check(bn254_pairing_product(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_g2 *>(q.data()), p.size(), &r.v));
    return r;
}
// out[j] = that fold over the pairs [offsets[j], offsets[j+1]) (CSR segments, offsets.size() = m + 1): ONE final exponentiation per segment
inline std::vector<Gt> pairing_product_batch(const std::vector<G1> &p, const std::vector<G2> &q, const std::vector<size_t> &offsets) {
    if (p.size() != q.size()) throw std::invalid_argument("pairing_product_batch: length mismatch");
    if (offsets.empty() || offsets.back() != p.size()) throw std::invalid_argument("pairing_product_batch: offsets must end at the pair count");
    std::vector<Gt> out(offsets.size() - 1);
    check(bn254_pairing_product_batch(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_g2 *>(q.data()), offsets.data(),
                                      out.size(), reinterpret_cast<bn_gt *>(out.data())));
    return out;
}
// out[j] = normalize(sum of p[i] * k[i] over the terms [offsets[j], offsets[j+1])) (CSR segments, offsets.size() = m + 1): many independent
// multi-scalar multiplications in one call, ONE inversion per segment; an empty or cancelling segment gives G::zero()
inline std::vector<G1> g1_msm_batch(const std::vector<G1> &p, const std::vector<Fr> &k, const std::vector<size_t> &offsets) {
    if (p.size() != k.size()) throw std::invalid_argument("g1_msm_batch: length mismatch");
    if (offsets.empty() || offsets.back() != p.size()) throw std::invalid_argument("g1_msm_batch: offsets must end at the term count");
    std::vector<G1> out(offsets.size() - 1);
    check(bn254_g1_msm_batch(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), offsets.data(),
                             out.size(), reinterpret_cast<bn_g1 *>(out.data())));
    return out;
}
inline std::vector<G2> g2_msm_batch(const std::vector<G2> &p, const std::vector<Fr> &k, const std::vector<size_t> &offsets) {
    if (p.size() != k.size()) throw std::invalid_argument("g2_msm_batch: length mismatch");
    if (offsets.empty() || offsets.back() != p.size()) throw std::invalid_argument("g2_msm_batch: offsets must end at the term count");
    std::vector<G2> out(offsets.size() - 1);
    check(bn254_g2_msm_batch(nullptr, reinterpret_cast<const bn_g2 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), offsets.data(),
                             out.size(), reinterpret_cast<bn_g2 *>(out.data())));
    return out;
}
// normalize(sum of p[i] * k[i] over ALL terms): one large multi-scalar multiplication - the bucket (Pippenger) method from
// BN254_OPT_MSM_BUCKET_MIN terms on, the one-segment g1_msm_batch below it; the same bytes either way
inline G1 g1_msm(const std::vector<G1> &p, const std::vector<Fr> &k) {
    if (p.size() != k.size()) throw std::invalid_argument("g1_msm: length mismatch");
    G1 out;
    check(bn254_g1_msm(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), p.size(), reinterpret_cast<bn_g1 *>(&out)));
    return out;
}
inline G2 g2_msm(const std::vector<G2> &p, const std::vector<Fr> &k) {
    if (p.size() != k.size()) throw std::invalid_argument("g2_msm: length mismatch");
    G2 out;
    check(bn254_g2_msm(nullptr, reinterpret_cast<const bn_g2 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), p.size(), reinterpret_cast<bn_g2 *>(&out)));
    return out;
}
// out[i] = normalize(base * k[i]): fixed-base scalar multiplication, many scalars against ONE point - the bytes of g1_mul_batch on the tiled
// base, by mixed additions over a table of multiples of `base` that the context caches (four bases per group)
inline std::vector<G1> g1_mul_base(const G1 &base, const std::vector<Fr> &k) {
    std::vector<G1> out(k.size());
    check(bn254_g1_mul_base_batch(nullptr, reinterpret_cast<const bn_g1 *>(&base), reinterpret_cast<const bn_fr *>(k.data()), reinterpret_cast<bn_g1 *>(out.data()), k.size()));
    return out;
}
inline std::vector<G2> g2_mul_base(const G2 &base, const std::vector<Fr> &k) {
    std::vector<G2> out(k.size());
    check(bn254_g2_mul_base_batch(nullptr, reinterpret_cast<const bn_g2 *>(&base), reinterpret_cast<const bn_fr *>(k.data()), reinterpret_cast<bn_g2 *>(out.data()), k.size()));
    return out;
}
// out[i] = p[i].normalize() = (x/z^2, y/z^3, 1), infinity as G::zero(): neighbouring points share one field inversion
inline std::vector<G1> g1_normalize(const std::vector<G1> &p) {
    std::vector<G1> out(p.size());
    check(bn254_g1_normalize_batch(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<bn_g1 *>(out.data()), p.size()));
    return out;
}
inline std::vector<G2> g2_normalize(const std::vector<G2> &p) {
    std::vector<G2> out(p.size());
    check(bn254_g2_normalize_batch(nullptr, reinterpret_cast<const bn_g2 *>(p.data()), reinterpret_cast<bn_g2 *>(out.data()), p.size()));
    return out;
}
// The crate's Fr operations (lib.rs:15-53) over arrays of scalars, on the device: out[i] = a[i] + b[i], a[i] - b[i], a[i] * b[i],
// a[i].pow(e[i]) (0^0 is one), Fr::interpret of 64-byte records, and a[i].inverse() as (values, ok) with Fr::zero() / false for a zero element
inline std::vector<Fr> fr_binary(int (*fn)(bn254_ctx *, const bn_fr *, const bn_fr *, bn_fr *, size_t), const std::vector<Fr> &a, const std::vector<Fr> &b) {
    if (a.size() != b.size()) throw std::invalid_argument("fr batch: length mismatch");
    std::vector<Fr> out(a.size());
    check(fn(nullptr, reinterpret_cast<const bn_fr *>(a.data()), reinterpret_cast<const bn_fr *>(b.data()), reinterpret_cast<bn_fr *>(out.data()), a.size()));
    return out;
}
inline std::vector<Fr> fr_add(const std::vector<Fr> &a, const std::vector<Fr> &b) {
    return fr_binary([](bn254_ctx *c, const bn_fr *x, const bn_fr *y, bn_fr *o, size_t n) { return bn254_fr_add_batch(c, x, y, o, n, 0); }, a, b);
}
inline std::vector<Fr> fr_sub(const std::vector<Fr> &a, const std::vector<Fr> &b) {
    return fr_binary([](bn254_ctx *c, const bn_fr *x, const bn_fr *y, bn_fr *o, size_t n) { return bn254_fr_add_batch(c, x, y, o, n, 1); }, a, b);
}
inline std::vector<Fr> fr_mul(const std::vector<Fr> &a, const std::vector<Fr> &b) { return fr_binary(bn254_fr_mul_batch, a, b); }
inline std::vector<Fr> fr_pow(const std::vector<Fr> &a, const std::vector<Fr> &e) { return fr_binary(bn254_fr_pow_batch, a, e); }
inline std::pair<std::vector<Fr>, std::vector<bool>> fr_inverse(const std::vector<Fr> &a) {
    std::vector<Fr> out(a.size());
    std::vector<int32_t> ok(a.size());
    check(bn254_fr_inverse_batch(nullptr, reinterpret_cast<const bn_fr *>(a.data()), reinterpret_cast<bn_fr *>(out.data()), ok.data(), a.size()));
    return {out, std::vector<bool>(ok.begin(), ok.end())};
}
// Option<Fr> square roots: the root whose canonical integer is not above (r - 1) / 2; false and Fr::zero() for a non-residue
inline std::pair<std::vector<Fr>, std::vector<bool>> fr_sqrt(const std::vector<Fr> &a) {
    std::vector<Fr> out(a.size());
    std::vector<int32_t> ok(a.size());
    check(bn254_fr_sqrt_batch(nullptr, reinterpret_cast<const bn_fr *>(a.data()), reinterpret_cast<bn_fr *>(out.data()), ok.data(), a.size()));
    return {out, std::vector<bool>(ok.begin(), ok.end())};
}
inline std::vector<Fr> fr_interpret(const std::vector<std::array<uint8_t, 64>> &bufs) {
    std::vector<Fr> out(bufs.size());
    check(bn254_fr_interpret_batch(nullptr, reinterpret_cast<const uint8_t *>(bufs.data()), reinterpret_cast<bn_fr *>(out.data()), bufs.size()));
    return out;
}
// w_n for n = 2^log_n (0..28): w_28^(2^(28 - log_n)), w_28 = 5^((r-1)/2^28); computed on the host
inline Fr fr_root_of_unity(int log_n) {
    Fr out;
    check(bn254_fr_root_of_unity(log_n, reinterpret_cast<bn_fr *>(&out)));
    return out;
}
// values.size() / 2^log_n number-theoretic transforms of 2^log_n elements each, natural order in and out.  Forward: the polynomial with
// coefficients `values` evaluated at shift * w_n^k; inverse: the coefficients back from such evaluations.  shift: nullptr for one.
inline std::vector<Fr> fr_ntt(const std::vector<Fr> &values, int log_n, bool inverse = false, const Fr *shift = nullptr) {
    if (log_n < 0 || log_n > BN254_NTT_LOG_MAX || values.size() % (size_t(1) << log_n)) throw std::invalid_argument("fr_ntt: not whole transforms of 2^log_n");
    std::vector<Fr> out(values.size());
    check(bn254_fr_ntt_batch(nullptr, reinterpret_cast<const bn_fr *>(values.data()), reinterpret_cast<bn_fr *>(out.data()), log_n, values.size() >> log_n, inverse ? 1 : 0,
                             reinterpret_cast<const bn_fr *>(shift)));
    return out;
}
// The same transforms with points for data and scalar multiplication for the product: points.size() / 2^log_n transforms of 2^log_n
// points each, natural order in and out, every output normalised.  The inverse transform of the powers tau^i G of a reference string
// gives its Lagrange points.
inline std::vector<G1> g1_ntt(const std::vector<G1> &points, int log_n, bool inverse = false, const Fr *shift = nullptr) {
    if (log_n < 0 || log_n > BN254_GROUP_NTT_LOG_MAX || points.size() % (size_t(1) << log_n)) throw std::invalid_argument("g1_ntt: not whole transforms of 2^log_n");
    std::vector<G1> out(points.size());
    check(bn254_g1_ntt_batch(nullptr, reinterpret_cast<const bn_g1 *>(points.data()), reinterpret_cast<bn_g1 *>(out.data()), log_n, points.size() >> log_n, inverse ? 1 : 0,
                             reinterpret_cast<const bn_fr *>(shift)));
    return out;
}
inline std::vector<G2> g2_ntt(const std::vector<G2> &points, int log_n, bool inverse = false, const Fr *shift = nullptr) {
    if (log_n < 0 || log_n > BN254_GROUP_NTT_LOG_MAX || points.size() % (size_t(1) << log_n)) throw std::invalid_argument("g2_ntt: not whole transforms of 2^log_n");
    std::vector<G2> out(points.size());
    check(bn254_g2_ntt_batch(nullptr, reinterpret_cast<const bn_g2 *>(points.data()), reinterpret_cast<bn_g2 *>(out.data()), log_n, points.size() >> log_n, inverse ? 1 : 0,
                             reinterpret_cast<const bn_fr *>(shift)));
    return out;
}
// out[j] = sum of coeff[t] * x[index[t]] over t in [offsets[j], offsets[j+1]): a sparse matrix in CSR form times the vector x - the witness
// map of an R1CS.  index: nullptr for x[t], a plain segmented inner product (x.size() == coeff.size()).  An empty segment gives Fr::zero().
inline std::vector<Fr> fr_dot(const std::vector<Fr> &coeff, const std::vector<uint64_t> *index, const std::vector<Fr> &x, const std::vector<size_t> &offsets) {
    if (offsets.empty() || offsets.back() != coeff.size() || (index ? index->size() != coeff.size() : x.size() != coeff.size()))
        throw std::invalid_argument("fr_dot: offsets, index and coeff disagree in length");
    std::vector<Fr> out(offsets.size() - 1);
    check(bn254_fr_dot_batch(nullptr, reinterpret_cast<const bn_fr *>(coeff.data()), index ? index->data() : nullptr, reinterpret_cast<const bn_fr *>(x.data()), x.size(),
                             offsets.data(), out.size(), reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// out[t] = a[t] * prev + b[t] over the terms of every segment [offsets[j], offsets[j+1]) in order, prev = out[t-1] or init[j] at the segment's
// first term: segmented prefix sums (a: nullptr), prefix products (b: nullptr), powers and Horner's rule (BN254_SCAN_A_PER_SEGMENT: a holds
// one factor per segment).  init: nullptr for Fr::zero() with b, Fr::one() without.  flags: BN254_SCAN_*.  One output per term.
inline std::vector<Fr> fr_scan(const std::vector<Fr> *a, const std::vector<Fr> *b, const std::vector<Fr> *init, const std::vector<size_t> &offsets, unsigned flags = 0) {
    if (offsets.empty() || (!a && !b)) throw std::invalid_argument("fr_scan: no offsets, or neither a nor b");
    const size_t m = offsets.size() - 1, n = offsets.back();
    if ((b && b->size() != n) || (init && init->size() != m) || (a && a->size() != ((flags & BN254_SCAN_A_PER_SEGMENT) ? m : n)))
        throw std::invalid_argument("fr_scan: offsets, a, b and init disagree in length");
    std::vector<Fr> out(n);
    auto ptr = [](const std::vector<Fr> *v) { return v ? reinterpret_cast<const bn_fr *>(v->data()) : nullptr; };
    check(bn254_fr_scan_batch(nullptr, ptr(a), ptr(b), ptr(init), offsets.data(), m, flags, reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// the table of eq(z, .) over the hypercube of z.size() variables: out[i] = prod_j (bit j of i ? z[j] : 1 - z[j]); no variables give {one}
inline std::vector<Fr> fr_mle_eq(const std::vector<Fr> &z) {
    if (z.size() > BN254_MLE_VARS_MAX) throw std::invalid_argument("fr_mle_eq: too many variables");
    std::vector<Fr> out(size_t(1) << z.size());
    check(bn254_fr_mle_eq(nullptr, reinterpret_cast<const bn_fr *>(z.data()), int(z.size()), reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// out[i] = a[i] + r * (a[i + a.size() / 2] - a[i]): the multilinear table a with its MOST significant variable bound to r; k tables stored
// index-major (a[i * k + j]) are folded by the one call
inline std::vector<Fr> fr_mle_fold(const std::vector<Fr> &a, const Fr &r) {
    if (a.size() % 2) throw std::invalid_argument("fr_mle_fold: an odd length");
    std::vector<Fr> out(a.size() / 2);
    check(bn254_fr_mle_fold(nullptr, reinterpret_cast<const bn_fr *>(a.data()), a.size(), reinterpret_cast<const bn_fr *>(&r), reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// the round polynomial of a sumcheck at t = 0 .. degree: out[t] = sum over i < n / 2 and the groups c of group_coeff[c] * prod over j in group c
// of (T_j[i] + t * (T_j[i + n / 2] - T_j[i])), T_j[i] = tables[i * k + j], n = tables.size() / k; group c holds the table numbers
// group_tables[group_offsets[c] .. group_offsets[c + 1])
inline std::vector<Fr> fr_sumcheck_round(const std::vector<Fr> &tables, size_t k, const std::vector<size_t> &group_offsets, const std::vector<uint64_t> &group_tables,
                                         const std::vector<Fr> &group_coeff, int degree) {
    if (k == 0 || tables.size() % (2 * k) || group_offsets.empty() || group_coeff.size() != group_offsets.size() - 1 || group_offsets.back() != group_tables.size() || degree < 1)
        throw std::invalid_argument("fr_sumcheck_round: tables, k and the groups disagree");
    std::vector<Fr> out(size_t(degree) + 1);
    check(bn254_fr_sumcheck_round(nullptr, reinterpret_cast<const bn_fr *>(tables.data()), tables.size() / k, k, group_offsets.data(), group_tables.data(),
                                  reinterpret_cast<const bn_fr *>(group_coeff.data()), group_coeff.size(), degree, reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// fr_mle_fold of the k index-major tables by r and fr_sumcheck_round of the folded tables in one pass: {folded, out} with
// folded[i * k + j] = T_j[i] + r * (T_j[i + n / 2] - T_j[i]) (n = tables.size() / k, a multiple of 4) and out the degree + 1 values of the round
// polynomial over folded - what a sumcheck prover does between two challenges
inline std::pair<std::vector<Fr>, std::vector<Fr>> fr_sumcheck_fold_round(const std::vector<Fr> &tables, size_t k, const Fr &r, const std::vector<size_t> &group_offsets,
                                                                          const std::vector<uint64_t> &group_tables, const std::vector<Fr> &group_coeff, int degree) {
    if (k == 0 || tables.empty() || tables.size() % (4 * k) || group_offsets.empty() || group_coeff.size() != group_offsets.size() - 1 || group_offsets.back() != group_tables.size() ||
        degree < 1)
        throw std::invalid_argument("fr_sumcheck_fold_round: tables, k and the groups disagree");
    std::vector<Fr> folded(tables.size() / 2), out(size_t(degree) + 1);
    check(bn254_fr_sumcheck_fold_round(nullptr, reinterpret_cast<const bn_fr *>(tables.data()), tables.size() / k, k, reinterpret_cast<const bn_fr *>(&r), group_offsets.data(),
                                       group_tables.data(), reinterpret_cast<const bn_fr *>(group_coeff.data()), group_coeff.size(), degree, reinterpret_cast<bn_fr *>(folded.data()),
                                       reinterpret_cast<bn_fr *>(out.data())));
    return {std::move(folded), std::move(out)};
}
// the quotients of a multilinear opening of the table a (2^z.size() values) at z, in heap order: out[0] = f(z) and out[2^j + i] = q_j[i] with
// f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1}); the field work of a multilinear KZG opening
inline std::vector<Fr> fr_mle_quotients(const std::vector<Fr> &a, const std::vector<Fr> &z) {
    if (z.size() > BN254_MLE_VARS_MAX || a.size() != size_t(1) << z.size()) throw std::invalid_argument("fr_mle_quotients: the table holds 2^z.size() values");
    std::vector<Fr> out(a.size());
    check(bn254_fr_mle_quotients(nullptr, reinterpret_cast<const bn_fr *>(a.data()), int(z.size()), reinterpret_cast<const bn_fr *>(z.data()), reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// out[i] = Poseidon(in[i * arity .. (i + 1) * arity)): the circomlib / iden3 hash over Fr, element 0 of the permutation of {0, x_1, .., x_arity}
inline std::vector<Fr> fr_poseidon(const std::vector<Fr> &in, int arity) {
    if (arity < 1 || arity > BN254_POSEIDON_ARITY_MAX || in.size() % size_t(arity)) throw std::invalid_argument("fr_poseidon: arity and the inputs disagree");
    std::vector<Fr> out(in.size() / size_t(arity));
    check(bn254_fr_poseidon_batch(nullptr, reinterpret_cast<const bn_fr *>(in.data()), arity, reinterpret_cast<bn_fr *>(out.data()), out.size()));
    return out;
}
// the Poseidon permutation on states.size() / t states of t elements each, t = 2 .. 5
inline std::vector<Fr> fr_poseidon_permute(const std::vector<Fr> &states, int t) {
    if (t < 2 || t > BN254_POSEIDON_ARITY_MAX + 1 || states.size() % size_t(t)) throw std::invalid_argument("fr_poseidon_permute: t and the states disagree");
    std::vector<Fr> out(states.size());
    check(bn254_fr_poseidon_permute_batch(nullptr, reinterpret_cast<const bn_fr *>(states.data()), t, reinterpret_cast<bn_fr *>(out.data()), states.size() / size_t(t)));
    return out;
}
// the n - 1 inner nodes of the binary Poseidon tree over n = 2^k leaves, level by level, the root last; one leaf gives no node
inline std::vector<Fr> fr_merkle_tree(const std::vector<Fr> &leaves) {
    const size_t n = leaves.size();
    int log_n = 0;
    while ((size_t(1) << log_n) < n) ++log_n;
    if (n == 0 || (size_t(1) << log_n) != n || log_n > BN254_MERKLE_LOG_MAX) throw std::invalid_argument("fr_merkle_tree: the leaves are not a power of two");
    std::vector<Fr> nodes(n - 1);
    check(bn254_fr_merkle_tree(nullptr, reinterpret_cast<const bn_fr *>(leaves.data()), log_n, reinterpret_cast<bn_fr *>(nodes.data())));
    return nodes;
}
// circomlib's PoseidonEx(n_inputs, n_outs) on in.size() / n_inputs rows of 1 .. 16 inputs: the first n_outs elements of the permutation of
// [init[i], row..] at width n_inputs + 1 (init: nullptr for zeros, else one element per row), n_outs consecutive outputs per row
inline std::vector<Fr> fr_poseidon_ex(const std::vector<Fr> &in, int n_inputs, const std::vector<Fr> *init = nullptr, int n_outs = 1) {
    if (n_inputs < 1 || n_inputs > BN254_POSEIDON_EX_INPUTS_MAX || n_outs < 1 || n_outs > n_inputs + 1 || in.size() % size_t(n_inputs) ||
        (init && init->size() != in.size() / size_t(n_inputs)))
        throw std::invalid_argument("fr_poseidon_ex: n_inputs, n_outs, init and the inputs disagree");
    const size_t n = in.size() / size_t(n_inputs);
    std::vector<Fr> out(n * size_t(n_outs));
    check(bn254_fr_poseidon_ex_batch(nullptr, reinterpret_cast<const bn_fr *>(in.data()), n_inputs, init ? reinterpret_cast<const bn_fr *>(init->data()) : nullptr, n_outs,
                                     reinterpret_cast<bn_fr *>(out.data()), n));
    return out;
}
// one digest per variable-length record in[offsets[j] .. offsets[j + 1]): c = len, then per block of `rate` elements (the last padded with zeros, an
// empty record is one block of zeros) c = permute([c, block..])[0] at width rate + 1.  The framing is this library's own.
inline std::vector<Fr> fr_poseidon_chain(const std::vector<Fr> &in, const std::vector<size_t> &offsets, int rate = 16) {
    if (rate < 1 || rate > BN254_POSEIDON_EX_INPUTS_MAX || offsets.empty() || offsets.back() != in.size()) throw std::invalid_argument("fr_poseidon_chain: rate, offsets and the inputs disagree");
    std::vector<Fr> out(offsets.size() - 1);
    check(bn254_fr_poseidon_chain_batch(nullptr, reinterpret_cast<const bn_fr *>(in.data()), offsets.data(), out.size(), rate, reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// Compressed encodings: x and one sign bit, 32 bytes per G1 and 64 per G2 point, in the layout `format` (BN254_COMPRESSED_ARK or
// BN254_COMPRESSED_GNARK: laid out as ark-serialize / gnark-crypto describe; not checked against those libraries here).  compress takes any
// Jacobian form and writes canonical bytes; decompress returns (x, y, 1) and one status per record (0 ok, 3 flags, 1 range, 4 no such point,
// 5 not in the subgroup), a rejected record as G::zero()
inline std::vector<uint8_t> g1_compress(const std::vector<G1> &p, int format = BN254_COMPRESSED_ARK) {
    std::vector<uint8_t> out(p.size() * BN254_G1_COMPRESSED_BYTES);
    check(bn254_g1_compress_batch(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), format, out.data(), p.size()));
    return out;
}
inline std::vector<uint8_t> g2_compress(const std::vector<G2> &p, int format = BN254_COMPRESSED_ARK) {
    std::vector<uint8_t> out(p.size() * BN254_G2_COMPRESSED_BYTES);
    check(bn254_g2_compress_batch(nullptr, reinterpret_cast<const bn_g2 *>(p.data()), format, out.data(), p.size()));
    return out;
}
inline std::vector<G1> g1_decompress(const std::vector<uint8_t> &records, std::vector<int32_t> &status, int format = BN254_COMPRESSED_ARK) {
    if (records.size() % BN254_G1_COMPRESSED_BYTES) throw std::invalid_argument("g1_decompress: not whole records of 32 bytes");
    std::vector<G1> out(records.size() / BN254_G1_COMPRESSED_BYTES);
    status.assign(out.size(), 0);
    check(bn254_g1_decompress_batch(nullptr, records.data(), format, reinterpret_cast<bn_g1 *>(out.data()), status.data(), out.size()));
    return out;
}
inline std::vector<G2> g2_decompress(const std::vector<uint8_t> &records, std::vector<int32_t> &status, int format = BN254_COMPRESSED_ARK) {
    if (records.size() % BN254_G2_COMPRESSED_BYTES) throw std::invalid_argument("g2_decompress: not whole records of 64 bytes");
    std::vector<G2> out(records.size() / BN254_G2_COMPRESSED_BYTES);
    status.assign(out.size(), 0);
    check(bn254_g2_decompress_batch(nullptr, records.data(), format, reinterpret_cast<bn_g2 *>(out.data()), status.data(), out.size()));
    return out;
}
// Hash to G1 (RFC 9380): the Shallue-van de Woestijne map on 48-byte big-endian integers taken mod q, hash_to_curve = map(u0) + map(u1) from 96
// uniform bytes per record, and the same behind expand_message_xmd over SHA-256 on the device for n messages of one length.  The map's
// constants are derived from the RFC's formulas; not checked against gnark-crypto or any other library.  Results are (x, y, 1), or G::zero()
// where the two maps of a hash cancel
inline std::vector<G1> g1_map_to_curve(const std::vector<uint8_t> &u) {
    if (u.size() % BN254_H2C_FIELD_BYTES) throw std::invalid_argument("g1_map_to_curve: not whole elements of 48 bytes");
    std::vector<G1> out(u.size() / BN254_H2C_FIELD_BYTES);
    check(bn254_g1_map_to_curve_batch(nullptr, u.data(), reinterpret_cast<bn_g1 *>(out.data()), out.size()));
    return out;
}
inline std::vector<G1> g1_hash_to_curve_uniform(const std::vector<uint8_t> &uniform) {
    if (uniform.size() % BN254_H2C_UNIFORM_BYTES) throw std::invalid_argument("g1_hash_to_curve_uniform: not whole records of 96 bytes");
    std::vector<G1> out(uniform.size() / BN254_H2C_UNIFORM_BYTES);
    check(bn254_g1_hash_to_curve_uniform_batch(nullptr, uniform.data(), reinterpret_cast<bn_g1 *>(out.data()), out.size()));
    return out;
}
inline std::vector<G1> g1_hash_to_curve(const std::vector<uint8_t> &msgs, size_t msg_len, size_t n, const std::vector<uint8_t> &dst) {
    if (msgs.size() != n * msg_len) throw std::invalid_argument("g1_hash_to_curve: msgs is not n messages of msg_len bytes");
    std::vector<G1> out(n);
    check(bn254_g1_hash_to_curve_batch(nullptr, msgs.data(), msg_len, dst.data(), dst.size(), reinterpret_cast<bn_g1 *>(out.data()), n));
    return out;
}
// Hash to G2 (RFC 9380 over Fq2): the map on 96-byte elements (c0 then c1) gives points of the twist that are NOT in G2; g2_clear_cofactor takes
// any point of the twist to G2 by [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P), normalised; hash_to_curve = clear(map(u0) + map(u1)) from 192
// uniform bytes per record, and the same behind expand_message_xmd over SHA-256 on the device.  The constants are derived from the RFC's
// formulas and the clearing is the one step the RFC defines no suite for; not checked against gnark-crypto or any other library.
inline std::vector<G2> g2_map_to_curve(const std::vector<uint8_t> &u) {
    if (u.size() % BN254_H2C_G2_FIELD_BYTES) throw std::invalid_argument("g2_map_to_curve: not whole elements of 96 bytes");
    std::vector<G2> out(u.size() / BN254_H2C_G2_FIELD_BYTES);
    check(bn254_g2_map_to_curve_batch(nullptr, u.data(), reinterpret_cast<bn_g2 *>(out.data()), out.size()));
    return out;
}
inline std::vector<G2> g2_clear_cofactor(const std::vector<G2> &p) {
    std::vector<G2> out(p.size());
    check(bn254_g2_clear_cofactor_batch(nullptr, reinterpret_cast<const bn_g2 *>(p.data()), reinterpret_cast<bn_g2 *>(out.data()), p.size()));
    return out;
}
inline std::vector<G2> g2_hash_to_curve_uniform(const std::vector<uint8_t> &uniform) {
    if (uniform.size() % BN254_H2C_G2_UNIFORM_BYTES) throw std::invalid_argument("g2_hash_to_curve_uniform: not whole records of 192 bytes");
    std::vector<G2> out(uniform.size() / BN254_H2C_G2_UNIFORM_BYTES);
    check(bn254_g2_hash_to_curve_uniform_batch(nullptr, uniform.data(), reinterpret_cast<bn_g2 *>(out.data()), out.size()));
    return out;
}
inline std::vector<G2> g2_hash_to_curve(const std::vector<uint8_t> &msgs, size_t msg_len, size_t n, const std::vector<uint8_t> &dst) {
    if (msgs.size() != n * msg_len) throw std::invalid_argument("g2_hash_to_curve: msgs is not n messages of msg_len bytes");
    std::vector<G2> out(n);
    check(bn254_g2_hash_to_curve_batch(nullptr, msgs.data(), msg_len, dst.data(), dst.size(), reinterpret_cast<bn_g2 *>(out.data()), n));
    return out;
}
// Validation of raw points: one status per record with the wire format's numbers (0 valid - infinity, z == 0, included -, 1 a coordinate is not
// below q, 4 not on the curve, 5 on the twist but not in G2: the endomorphism subgroup test).  Every other call trusts its inputs
inline std::vector<int32_t> g1_validate(const std::vector<G1> &p) {
    std::vector<int32_t> status(p.size());
    check(bn254_g1_validate_batch(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), status.data(), p.size()));
    return status;
}
inline std::vector<int32_t> g2_validate(const std::vector<G2> &p) {
    std::vector<int32_t> status(p.size());
    check(bn254_g2_validate_batch(nullptr, reinterpret_cast<const bn_g2 *>(p.data()), status.data(), p.size()));
    return status;
}
// Baby Jubjub (the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr, a = 168700, d = 168696) and EdDSA-Poseidon on it.  A point is two
// consecutive Fr, x then y, affine: a vector of 2 n elements holds n points.  bjj_validate: 0 valid (O = (0, 1) included), 1 a coordinate is not
// below r, 4 not on the curve, 5 on the curve but [l]P != O.  eddsa_poseidon_verify is circomlib's verifyPoseidon: 1 range (S below l included),
// 4 R8 or A not on the curve, 6 [S]B8 != R8 + [8 hm]A, 0 valid; there is NO subgroup check
inline std::vector<int32_t> bjj_validate(const std::vector<Fr> &p) {
    if (p.size() % 2) throw std::invalid_argument("bjj_validate: a point is two Fr");
    std::vector<int32_t> status(p.size() / 2);
    check(bn254_bjj_validate_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), status.data(), status.size()));
    return status;
}
inline std::vector<Fr> bjj_add(const std::vector<Fr> &p, const std::vector<Fr> &q) {
    if (p.size() % 2 || p.size() != q.size()) throw std::invalid_argument("bjj_add: length mismatch");
    std::vector<Fr> out(p.size());
    check(bn254_bjj_add_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), reinterpret_cast<const bn_fr *>(q.data()), reinterpret_cast<bn_fr *>(out.data()), p.size() / 2));
    return out;
}
inline std::vector<Fr> bjj_mul(const std::vector<Fr> &p, const std::vector<Fr> &k) {
    if (p.size() != 2 * k.size()) throw std::invalid_argument("bjj_mul: length mismatch");
    std::vector<Fr> out(p.size());
    check(bn254_bjj_mul_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), reinterpret_cast<bn_fr *>(out.data()), k.size()));
    return out;
}
inline std::vector<Fr> eddsa_poseidon_challenge(const std::vector<Fr> &a, const std::vector<Fr> &r8, const std::vector<Fr> &msg) {
    if (a.size() != 2 * msg.size() || r8.size() != 2 * msg.size()) throw std::invalid_argument("eddsa_poseidon_challenge: length mismatch");
    std::vector<Fr> out(msg.size());
    check(bn254_eddsa_poseidon_challenge_batch(nullptr, reinterpret_cast<const bn_fr *>(a.data()), reinterpret_cast<const bn_fr *>(r8.data()), reinterpret_cast<const bn_fr *>(msg.data()),
                                               reinterpret_cast<bn_fr *>(out.data()), msg.size()));
    return out;
}
inline std::vector<int32_t> eddsa_poseidon_verify(const std::vector<Fr> &a, const std::vector<Fr> &r8, const std::vector<Fr> &s, const std::vector<Fr> &msg) {
    if (a.size() != 2 * msg.size() || r8.size() != 2 * msg.size() || s.size() != msg.size()) throw std::invalid_argument("eddsa_poseidon_verify: length mismatch");
    std::vector<int32_t> status(msg.size());
    check(bn254_eddsa_poseidon_verify_batch(nullptr, reinterpret_cast<const bn_fr *>(a.data()), reinterpret_cast<const bn_fr *>(r8.data()), reinterpret_cast<const bn_fr *>(s.data()),
                                            reinterpret_cast<const bn_fr *>(msg.data()), status.data(), msg.size()));
    return status;
}
// Packed points and signatures (circomlib's packPoint / packSignature): 32 bytes per point - y little endian, the sign of x in the top bit -
// and 64 per signature - the packed R8, then S little endian.  bjj_unpack: 1 y not below r, 4 no point has this y, 3 x == 0 with the sign bit
// set, 0 otherwise; a rejected record gives O.  eddsa_poseidon_verify_packed: 1 range, 4 a point has no x, 3 a non-canonical sign, 6, 0
inline std::vector<uint8_t> bjj_pack(const std::vector<Fr> &p) {
    if (p.size() % 2) throw std::invalid_argument("bjj_pack: a point is two Fr");
    std::vector<uint8_t> out(16 * p.size());
    check(bn254_bjj_pack_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), out.data(), p.size() / 2));
    return out;
}
inline std::pair<std::vector<Fr>, std::vector<int32_t>> bjj_unpack(const std::vector<uint8_t> &in32) {
    if (in32.size() % 32) throw std::invalid_argument("bjj_unpack: a record is 32 bytes");
    std::vector<Fr> out(in32.size() / 16);
    std::vector<int32_t> status(in32.size() / 32);
    check(bn254_bjj_unpack_batch(nullptr, in32.data(), reinterpret_cast<bn_fr *>(out.data()), status.data(), status.size()));
    return {out, status};
}
inline std::vector<int32_t> eddsa_poseidon_verify_packed(const std::vector<uint8_t> &a32, const std::vector<uint8_t> &sig64, const std::vector<Fr> &msg) {
    if (a32.size() != 32 * msg.size() || sig64.size() != 64 * msg.size()) throw std::invalid_argument("eddsa_poseidon_verify_packed: length mismatch");
    std::vector<int32_t> status(msg.size());
    check(bn254_eddsa_poseidon_verify_packed_batch(nullptr, a32.data(), sig64.data(), reinterpret_cast<const bn_fr *>(msg.data()), status.data(), msg.size()));
    return status;
}
// Grumpkin (y^2 = x^3 - 17 over Fr, the other half of the BN254 curve cycle: prime order q, cofactor 1).  A point is two consecutive Fr, x then
// y, affine, infinity (0, 0): a vector of 2 n elements holds n points.  A scalar is 32 bytes, the little-endian integer (any value below 2^256,
// NOT a Montgomery image): a vector of 32 n bytes.  grumpkin_validate: 0 a point of the curve ((0, 0) included), 1 a coordinate is not below r,
// 4 not on the curve; there is no subgroup status
inline std::vector<int32_t> grumpkin_validate(const std::vector<Fr> &p) {
    if (p.size() % 2) throw std::invalid_argument("grumpkin_validate: a point is two Fr");
    std::vector<int32_t> status(p.size() / 2);
    check(bn254_grumpkin_validate_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), status.data(), status.size()));
    return status;
}
inline std::vector<Fr> grumpkin_add(const std::vector<Fr> &p, const std::vector<Fr> &q) {
    if (p.size() % 2 || p.size() != q.size()) throw std::invalid_argument("grumpkin_add: length mismatch");
    std::vector<Fr> out(p.size());
    check(bn254_grumpkin_add_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), reinterpret_cast<const bn_fr *>(q.data()), reinterpret_cast<bn_fr *>(out.data()), p.size() / 2));
    return out;
}
inline std::vector<Fr> grumpkin_mul(const std::vector<Fr> &p, const std::vector<uint8_t> &k32) {
    if (k32.size() % 32 || p.size() != 2 * (k32.size() / 32)) throw std::invalid_argument("grumpkin_mul: length mismatch");
    std::vector<Fr> out(p.size());
    check(bn254_grumpkin_mul_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), k32.data(), reinterpret_cast<bn_fr *>(out.data()), k32.size() / 32));
    return out;
}
// out[j] = sum of [k[t]] p[t] over t in [offsets[j], offsets[j+1]); an empty or cancelling segment gives (0, 0)
inline std::vector<Fr> grumpkin_msm(const std::vector<Fr> &p, const std::vector<uint8_t> &k32, const std::vector<size_t> &offsets) {
    if (offsets.empty() || k32.size() != 32 * offsets.back() || p.size() != 2 * offsets.back()) throw std::invalid_argument("grumpkin_msm: offsets, points and scalars disagree in length");
    std::vector<Fr> out(2 * (offsets.size() - 1));
    check(bn254_grumpkin_msm_batch(nullptr, reinterpret_cast<const bn_fr *>(p.data()), k32.data(), offsets.data(), offsets.size() - 1, reinterpret_cast<bn_fr *>(out.data())));
    return out;
}
// out[i] = (a[i] == b[i]) as group elements, whatever their Jacobian representations (groups/mod.rs:83-109): nothing is normalized
inline std::vector<bool> g1_eq(const std::vector<G1> &a, const std::vector<G1> &b) {
    if (a.size() != b.size()) throw std::invalid_argument("g1_eq: length mismatch");
    std::vector<int32_t> r(a.size());
    check(bn254_g1_eq_batch(nullptr, reinterpret_cast<const bn_g1 *>(a.data()), reinterpret_cast<const bn_g1 *>(b.data()), r.data(), a.size()));
    return std::vector<bool>(r.begin(), r.end());
}
inline std::vector<bool> g2_eq(const std::vector<G2> &a, const std::vector<G2> &b) {
    if (a.size() != b.size()) throw std::invalid_argument("g2_eq: length mismatch");
    std::vector<int32_t> r(a.size());
    check(bn254_g2_eq_batch(nullptr, reinterpret_cast<const bn_g2 *>(a.data()), reinterpret_cast<const bn_g2 *>(b.data()), r.data(), a.size()));
    return std::vector<bool>(r.begin(), r.end());
}
// ok[j] = (product of segment j == Gt::one()): the predicate of a block of pairing checks
inline std::vector<bool> pairing_check_batch(const std::vector<G1> &p, const std::vector<G2> &q, const std::vector<size_t> &offsets) {
    const std::vector<Gt> r = pairing_product_batch(p, q, offsets);
    std::vector<bool> ok(r.size());
    for (size_t j = 0; j < r.size(); ++j) ok[j] = r[j] == Gt::one();
    return ok;
}

// G2 points prepared ONCE for many pairings: the device-resident counterpart of the crate's internal G2Precomp (groups/mod.rs:472-483; `precompute`
// :557-588 runs in the constructor, on the GPU).  One point: shared by every p; several: point i is paired with p[i].
class PreparedG2 {
    bn254_g2_prepared *h_ = nullptr;
public:
    explicit PreparedG2(const std::vector<G2> &q) { check(bn254_g2_prepare(nullptr, reinterpret_cast<const bn_g2 *>(q.data()), q.size(), &h_)); }
    explicit PreparedG2(const G2 &q) { check(bn254_g2_prepare(nullptr, &q.v, 1, &h_)); }
    ~PreparedG2() { bn254_g2_prepared_destroy(h_); }
    PreparedG2(const PreparedG2 &) = delete;
    PreparedG2 &operator=(const PreparedG2 &) = delete;
    size_t size() const { return bn254_g2_prepared_count(h_); }
    size_t device_bytes() const { return bn254_g2_prepared_bytes(h_); }
    // out[i] == bn::pairing(p[i], q) (one prepared point) resp. bn::pairing(p[i], q[i])   (groups/mod.rs:486-519,764-771)
    std::vector<Gt> pairing_batch(const std::vector<G1> &p) const {
        std::vector<Gt> out(p.size());
        check(bn254_pairing_prepared_native_batch(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), h_, reinterpret_cast<bn_gt *>(out.data()), p.size()));
        return out;
    }
    Gt pairing(const G1 &p) const { Gt r; check(bn254_pairing_prepared_native_batch(nullptr, &p.v, h_, &r.v, 1)); return r; }
    // == fold(Gt::one(), acc * bn::pairing(p[i], q[i]))   (shootout/main.rs:11-16): ONE final exponentiation, shared Miller accumulators
    Gt pairing_product(const std::vector<G1> &p) const {
        Gt r;
        check(bn254_pairing_product_prepared_native(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), h_, p.size(), &r.v));
        return r;
    }
    // out[j] = fold(Gt::one(), acc * bn::pairing(p[i], point q_index[i])) over the pairs [offsets[j], offsets[j+1]) (CSR segments, offsets.size() = m + 1):
    // bn::pairing_product_batch with the G2 side prepared, ONE final exponentiation per segment.  q_index empty: pair i uses point i (one prepared point: point 0)
    std::vector<Gt> pairing_product_batch(const std::vector<G1> &p, const std::vector<size_t> &q_index, const std::vector<size_t> &offsets) const {
        if (!q_index.empty() && q_index.size() != p.size()) throw std::invalid_argument("pairing_product_batch: one index per pair");
        if (offsets.empty() || offsets.back() != p.size()) throw std::invalid_argument("pairing_product_batch: offsets must end at the pair count");
        std::vector<Gt> out(offsets.size() - 1);
        check(bn254_pairing_product_batch_prepared_native(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), h_, q_index.empty() ? nullptr : q_index.data(), offsets.data(),
                                                          out.size(), reinterpret_cast<bn_gt *>(out.data())));
        return out;
    }
    // ok[j] = (product of segment j == Gt::one()): a block of Groth16 / EIP-197-style checks against prepared points
    std::vector<bool> pairing_check_batch(const std::vector<G1> &p, const std::vector<size_t> &q_index, const std::vector<size_t> &offsets) const {
        const std::vector<Gt> r = pairing_product_batch(p, q_index, offsets);
        std::vector<bool> ok(r.size());
        for (size_t j = 0; j < r.size(); ++j) ok[j] = r[j] == Gt::one();
        return ok;
    }
};

// Points prepared ONCE for many multi-scalar multiplications (a proving key, an SRS): the handle keeps the affine multiples 2^(c w) P_i in
// device memory.  msm(k, first) == bn::g1_msm / bn::g2_msm over the points [first, first + k.size()) - the same bytes.
// window_bits: 0 for the default of the size, or 3 .. 16.
template <class G>
class PreparedMsm {
    static constexpr bool IS_G1 = sizeof(G) == sizeof(bn_g1);
    void *h_ = nullptr;
public:
    explicit PreparedMsm(const std::vector<G> &p, int window_bits = 0) {
        if constexpr (IS_G1) check(bn254_g1_msm_prepare(nullptr, reinterpret_cast<const bn_g1 *>(p.data()), p.size(), window_bits, &h_));
        else check(bn254_g2_msm_prepare(nullptr, reinterpret_cast<const bn_g2 *>(p.data()), p.size(), window_bits, &h_));
    }
    ~PreparedMsm() { bn254_msm_prepared_destroy(h_); }
    PreparedMsm(const PreparedMsm &) = delete;
    PreparedMsm &operator=(const PreparedMsm &) = delete;
    size_t size() const { return bn254_msm_prepared_count(h_); }
    size_t device_bytes() const { return bn254_msm_prepared_bytes(h_); }
    int group() const { return bn254_msm_prepared_group(h_); }
    int window_bits() const { return bn254_msm_prepared_window_bits(h_); }
    G msm(const std::vector<Fr> &k, size_t first = 0) const {
        G out;
        if constexpr (IS_G1) check(bn254_g1_msm_prepared(nullptr, h_, first, reinterpret_cast<const bn_fr *>(k.data()), k.size(), reinterpret_cast<bn_g1 *>(&out)));
        else check(bn254_g2_msm_prepared(nullptr, h_, first, reinterpret_cast<const bn_fr *>(k.data()), k.size(), reinterpret_cast<bn_g2 *>(&out)));
        return out;
    }
    // device-resident forms, asynchronous on `stream` (bn254_g{1,2}_msm_prepared_dev)
    void msm_dev(size_t first, const void *d_k, size_t n, void *d_out, void *stream = nullptr) const {
        check(IS_G1 ? bn254_g1_msm_prepared_dev(nullptr, h_, first, d_k, n, d_out, stream) : bn254_g2_msm_prepared_dev(nullptr, h_, first, d_k, n, d_out, stream));
    }
    static void *prepare_dev(const void *d_p, size_t n, int window_bits = 0, void *stream = nullptr) {
        void *h = nullptr;
        check(IS_G1 ? bn254_g1_msm_prepare_dev(nullptr, d_p, n, window_bits, &h, stream) : bn254_g2_msm_prepare_dev(nullptr, d_p, n, window_bits, &h, stream));
        return h;
    }
    // the table as W * size() entries of 80 (G1) / 160 (G2) bytes, for tests
    std::vector<unsigned char> export_table() const {
        std::vector<unsigned char> t((size_t)((254 + window_bits() - 1) / window_bits()) * size() * (IS_G1 ? 80 : 160));
        check(bn254_msm_prepared_export(nullptr, h_, t.data(), t.size()));
        return t;
    }
};
typedef PreparedMsm<G1> PreparedMsmG1;
typedef PreparedMsm<G2> PreparedMsmG2;

// tunables of the default context (BN254_OPT_* of bn254_hip.h; value < 0 restores the default derived from the device)
inline void set_option(int key, long value) { check(bn254_ctx_set_option(nullptr, key, value)); }
inline long get_option(int key) { long v = 0; check(bn254_ctx_get_option(nullptr, key, &v)); return v; }

// several GPUs of one node behind one handle (bn254_multi_*): shards of independent pairings, and the multi-pairing product with
// its single 384-byte-per-GPU exchange (RCCL all-gather over xGMI) and ONE final exponentiation
class MultiGpu {
    bn254_multi *m_ = nullptr;
public:
    // exchange: BN254_EXCHANGE_AUTO (RCCL when every rank has its own GPU), _PEER, _RCCL (throws instead of falling back)
    explicit MultiGpu(const std::vector<int> &devices, int exchange = BN254_EXCHANGE_AUTO) { check(bn254_multi_create_ex(devices.data(), (int)devices.size(), exchange, &m_)); }
    void set_option(int key, long value) { check(bn254_multi_set_option(m_, key, value)); }           // BN254_OPT_*, every rank's context
    int rank_numa_node(int rank) const { return bn254_multi_rank_numa_node(m_, rank); }
    ~MultiGpu() { bn254_multi_destroy(m_); }
    MultiGpu(const MultiGpu &) = delete;
    MultiGpu &operator=(const MultiGpu &) = delete;
    bool uses_rccl() const { return bn254_multi_exchange_kind(m_) == BN254_EXCHANGE_RCCL; }
    std::vector<Gt> pairing_batch(const std::vector<G1> &p, const std::vector<G2> &q) {
        if (p.size() != q.size()) throw std::invalid_argument("pairing_batch: length mismatch");
        std::vector<Gt> out(p.size());
        check(bn254_pairing_batch_multi(m_, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_g2 *>(q.data()),
                                        reinterpret_cast<bn_gt *>(out.data()), p.size()));
        return out;
    }
    Gt pairing_product(const std::vector<G1> &p, const std::vector<G2> &q) {
        if (p.size() != q.size()) throw std::invalid_argument("pairing_product: length mismatch");
        Gt r;
        check(bn254_pairing_product_multi(m_, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_g2 *>(q.data()), p.size(), &r.v));
        return r;
    }
    // bn::pairing_product_batch with the segments sharded over the GPUs (no exchange)
    std::vector<Gt> pairing_product_batch(const std::vector<G1> &p, const std::vector<G2> &q, const std::vector<size_t> &offsets) {
        if (p.size() != q.size()) throw std::invalid_argument("pairing_product_batch: length mismatch");
        if (offsets.empty() || offsets.back() != p.size()) throw std::invalid_argument("pairing_product_batch: offsets must end at the pair count");
        std::vector<Gt> out(offsets.size() - 1);
        check(bn254_pairing_product_batch_multi(m_, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_g2 *>(q.data()), offsets.data(),
                                                out.size(), reinterpret_cast<bn_gt *>(out.data())));
        return out;
    }
    // bn::g1_msm_batch / g2_msm_batch with the segments sharded over the GPUs (no exchange)
    std::vector<G1> g1_msm_batch(const std::vector<G1> &p, const std::vector<Fr> &k, const std::vector<size_t> &offsets) {
        if (p.size() != k.size()) throw std::invalid_argument("g1_msm_batch: length mismatch");
        if (offsets.empty() || offsets.back() != p.size()) throw std::invalid_argument("g1_msm_batch: offsets must end at the term count");
        std::vector<G1> out(offsets.size() - 1);
        check(bn254_g1_msm_batch_multi(m_, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), offsets.data(),
                                       out.size(), reinterpret_cast<bn_g1 *>(out.data())));
        return out;
    }
    std::vector<G2> g2_msm_batch(const std::vector<G2> &p, const std::vector<Fr> &k, const std::vector<size_t> &offsets) {
        if (p.size() != k.size()) throw std::invalid_argument("g2_msm_batch: length mismatch");
        if (offsets.empty() || offsets.back() != p.size()) throw std::invalid_argument("g2_msm_batch: offsets must end at the term count");
        std::vector<G2> out(offsets.size() - 1);
        check(bn254_g2_msm_batch_multi(m_, reinterpret_cast<const bn_g2 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), offsets.data(),
                                       out.size(), reinterpret_cast<bn_g2 *>(out.data())));
        return out;
    }
    // bn::g1_msm / g2_msm with the terms sharded over the GPUs; GPU 0 adds the partial sums
    G1 g1_msm(const std::vector<G1> &p, const std::vector<Fr> &k) {
        if (p.size() != k.size()) throw std::invalid_argument("g1_msm: length mismatch");
        G1 out;
        check(bn254_g1_msm_multi(m_, reinterpret_cast<const bn_g1 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), p.size(), reinterpret_cast<bn_g1 *>(&out)));
        return out;
    }
    G2 g2_msm(const std::vector<G2> &p, const std::vector<Fr> &k) {
        if (p.size() != k.size()) throw std::invalid_argument("g2_msm: length mismatch");
        G2 out;
        check(bn254_g2_msm_multi(m_, reinterpret_cast<const bn_g2 *>(p.data()), reinterpret_cast<const bn_fr *>(k.data()), p.size(), reinterpret_cast<bn_g2 *>(&out)));
        return out;
    }
};

}  // namespace bn
