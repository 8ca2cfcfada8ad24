//! UNVERIFIED SOURCE (no rustc/cargo in the build image; never compiled).
//!
//! Batch GPU entry points for the `bn` crate (zcash-hackworks/bn v0.4.3) over the C ABI of `include/bn254_hip.h`.
//! `bn::{Fr, G1, G2, Gt}` are `#[repr(C)]` newtype chains down to `[u64; 4]` (src/lib.rs:15-17, 79-81, 122-124, 165-167), so a
//! slice of them is bit-for-bit an array of `bn_fr` / `bn_g1` / `bn_g2` / `bn_gt`: no conversion, no copies beyond the DMA.
//! Results are `==`-equal (and, for `Gt`, byte-equal) to what the crate computes on the CPU.
extern crate bn;

use bn::{Fr, Group, G1, G2, Gt};          // Group: `zero()` / `one()` of G1 and G2 are trait methods (src/lib.rs:56-77)
use std::os::raw::{c_int, c_long, c_void};

extern "C" {
    fn bn254_pairing_batch(ctx: *mut c_void, p: *const G1, q: *const G2, out: *mut Gt, n: usize) -> c_int;
    fn bn254_pairing_product(ctx: *mut c_void, p: *const G1, q: *const G2, n: usize, out: *mut Gt) -> c_int;
    fn bn254_g1_mul_batch(ctx: *mut c_void, p: *const G1, k: *const Fr, out: *mut G1, n: usize) -> c_int;
    fn bn254_g2_mul_batch(ctx: *mut c_void, p: *const G2, k: *const Fr, out: *mut G2, n: usize) -> c_int;
    fn bn254_gt_mul_batch(ctx: *mut c_void, a: *const Gt, b: *const Gt, out: *mut Gt, n: usize) -> c_int;
    fn bn254_gt_pow_batch(ctx: *mut c_void, a: *const Gt, k: *const Fr, out: *mut Gt, n: usize) -> c_int;
    fn bn254_g1_add_batch(ctx: *mut c_void, a: *const G1, b: *const G1, out: *mut G1, n: usize, negate_b: c_int) -> c_int;
    fn bn254_g2_add_batch(ctx: *mut c_void, a: *const G2, b: *const G2, out: *mut G2, n: usize, negate_b: c_int) -> c_int;
    fn bn254_g1_decode_batch(ctx: *mut c_void, bytes: *const u8, out: *mut G1, status: *mut i32, n: usize) -> c_int;
    fn bn254_g2_decode_batch(ctx: *mut c_void, bytes: *const u8, out: *mut G2, status: *mut i32, n: usize) -> c_int;
    fn bn254_gt_inverse_batch(ctx: *mut c_void, a: *const Gt, out: *mut Gt, n: usize) -> c_int;
    // compressed encodings (x and a sign bit; format: BN254_COMPRESSED_ARK = 0, BN254_COMPRESSED_GNARK = 1)
    fn bn254_g1_compress_batch(ctx: *mut c_void, p: *const G1, format: c_int, out: *mut u8, n: usize) -> c_int;
    fn bn254_g2_compress_batch(ctx: *mut c_void, p: *const G2, format: c_int, out: *mut u8, n: usize) -> c_int;
    fn bn254_g1_decompress_batch(ctx: *mut c_void, bytes: *const u8, format: c_int, out: *mut G1, status: *mut i32, n: usize) -> c_int;
    fn bn254_g2_decompress_batch(ctx: *mut c_void, bytes: *const u8, format: c_int, out: *mut G2, status: *mut i32, n: usize) -> c_int;
    fn bn254_g1_compress_batch_dev(ctx: *mut c_void, d_p: *const c_void, format: c_int, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_compress_batch_dev(ctx: *mut c_void, d_p: *const c_void, format: c_int, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g1_decompress_batch_dev(ctx: *mut c_void, d_in: *const c_void, format: c_int, d_out: *mut c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_decompress_batch_dev(ctx: *mut c_void, d_in: *const c_void, format: c_int, d_out: *mut c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    // hash to G1 (RFC 9380: SvdW map, SHA-256 XMD); `dst` is a host pointer in the _dev form too
    fn bn254_g1_map_to_curve_batch(ctx: *mut c_void, u: *const u8, out: *mut G1, n: usize) -> c_int;
    fn bn254_g1_hash_to_curve_uniform_batch(ctx: *mut c_void, uniform: *const u8, out: *mut G1, n: usize) -> c_int;
    fn bn254_g1_hash_to_curve_batch(ctx: *mut c_void, msgs: *const u8, msg_len: usize, dst: *const u8, dst_len: usize, out: *mut G1, n: usize) -> c_int;
    fn bn254_g1_map_to_curve_batch_dev(ctx: *mut c_void, d_u: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g1_hash_to_curve_uniform_batch_dev(ctx: *mut c_void, d_uniform: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g1_hash_to_curve_batch_dev(ctx: *mut c_void, d_msgs: *const c_void, msg_len: usize, dst: *const u8, dst_len: usize, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_map_to_curve_batch(ctx: *mut c_void, u: *const u8, out: *mut G2, n: usize) -> c_int;
    fn bn254_g2_clear_cofactor_batch(ctx: *mut c_void, p: *const G2, out: *mut G2, n: usize) -> c_int;
    fn bn254_g2_hash_to_curve_uniform_batch(ctx: *mut c_void, uniform: *const u8, out: *mut G2, n: usize) -> c_int;
    fn bn254_g2_hash_to_curve_batch(ctx: *mut c_void, msgs: *const u8, msg_len: usize, dst: *const u8, dst_len: usize, out: *mut G2, n: usize) -> c_int;
    fn bn254_g2_map_to_curve_batch_dev(ctx: *mut c_void, d_u: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_clear_cofactor_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_hash_to_curve_uniform_batch_dev(ctx: *mut c_void, d_uniform: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_hash_to_curve_batch_dev(ctx: *mut c_void, d_msgs: *const c_void, msg_len: usize, dst: *const u8, dst_len: usize, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    // validation of raw points: one status per record (0 valid, 1 range, 4 not on the curve, 5 not in the subgroup)
    fn bn254_g1_validate_batch(ctx: *mut c_void, p: *const G1, status: *mut i32, n: usize) -> c_int;
    fn bn254_g2_validate_batch(ctx: *mut c_void, p: *const G2, status: *mut i32, n: usize) -> c_int;
    fn bn254_g1_validate_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_validate_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_bjj_validate_batch(ctx: *mut c_void, p: *const Fr, status: *mut i32, n: usize) -> c_int;
    fn bn254_bjj_add_batch(ctx: *mut c_void, p: *const Fr, q: *const Fr, out: *mut Fr, n: usize) -> c_int;
    fn bn254_bjj_mul_batch(ctx: *mut c_void, p: *const Fr, k: *const Fr, out: *mut Fr, n: usize) -> c_int;
    fn bn254_eddsa_poseidon_challenge_batch(ctx: *mut c_void, a: *const Fr, r8: *const Fr, msg: *const Fr, out: *mut Fr, n: usize) -> c_int;
    fn bn254_eddsa_poseidon_verify_batch(ctx: *mut c_void, a: *const Fr, r8: *const Fr, s: *const Fr, msg: *const Fr, status: *mut i32, n: usize) -> c_int;
    fn bn254_bjj_validate_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_bjj_add_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_q: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_bjj_mul_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_k: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_eddsa_poseidon_challenge_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_r8: *const c_void, d_msg: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_eddsa_poseidon_verify_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_r8: *const c_void, d_s: *const c_void, d_msg: *const c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_bjj_pack_batch(ctx: *mut c_void, p: *const Fr, out32: *mut u8, n: usize) -> c_int;
    fn bn254_bjj_unpack_batch(ctx: *mut c_void, in32: *const u8, out: *mut Fr, status: *mut i32, n: usize) -> c_int;
    fn bn254_eddsa_poseidon_verify_packed_batch(ctx: *mut c_void, a32: *const u8, sig64: *const u8, msg: *const Fr, status: *mut i32, n: usize) -> c_int;
    fn bn254_bjj_pack_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_out32: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_bjj_unpack_batch_dev(ctx: *mut c_void, d_in32: *const c_void, d_out: *mut c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_eddsa_poseidon_verify_packed_batch_dev(ctx: *mut c_void, d_a32: *const c_void, d_sig64: *const c_void, d_msg: *const c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_grumpkin_validate_batch(ctx: *mut c_void, p: *const Fr, status: *mut i32, n: usize) -> c_int;
    fn bn254_grumpkin_add_batch(ctx: *mut c_void, p: *const Fr, q: *const Fr, out: *mut Fr, n: usize) -> c_int;
    fn bn254_grumpkin_mul_batch(ctx: *mut c_void, p: *const Fr, k32: *const u8, out: *mut Fr, n: usize) -> c_int;
    fn bn254_grumpkin_msm_batch(ctx: *mut c_void, p: *const Fr, k32: *const u8, offsets: *const usize, m: usize, out: *mut Fr) -> c_int;
    fn bn254_grumpkin_validate_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_status: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_grumpkin_add_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_q: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_grumpkin_mul_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_k32: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_grumpkin_msm_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_k32: *const c_void, offsets: *const usize, m: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    // prepared-G2 mode (the crate's internal G2Precomp, src/groups/mod.rs:472-483): 102 line coefficients per Q, then many P against them
    fn bn254_g2_precompute(ctx: *mut c_void, q: *const G2, coeffs: *mut EllCoeffs, n: usize) -> c_int;
    fn bn254_pairing_prepared_batch(ctx: *mut c_void, p: *const G1, coeffs: *const EllCoeffs, shared: c_int, out: *mut Gt, n: usize) -> c_int;
    // native prepared-G2 mode: the device-resident counterpart of G2Precomp behind an opaque handle (include/bn254_hip.h bn254_g2_prepare)
    fn bn254_g2_prepare(ctx: *mut c_void, q: *const G2, nq: usize, out: *mut *mut c_void) -> c_int;
    fn bn254_g2_prepared_destroy(prep: *mut c_void);
    fn bn254_g2_prepared_count(prep: *const c_void) -> usize;
    fn bn254_g2_prepared_bytes(prep: *const c_void) -> usize;
    fn bn254_pairing_prepared_native_batch(ctx: *mut c_void, p: *const G1, prep: *const c_void, out: *mut Gt, n: usize) -> c_int;
    fn bn254_pairing_product_prepared_native(ctx: *mut c_void, p: *const G1, prep: *const c_void, n: usize, out: *mut Gt) -> c_int;
    fn bn254_pairing_product_batch_prepared_native(ctx: *mut c_void, p: *const G1, prep: *const c_void, q_index: *const usize, offsets: *const usize, m: usize, out: *mut Gt) -> c_int;
    fn bn254_pairing_product_batch_prepared_native_dev(ctx: *mut c_void, d_p: *const c_void, prep: *const c_void, d_q_index: *const c_void, offsets: *const usize, m: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    // wire format of the crate's Encodable / Decodable impls (src/groups/mod.rs:143-205, src/fields/fp.rs:24-36), fixed-size records and the stream
    fn bn254_fr_encode_batch(ctx: *mut c_void, k: *const Fr, out: *mut u8, n: usize) -> c_int;
    fn bn254_fr_decode_batch(ctx: *mut c_void, bytes: *const u8, out: *mut Fr, status: *mut i32, n: usize) -> c_int;
    fn bn254_g1_encode_batch(ctx: *mut c_void, p: *const G1, out: *mut u8, n: usize) -> c_int;
    fn bn254_g2_encode_batch(ctx: *mut c_void, p: *const G2, out: *mut u8, n: usize) -> c_int;
    fn bn254_g1_encode_stream(ctx: *mut c_void, p: *const G1, n: usize, out: *mut u8, cap: usize, written: *mut usize) -> c_int;
    fn bn254_g2_encode_stream(ctx: *mut c_void, p: *const G2, n: usize, out: *mut u8, cap: usize, written: *mut usize) -> c_int;
    fn bn254_g1_decode_stream(ctx: *mut c_void, bytes: *const u8, len: usize, out: *mut G1, status: *mut i32, max_points: usize, count: *mut usize, consumed: *mut usize) -> c_int;
    fn bn254_g2_decode_stream(ctx: *mut c_void, bytes: *const u8, len: usize, out: *mut G2, status: *mut i32, max_points: usize, count: *mut usize, consumed: *mut usize) -> c_int;
    // one node, several GPUs (include/bn254_hip.h "bn254_multi"): one context + host thread per device inside the library
    fn bn254_multi_create(devices: *const c_int, ndev: c_int, out: *mut *mut c_void) -> c_int;
    fn bn254_multi_create_ex(devices: *const c_int, ndev: c_int, exchange: c_int, out: *mut *mut c_void) -> c_int;     // -1 auto, 0 peer copies, 1 RCCL
    fn bn254_multi_set_option(m: *mut c_void, key: c_int, value: c_long) -> c_int;
    fn bn254_multi_rank_numa_node(m: *const c_void, rank: c_int) -> c_int;
    // tunables of a context (NULL = the default context of the current device): BN254_OPT_* of include/bn254_hip.h; value < 0 = default
    fn bn254_ctx_set_option(ctx: *mut c_void, key: c_int, value: c_long) -> c_int;
    fn bn254_ctx_get_option(ctx: *mut c_void, key: c_int, value: *mut c_long) -> c_int;
    fn bn254_ctx_get_option_raw(ctx: *mut c_void, key: c_int, value: *mut c_long) -> c_int;
    fn bn254_multi_destroy(m: *mut c_void);
    fn bn254_g2_prepare_multi(m: *mut c_void, q: *const G2, nq: usize, out: *mut *mut c_void) -> c_int;
    fn bn254_multi_prepared_destroy(prep: *mut c_void);
    fn bn254_multi_prepared_count(prep: *const c_void) -> usize;
    fn bn254_pairing_prepared_native_batch_multi(m: *mut c_void, p: *const G1, prep: *const c_void, out: *mut Gt, n: usize) -> c_int;
    fn bn254_pairing_product_prepared_native_multi(m: *mut c_void, p: *const G1, prep: *const c_void, n: usize, out: *mut Gt) -> c_int;
    fn bn254_pairing_batch_multi(m: *mut c_void, p: *const G1, q: *const G2, out: *mut Gt, n: usize) -> c_int;
    fn bn254_pairing_product_multi(m: *mut c_void, p: *const G1, q: *const G2, n: usize, out: *mut Gt) -> c_int;
    fn bn254_pairing_product_batch(ctx: *mut c_void, p: *const G1, q: *const G2, offsets: *const usize, m: usize, out: *mut Gt) -> c_int;
    fn bn254_pairing_product_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_q: *const c_void, offsets: *const usize, m: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_pairing_product_batch_multi(mh: *mut c_void, p: *const G1, q: *const G2, offsets: *const usize, m: usize, out: *mut Gt) -> c_int;
    fn bn254_g1_msm_batch(ctx: *mut c_void, p: *const G1, k: *const Fr, offsets: *const usize, m: usize, out: *mut G1) -> c_int;
    fn bn254_g2_msm_batch(ctx: *mut c_void, p: *const G2, k: *const Fr, offsets: *const usize, m: usize, out: *mut G2) -> c_int;
    fn bn254_g1_msm_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_k: *const c_void, offsets: *const usize, m: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_g2_msm_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_k: *const c_void, offsets: *const usize, m: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_g1_msm_batch_multi(mh: *mut c_void, p: *const G1, k: *const Fr, offsets: *const usize, m: usize, out: *mut G1) -> c_int;
    fn bn254_g2_msm_batch_multi(mh: *mut c_void, p: *const G2, k: *const Fr, offsets: *const usize, m: usize, out: *mut G2) -> c_int;
    fn bn254_g1_msm(ctx: *mut c_void, p: *const G1, k: *const Fr, n: usize, out: *mut G1) -> c_int;
    fn bn254_g2_msm(ctx: *mut c_void, p: *const G2, k: *const Fr, n: usize, out: *mut G2) -> c_int;
    fn bn254_g1_msm_dev(ctx: *mut c_void, d_p: *const c_void, d_k: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_g2_msm_dev(ctx: *mut c_void, d_p: *const c_void, d_k: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_g1_msm_prepare(ctx: *mut c_void, p: *const G1, n: usize, window_bits: c_int, out: *mut *mut c_void) -> c_int;
    fn bn254_g2_msm_prepare(ctx: *mut c_void, p: *const G2, n: usize, window_bits: c_int, out: *mut *mut c_void) -> c_int;
    fn bn254_g1_msm_prepare_dev(ctx: *mut c_void, d_p: *const c_void, n: usize, window_bits: c_int, out: *mut *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_g2_msm_prepare_dev(ctx: *mut c_void, d_p: *const c_void, n: usize, window_bits: c_int, out: *mut *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_msm_prepared_destroy(prep: *mut c_void);
    fn bn254_msm_prepared_count(prep: *const c_void) -> usize;
    fn bn254_msm_prepared_bytes(prep: *const c_void) -> usize;
    fn bn254_msm_prepared_group(prep: *const c_void) -> c_int;
    fn bn254_msm_prepared_window_bits(prep: *const c_void) -> c_int;
    fn bn254_msm_prepared_export(ctx: *mut c_void, prep: *const c_void, host_table: *mut c_void, bytes: usize) -> c_int;
    fn bn254_g1_msm_prepared(ctx: *mut c_void, prep: *const c_void, first: usize, k: *const Fr, n: usize, out: *mut G1) -> c_int;
    fn bn254_g2_msm_prepared(ctx: *mut c_void, prep: *const c_void, first: usize, k: *const Fr, n: usize, out: *mut G2) -> c_int;
    fn bn254_g1_msm_prepared_dev(ctx: *mut c_void, prep: *const c_void, first: usize, d_k: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_g2_msm_prepared_dev(ctx: *mut c_void, prep: *const c_void, first: usize, d_k: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_g1_msm_multi(mh: *mut c_void, p: *const G1, k: *const Fr, n: usize, out: *mut G1) -> c_int;
    fn bn254_g2_msm_multi(mh: *mut c_void, p: *const G2, k: *const Fr, n: usize, out: *mut G2) -> c_int;
    fn bn254_g1_mul_base_batch(ctx: *mut c_void, base: *const G1, k: *const Fr, out: *mut G1, n: usize) -> c_int;
    fn bn254_g2_mul_base_batch(ctx: *mut c_void, base: *const G2, k: *const Fr, out: *mut G2, n: usize) -> c_int;
    fn bn254_g1_mul_base_batch_dev(ctx: *mut c_void, base: *const G1, d_k: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_mul_base_batch_dev(ctx: *mut c_void, base: *const G2, d_k: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g1_normalize_batch(ctx: *mut c_void, p: *const G1, out: *mut G1, n: usize) -> c_int;
    fn bn254_g2_normalize_batch(ctx: *mut c_void, p: *const G2, out: *mut G2, n: usize) -> c_int;
    fn bn254_g1_eq_batch(ctx: *mut c_void, a: *const G1, b: *const G1, out: *mut i32, n: usize) -> c_int;
    fn bn254_g2_eq_batch(ctx: *mut c_void, a: *const G2, b: *const G2, out: *mut i32, n: usize) -> c_int;
    fn bn254_g1_normalize_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_normalize_batch_dev(ctx: *mut c_void, d_p: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g1_eq_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_b: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_g2_eq_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_b: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_add_batch(ctx: *mut c_void, a: *const Fr, b: *const Fr, out: *mut Fr, n: usize, negate_b: c_int) -> c_int;
    fn bn254_fr_mul_batch(ctx: *mut c_void, a: *const Fr, b: *const Fr, out: *mut Fr, n: usize) -> c_int;
    fn bn254_fr_inverse_batch(ctx: *mut c_void, a: *const Fr, out: *mut Fr, ok: *mut i32, n: usize) -> c_int;
    fn bn254_fr_pow_batch(ctx: *mut c_void, a: *const Fr, e: *const Fr, out: *mut Fr, n: usize) -> c_int;
    fn bn254_fr_interpret_batch(ctx: *mut c_void, bytes: *const u8, out: *mut Fr, n: usize) -> c_int;
    fn bn254_fr_sqrt_batch(ctx: *mut c_void, a: *const Fr, out: *mut Fr, ok: *mut i32, n: usize) -> c_int;
    fn bn254_fr_root_of_unity(log_n: c_int, out: *mut Fr) -> c_int;
    fn bn254_fr_ntt_batch(ctx: *mut c_void, input: *const Fr, out: *mut Fr, log_n: c_int, count: usize, inverse: c_int, shift: *const Fr) -> c_int;
    fn bn254_fr_dot_batch(ctx: *mut c_void, coeff: *const Fr, index: *const u64, x: *const Fr, nx: usize, offsets: *const usize, m: usize, out: *mut Fr) -> c_int;
    fn bn254_fr_scan_batch(ctx: *mut c_void, a: *const Fr, b: *const Fr, init: *const Fr, offsets: *const usize, m: usize, flags: c_int, out: *mut Fr) -> c_int;
    fn bn254_fr_mle_eq(ctx: *mut c_void, z: *const Fr, nv: c_int, out: *mut Fr) -> c_int;
    fn bn254_fr_mle_fold(ctx: *mut c_void, input: *const Fr, len: usize, r: *const Fr, out: *mut Fr) -> c_int;
    fn bn254_fr_sumcheck_round(ctx: *mut c_void, tables: *const Fr, n: usize, k: usize, group_offsets: *const usize, group_tables: *const u64, group_coeff: *const Fr, g: usize, degree: c_int, out: *mut Fr) -> c_int;
    fn bn254_fr_sumcheck_fold_round(ctx: *mut c_void, tables: *const Fr, n: usize, k: usize, r: *const Fr, group_offsets: *const usize, group_tables: *const u64, group_coeff: *const Fr, g: usize, degree: c_int, folded: *mut Fr, out: *mut Fr) -> c_int;
    fn bn254_fr_mle_quotients(ctx: *mut c_void, a: *const Fr, nv: c_int, z: *const Fr, out: *mut Fr) -> c_int;
    fn bn254_fr_poseidon_batch(ctx: *mut c_void, input: *const Fr, arity: c_int, out: *mut Fr, n: usize) -> c_int;
    fn bn254_fr_poseidon_permute_batch(ctx: *mut c_void, input: *const Fr, t: c_int, out: *mut Fr, n: usize) -> c_int;
    fn bn254_fr_merkle_tree(ctx: *mut c_void, leaves: *const Fr, log_n: c_int, nodes: *mut Fr) -> c_int;
    fn bn254_fr_poseidon_ex_batch(ctx: *mut c_void, input: *const Fr, n_inputs: c_int, init: *const Fr, n_outs: c_int, out: *mut Fr, n: usize) -> c_int;
    fn bn254_fr_poseidon_chain_batch(ctx: *mut c_void, input: *const Fr, offsets: *const usize, m: usize, rate: c_int, out: *mut Fr) -> c_int;
    fn bn254_fr_add_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_b: *const c_void, d_out: *mut c_void, n: usize, negate_b: c_int, stream: *mut c_void) -> c_int;
    fn bn254_fr_mul_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_b: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_inverse_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_out: *mut c_void, d_ok: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_pow_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_e: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_interpret_batch_dev(ctx: *mut c_void, d_in: *const c_void, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_sqrt_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_out: *mut c_void, d_ok: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_ntt_batch_dev(ctx: *mut c_void, d_in: *const c_void, d_out: *mut c_void, log_n: c_int, count: usize, inverse: c_int, shift: *const Fr, stream: *mut c_void) -> c_int;
    fn bn254_g1_ntt_batch(ctx: *mut c_void, input: *const G1, out: *mut G1, log_n: c_int, count: usize, inverse: c_int, shift: *const Fr) -> c_int;
    fn bn254_g2_ntt_batch(ctx: *mut c_void, input: *const G2, out: *mut G2, log_n: c_int, count: usize, inverse: c_int, shift: *const Fr) -> c_int;
    fn bn254_g1_ntt_batch_dev(ctx: *mut c_void, d_in: *const c_void, d_out: *mut c_void, log_n: c_int, count: usize, inverse: c_int, shift: *const Fr, stream: *mut c_void) -> c_int;
    fn bn254_g2_ntt_batch_dev(ctx: *mut c_void, d_in: *const c_void, d_out: *mut c_void, log_n: c_int, count: usize, inverse: c_int, shift: *const Fr, stream: *mut c_void) -> c_int;
    fn bn254_fr_dot_batch_dev(ctx: *mut c_void, d_coeff: *const c_void, d_index: *const c_void, d_x: *const c_void, nx: usize, offsets: *const usize, m: usize, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_scan_batch_dev(ctx: *mut c_void, d_a: *const c_void, d_b: *const c_void, d_init: *const c_void, offsets: *const usize, m: usize, flags: c_int, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_mle_eq_dev(ctx: *mut c_void, d_z: *const c_void, nv: c_int, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_mle_fold_dev(ctx: *mut c_void, d_in: *const c_void, len: usize, r: *const Fr, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_sumcheck_round_dev(ctx: *mut c_void, d_tables: *const c_void, n: usize, k: usize, group_offsets: *const usize, group_tables: *const u64, group_coeff: *const Fr, g: usize, degree: c_int, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_sumcheck_fold_round_dev(ctx: *mut c_void, d_tables: *const c_void, n: usize, k: usize, r: *const Fr, group_offsets: *const usize, group_tables: *const u64, group_coeff: *const Fr, g: usize, degree: c_int, d_folded: *mut c_void, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_mle_quotients_dev(ctx: *mut c_void, d_a: *const c_void, nv: c_int, z: *const Fr, d_out: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_poseidon_batch_dev(ctx: *mut c_void, d_in: *const c_void, arity: c_int, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_poseidon_permute_batch_dev(ctx: *mut c_void, d_in: *const c_void, t: c_int, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_merkle_tree_dev(ctx: *mut c_void, d_leaves: *const c_void, log_n: c_int, d_nodes: *mut c_void, stream: *mut c_void) -> c_int;
    fn bn254_fr_poseidon_ex_batch_dev(ctx: *mut c_void, d_in: *const c_void, n_inputs: c_int, d_init: *const c_void, n_outs: c_int, d_out: *mut c_void, n: usize, stream: *mut c_void) -> c_int;
    fn bn254_fr_poseidon_chain_batch_dev(ctx: *mut c_void, d_in: *const c_void, offsets: *const usize, m: usize, rate: c_int, d_out: *mut c_void, stream: *mut c_void) -> c_int;
}

/// One line-function coefficient of a prepared G2 point: the crate's `EllCoeffs { ell_0, ell_vw, ell_vv: Fq2 }` (src/groups/mod.rs:472-476) as the
/// C ABI lays it out (`bn_ell_coeffs`: three Fq2 = 3 x 8 u64 Montgomery limbs); the crate keeps the type private, so the binding carries its own.
#[derive(Clone, Copy)]
#[repr(C)]
pub struct EllCoeffs { pub ell_0: [u64; 8], pub ell_vw: [u64; 8], pub ell_vv: [u64; 8] }
/// `BN254_PREPARED_COEFFS` of include/bn254_hip.h: coefficients per prepared point (G2Precomp.coeffs, src/groups/mod.rs:478-483)
pub const PREPARED_COEFFS: usize = 102;
/// `BN254_PREPARED_NATIVE_LINES` / `BN254_PREPARED_NATIVE_BYTES`: lines and device bytes per point of a `PreparedG2`
pub const PREPARED_NATIVE_LINES: usize = 88;
pub const PREPARED_NATIVE_BYTES: usize = 33792;
/// `BN254_FR_WIRE_BYTES` / `BN254_G1_WIRE_BYTES` / `BN254_G2_WIRE_BYTES`
pub const FR_WIRE_BYTES: usize = 32;
pub const G1_WIRE_BYTES: usize = 65;
pub const G2_WIRE_BYTES: usize = 129;

// Thread safety: every host-buffer entry point of the C ABI may be called from any number of threads on one context (including the
// process-wide default context behind a NULL ctx), like the crate's own `pairing` (its types are `Send + Sync`,
// src/lib.rs:55-61): the batch entry points lease one of two pipeline slots per call (two callers overlap on the GPU, more queue),
// the others lock the context for the call.

/// `BN254_OPT_*` of include/bn254_hip.h: per-context policies whose defaults derive from the device's CU count
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
#[repr(i32)]
pub enum GpuOption {
    WavePairingMax = 1, WaveFeMax = 2, QuadMax = 3, MillerShared = 4, GtPowMode = 5, ProductChunk = 6, ProductPerWave = 7,
    ProductBfly = 8, RoundPairs = 9, PipelineChunk = 10, PipelineSlots = 11, StreamStopAtError = 12,
    MsmBucketMin = 13, MsmWindowBits = 14, MsmChunk = 15,
}
/// sets an option of the process-wide default context of the current HIP device; `None` restores the default
pub fn set_option(key: GpuOption, value: Option<i64>) -> Result<(), GpuError> {
    check(unsafe { bn254_ctx_set_option(std::ptr::null_mut(), key as c_int, value.unwrap_or(-1) as c_long) })
}
/// the explicitly set value of an option of the default context, `None` while its default is in effect
pub fn get_option_raw(key: GpuOption) -> Result<Option<i64>, GpuError> {
    let mut v: c_long = 0;
    check(unsafe { bn254_ctx_get_option_raw(std::ptr::null_mut(), key as c_int, &mut v) })?;
    Ok(if v < 0 { None } else { Some(v as i64) })
}
/// the effective value of an option of the default context
pub fn get_option(key: GpuOption) -> Result<i64, GpuError> {
    let mut v: c_long = 0;
    check(unsafe { bn254_ctx_get_option(std::ptr::null_mut(), key as c_int, &mut v) })?;
    Ok(v as i64)
}

/// Error code of the HIP engine: negative `BN254_E_*`, positive `hipError_t`.  There is no CPU fallback.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct GpuError(pub i32);

fn check(rc: c_int) -> Result<(), GpuError> { if rc == 0 { Ok(()) } else { Err(GpuError(rc)) } }

/// `out[i] = bn::pairing(p[i], q[i])` (src/lib.rs:181-183)
pub fn pairing_batch(p: &[G1], q: &[G2]) -> Result<Vec<Gt>, GpuError> {
    assert_eq!(p.len(), q.len());
    let mut out = vec![Gt::one(); p.len()];
    check(unsafe { bn254_pairing_batch(std::ptr::null_mut(), p.as_ptr(), q.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

/// `fold(Gt::one(), |acc, (p, q)| acc * pairing(p, q))` (shootout/main.rs:11-16) with a single final exponentiation
pub fn pairing_product(p: &[G1], q: &[G2]) -> Result<Gt, GpuError> {
    assert_eq!(p.len(), q.len());
    let mut out = Gt::one();
    check(unsafe { bn254_pairing_product(std::ptr::null_mut(), p.as_ptr(), q.as_ptr(), p.len(), &mut out) })?;
    Ok(out)
}

/// `out[j]` = that fold over the pairs `offsets[j]..offsets[j+1]` (CSR segments, `offsets.len()` = m + 1): many independent
/// multi-pairings in one call, ONE final exponentiation per segment; an empty segment gives `Gt::one()`
pub fn pairing_product_batch(p: &[G1], q: &[G2], offsets: &[usize]) -> Result<Vec<Gt>, GpuError> {
    assert_eq!(p.len(), q.len());
    assert!(!offsets.is_empty() && offsets[offsets.len() - 1] == p.len());
    let mut out = vec![Gt::one(); offsets.len() - 1];
    check(unsafe { bn254_pairing_product_batch(std::ptr::null_mut(), p.as_ptr(), q.as_ptr(), offsets.as_ptr(), out.len(), out.as_mut_ptr()) })?;
    Ok(out)
}

/// `ok[j]` = (product of segment j == `Gt::one()`): a block of Groth16 / EIP-197-style pairing checks
pub fn pairing_check_batch(p: &[G1], q: &[G2], offsets: &[usize]) -> Result<Vec<bool>, GpuError> {
    Ok(pairing_product_batch(p, q, offsets)?.into_iter().map(|g| g == Gt::one()).collect())
}

/// `out[i] = p[i] * k[i]`, returned normalized (src/lib.rs:88-95): equal to the crate's result under its projective `==`
pub fn g1_mul_batch(p: &[G1], k: &[Fr]) -> Result<Vec<G1>, GpuError> {
    assert_eq!(p.len(), k.len());
    let mut out = p.to_vec();
    check(unsafe { bn254_g1_mul_batch(std::ptr::null_mut(), p.as_ptr(), k.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

pub fn g2_mul_batch(p: &[G2], k: &[Fr]) -> Result<Vec<G2>, GpuError> {
    assert_eq!(p.len(), k.len());
    let mut out = p.to_vec();
    check(unsafe { bn254_g2_mul_batch(std::ptr::null_mut(), p.as_ptr(), k.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

/// `out[j]` = normalized sum of `p[i] * k[i]` over the terms `offsets[j]..offsets[j+1]` (CSR segments, `offsets.len()` = m + 1): many
/// independent multi-scalar multiplications in one call, ONE inversion per segment; an empty or cancelling segment gives `G1::zero()`
pub fn g1_msm_batch(p: &[G1], k: &[Fr], offsets: &[usize]) -> Result<Vec<G1>, GpuError> {
    assert_eq!(p.len(), k.len());
    assert!(!offsets.is_empty() && offsets[offsets.len() - 1] == p.len());
    let mut out = vec![G1::zero(); offsets.len() - 1];
    check(unsafe { bn254_g1_msm_batch(std::ptr::null_mut(), p.as_ptr(), k.as_ptr(), offsets.as_ptr(), out.len(), out.as_mut_ptr()) })?;
    Ok(out)
}

pub fn g2_msm_batch(p: &[G2], k: &[Fr], offsets: &[usize]) -> Result<Vec<G2>, GpuError> {
    assert_eq!(p.len(), k.len());
    assert!(!offsets.is_empty() && offsets[offsets.len() - 1] == p.len());
    let mut out = vec![G2::zero(); offsets.len() - 1];
    check(unsafe { bn254_g2_msm_batch(std::ptr::null_mut(), p.as_ptr(), k.as_ptr(), offsets.as_ptr(), out.len(), out.as_mut_ptr()) })?;
    Ok(out)
}

/// the normalized sum of `p[i] * k[i]` over ALL terms: one large multi-scalar multiplication - the bucket (Pippenger) method from
/// `GpuOption::MsmBucketMin` terms on, below it the one-segment `g1_msm_batch`; the same bytes either way, `G1::zero()` for an empty or
/// cancelling sum
pub fn g1_msm(p: &[G1], k: &[Fr]) -> Result<G1, GpuError> {
    assert_eq!(p.len(), k.len());
    let mut out = G1::zero();
    check(unsafe { bn254_g1_msm(std::ptr::null_mut(), p.as_ptr(), k.as_ptr(), p.len(), &mut out) })?;
    Ok(out)
}

pub fn g2_msm(p: &[G2], k: &[Fr]) -> Result<G2, GpuError> {
    assert_eq!(p.len(), k.len());
    let mut out = G2::zero();
    check(unsafe { bn254_g2_msm(std::ptr::null_mut(), p.as_ptr(), k.as_ptr(), p.len(), &mut out) })?;
    Ok(out)
}

/// Points a prover multiplies fresh scalars against, call after call (a proving key, an SRS), prepared once: the handle keeps the affine
/// multiples `2^(c w) P_i` in device memory, and `msm(first, k)` is `normalize(sum P[first + i] * k[i])` - the bytes of `g1_msm` / `g2_msm`
/// on the same points and scalars.  `window_bits`: 0 for the default of the size, or 3..=16.
pub struct PreparedMsmG1(*mut c_void);
unsafe impl Send for PreparedMsmG1 {}
unsafe impl Sync for PreparedMsmG1 {}
impl PreparedMsmG1 {
    pub fn new(p: &[G1], window_bits: i32) -> Result<PreparedMsmG1, GpuError> {
        let mut h = std::ptr::null_mut();
        check(unsafe { bn254_g1_msm_prepare(std::ptr::null_mut(), p.as_ptr(), p.len(), window_bits, &mut h) })?;
        Ok(PreparedMsmG1(h))
    }
    pub fn len(&self) -> usize { unsafe { bn254_msm_prepared_count(self.0) } }
    pub fn device_bytes(&self) -> usize { unsafe { bn254_msm_prepared_bytes(self.0) } }
    pub fn window_bits(&self) -> i32 { unsafe { bn254_msm_prepared_window_bits(self.0) } }
    pub fn msm(&self, first: usize, k: &[Fr]) -> Result<G1, GpuError> {
        let mut out = G1::zero();
        check(unsafe { bn254_g1_msm_prepared(std::ptr::null_mut(), self.0, first, k.as_ptr(), k.len(), &mut out) })?;
        Ok(out)
    }
}
impl Drop for PreparedMsmG1 {
    fn drop(&mut self) { unsafe { bn254_msm_prepared_destroy(self.0) } }
}
pub struct PreparedMsmG2(*mut c_void);
unsafe impl Send for PreparedMsmG2 {}
unsafe impl Sync for PreparedMsmG2 {}
impl PreparedMsmG2 {
    pub fn new(p: &[G2], window_bits: i32) -> Result<PreparedMsmG2, GpuError> {
        let mut h = std::ptr::null_mut();
        check(unsafe { bn254_g2_msm_prepare(std::ptr::null_mut(), p.as_ptr(), p.len(), window_bits, &mut h) })?;
        Ok(PreparedMsmG2(h))
    }
    pub fn len(&self) -> usize { unsafe { bn254_msm_prepared_count(self.0) } }
    pub fn device_bytes(&self) -> usize { unsafe { bn254_msm_prepared_bytes(self.0) } }
    pub fn window_bits(&self) -> i32 { unsafe { bn254_msm_prepared_window_bits(self.0) } }
    pub fn msm(&self, first: usize, k: &[Fr]) -> Result<G2, GpuError> {
        let mut out = G2::zero();
        check(unsafe { bn254_g2_msm_prepared(std::ptr::null_mut(), self.0, first, k.as_ptr(), k.len(), &mut out) })?;
        Ok(out)
    }
}
impl Drop for PreparedMsmG2 {
    fn drop(&mut self) { unsafe { bn254_msm_prepared_destroy(self.0) } }
}

/// `out[i] = (base * k[i]).normalize()`: fixed-base scalar multiplication - many scalars against ONE point (key and SRS generation,
/// `G::random`).  The same bytes as `g1_mul_batch` on `k.len()` copies of `base`; the context keeps a table of multiples of the four most
/// recently used bases per group, after which a product is at most 22 mixed additions
pub fn g1_mul_base(base: &G1, k: &[Fr]) -> Result<Vec<G1>, GpuError> {
    let mut out = vec![G1::zero(); k.len()];
    check(unsafe { bn254_g1_mul_base_batch(std::ptr::null_mut(), base, k.as_ptr(), out.as_mut_ptr(), k.len()) })?;
    Ok(out)
}

pub fn g2_mul_base(base: &G2, k: &[Fr]) -> Result<Vec<G2>, GpuError> {
    let mut out = vec![G2::zero(); k.len()];
    check(unsafe { bn254_g2_mul_base_batch(std::ptr::null_mut(), base, k.as_ptr(), out.as_mut_ptr(), k.len()) })?;
    Ok(out)
}

/// `out[i] = p[i].normalize()` (src/lib.rs:88-95): `(x/z^2, y/z^3, 1)`, the point at infinity as `G1::zero()`; neighbouring points share
/// one field inversion.  The same bytes as `g1_mul_batch` by `Fr::one()`
pub fn g1_normalize(p: &[G1]) -> Result<Vec<G1>, GpuError> {
    let mut out = vec![G1::zero(); p.len()];
    check(unsafe { bn254_g1_normalize_batch(std::ptr::null_mut(), p.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

pub fn g2_normalize(p: &[G2]) -> Result<Vec<G2>, GpuError> {
    let mut out = vec![G2::zero(); p.len()];
    check(unsafe { bn254_g2_normalize_batch(std::ptr::null_mut(), p.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

/// `out[i] = (a[i] == b[i])` as group elements (`PartialEq for G<P>`, src/groups/mod.rs:83-109), whatever their Jacobian representations;
/// nothing is normalized
pub fn g1_eq(a: &[G1], b: &[G1]) -> Result<Vec<bool>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = vec![0i32; a.len()];
    check(unsafe { bn254_g1_eq_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len()) })?;
    Ok(out.into_iter().map(|r| r != 0).collect())
}

pub fn g2_eq(a: &[G2], b: &[G2]) -> Result<Vec<bool>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = vec![0i32; a.len()];
    check(unsafe { bn254_g2_eq_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len()) })?;
    Ok(out.into_iter().map(|r| r != 0).collect())
}

/// `out[i] = a[i] + b[i]` in the scalar field (src/lib.rs:33-37), for arrays of scalars that feed `g1_msm`, `g1_mul_base`, `Gt::pow` ...
pub fn fr_add(a: &[Fr], b: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = vec![Fr::zero(); a.len()];
    check(unsafe { bn254_fr_add_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len(), 0) })?;
    Ok(out)
}

/// `out[i] = a[i] - b[i]` (src/lib.rs:39-41); `-b` is `fr_sub(&zeros, b)` (src/lib.rs:43-47)
pub fn fr_sub(a: &[Fr], b: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = vec![Fr::zero(); a.len()];
    check(unsafe { bn254_fr_add_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len(), 1) })?;
    Ok(out)
}

/// `out[i] = a[i] * b[i]` (src/lib.rs:49-53)
pub fn fr_mul(a: &[Fr], b: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = vec![Fr::zero(); a.len()];
    check(unsafe { bn254_fr_mul_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len()) })?;
    Ok(out)
}

/// `out[i] = a[i].inverse()` (src/lib.rs:25): `None` for a zero element; neighbouring elements share one exponentiation
pub fn fr_inverse(a: &[Fr]) -> Result<Vec<Option<Fr>>, GpuError> {
    let mut out = vec![Fr::zero(); a.len()];
    let mut ok = vec![0i32; a.len()];
    check(unsafe { bn254_fr_inverse_batch(std::ptr::null_mut(), a.as_ptr(), out.as_mut_ptr(), ok.as_mut_ptr(), a.len()) })?;
    Ok(out.into_iter().zip(ok).map(|(x, k)| if k != 0 { Some(x) } else { None }).collect())
}

/// `out[i] = a[i].pow(e[i])` (src/lib.rs:23); `0^0` is one
pub fn fr_pow(a: &[Fr], e: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert_eq!(a.len(), e.len());
    let mut out = vec![Fr::zero(); a.len()];
    check(unsafe { bn254_fr_pow_batch(std::ptr::null_mut(), a.as_ptr(), e.as_ptr(), out.as_mut_ptr(), a.len()) })?;
    Ok(out)
}

/// `out[i] = Fr::interpret(&bufs[i])` (src/lib.rs:27-29): 64 bytes as a big-endian 512-bit integer, mod r
pub fn fr_interpret(bufs: &[[u8; 64]]) -> Result<Vec<Fr>, GpuError> {
    let mut out = vec![Fr::zero(); bufs.len()];
    check(unsafe { bn254_fr_interpret_batch(std::ptr::null_mut(), bufs.as_ptr() as *const u8, out.as_mut_ptr(), bufs.len()) })?;
    Ok(out)
}

/// `w_n` for `n = 2^log_n` (0..=28): `w_28^(2^(28 - log_n))` with `w_28 = 5^((r-1)/2^28)`, ark-bn254's root.  Host only.
pub fn fr_root_of_unity(log_n: u32) -> Result<Fr, GpuError> {
    let mut out = Fr::zero();
    check(unsafe { bn254_fr_root_of_unity(log_n as c_int, &mut out) })?;
    Ok(out)
}

/// `values.len() / 2^log_n` number-theoretic transforms of `2^log_n` elements each, natural order in and out.  Forward: the polynomial with
/// coefficients `values` evaluated at `shift * w_n^k`; inverse: the coefficients back from such evaluations.  `shift`: `None` for one.
pub fn fr_ntt(values: &[Fr], log_n: u32, inverse: bool, shift: Option<&Fr>) -> Result<Vec<Fr>, GpuError> {
    assert!(log_n <= 24 && values.len() % (1usize << log_n) == 0);
    let mut out = vec![Fr::zero(); values.len()];
    let sh = shift.map_or(std::ptr::null(), |s| s as *const Fr);
    check(unsafe { bn254_fr_ntt_batch(std::ptr::null_mut(), values.as_ptr(), out.as_mut_ptr(), log_n as c_int, values.len() >> log_n, inverse as c_int, sh) })?;
    Ok(out)
}

/// The same transforms with points for data and scalar multiplication for the product: `points.len() / 2^log_n` transforms of `2^log_n`
/// points each, natural order in and out, every output normalised.  The inverse transform of the powers `tau^i G` of a reference string
/// gives its Lagrange points.
pub fn g1_ntt(points: &[G1], log_n: u32, inverse: bool, shift: Option<&Fr>) -> Result<Vec<G1>, GpuError> {
    assert!(log_n <= 22 && points.len() % (1usize << log_n) == 0);
    let mut out = vec![G1::zero(); points.len()];
    let sh = shift.map_or(std::ptr::null(), |s| s as *const Fr);
    check(unsafe { bn254_g1_ntt_batch(std::ptr::null_mut(), points.as_ptr(), out.as_mut_ptr(), log_n as c_int, points.len() >> log_n, inverse as c_int, sh) })?;
    Ok(out)
}

pub fn g2_ntt(points: &[G2], log_n: u32, inverse: bool, shift: Option<&Fr>) -> Result<Vec<G2>, GpuError> {
    assert!(log_n <= 22 && points.len() % (1usize << log_n) == 0);
    let mut out = vec![G2::zero(); points.len()];
    let sh = shift.map_or(std::ptr::null(), |s| s as *const Fr);
    check(unsafe { bn254_g2_ntt_batch(std::ptr::null_mut(), points.as_ptr(), out.as_mut_ptr(), log_n as c_int, points.len() >> log_n, inverse as c_int, sh) })?;
    Ok(out)
}

/// `out[j] = sum of coeff[t] * x[index[t]] over t in offsets[j]..offsets[j + 1]`: a sparse matrix in CSR form (`offsets`, `index`, `coeff`)
/// times the vector `x` - the witness map of an R1CS.  `index`: `None` for `x[t]`, a plain segmented inner product (`x.len() == coeff.len()`).
/// An empty segment gives `Fr::zero()`; an index `>= x.len()` is an error, never a wrong sum.
pub fn fr_dot(coeff: &[Fr], index: Option<&[u64]>, x: &[Fr], offsets: &[usize]) -> Result<Vec<Fr>, GpuError> {
    assert!(!offsets.is_empty() && *offsets.last().unwrap() == coeff.len());
    assert!(index.map_or(x.len() == coeff.len(), |i| i.len() == coeff.len()));
    let m = offsets.len() - 1;
    let mut out = vec![Fr::zero(); m];
    let idx = index.map_or(std::ptr::null(), |i| i.as_ptr());
    check(unsafe { bn254_fr_dot_batch(std::ptr::null_mut(), coeff.as_ptr(), idx, x.as_ptr(), x.len(), offsets.as_ptr(), m, out.as_mut_ptr()) })?;
    Ok(out)
}

/// Flags of [`fr_scan`] (the header's `BN254_SCAN_*`): from each segment's last term to its first; `out[t]` is the value BEFORE term `t`;
/// `a` holds one factor per segment.
pub const SCAN_REVERSE: c_int = 1;
pub const SCAN_EXCLUSIVE: c_int = 2;
pub const SCAN_A_PER_SEGMENT: c_int = 4;

/// `out[t] = a[t] * prev + b[t]` over the terms of every segment `offsets[j]..offsets[j + 1]` in order, `prev = out[t - 1]` or `init[j]` at the
/// segment's first term: segmented prefix sums (`a`: `None`), prefix products (`b`: `None`), powers and Horner's rule (`SCAN_A_PER_SEGMENT`).
/// `init`: `None` for `Fr::zero()` with `b`, `Fr::one()` without.  One output per term; an empty segment writes nothing.
pub fn fr_scan(a: Option<&[Fr]>, b: Option<&[Fr]>, init: Option<&[Fr]>, offsets: &[usize], flags: c_int) -> Result<Vec<Fr>, GpuError> {
    assert!(!offsets.is_empty() && (a.is_some() || b.is_some()));
    let (m, n) = (offsets.len() - 1, *offsets.last().unwrap());
    assert!(b.map_or(true, |v| v.len() == n) && init.map_or(true, |v| v.len() == m));
    assert!(a.map_or(true, |v| v.len() == if flags & SCAN_A_PER_SEGMENT != 0 { m } else { n }));
    let mut out = vec![Fr::zero(); n];
    let ptr = |v: Option<&[Fr]>| v.map_or(std::ptr::null(), |s| s.as_ptr());
    check(unsafe { bn254_fr_scan_batch(std::ptr::null_mut(), ptr(a), ptr(b), ptr(init), offsets.as_ptr(), m, flags, out.as_mut_ptr()) })?;
    Ok(out)
}

/// The table of `eq(z, .)` over the hypercube of `z.len()` variables: `out[i] = prod_j (if bit j of i { z[j] } else { 1 - z[j] })`, `2^z.len()`
/// values; no variables give `[Fr::one()]`.
pub fn fr_mle_eq(z: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert!(z.len() <= 30);
    let mut out = vec![Fr::zero(); 1usize << z.len()];
    check(unsafe { bn254_fr_mle_eq(std::ptr::null_mut(), z.as_ptr(), z.len() as c_int, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `out[i] = a[i] + r * (a[i + a.len() / 2] - a[i])`: the multilinear table `a` (index `i` is the point whose variable `j` is bit `j` of `i`) with
/// its MOST significant variable bound to `r`.  `k` tables stored index-major (`a[i * k + j]`) are folded by the one call.
pub fn fr_mle_fold(a: &[Fr], r: &Fr) -> Result<Vec<Fr>, GpuError> {
    assert!(a.len() % 2 == 0);
    let mut out = vec![Fr::zero(); a.len() / 2];
    check(unsafe { bn254_fr_mle_fold(std::ptr::null_mut(), a.as_ptr(), a.len(), r as *const Fr, out.as_mut_ptr()) })?;
    Ok(out)
}

/// The round polynomial of a sumcheck at `t = 0 ..= degree`: `out[t] = sum over i < n / 2 and the groups c of group_coeff[c] * prod over j in
/// group c of (T_j[i] + t * (T_j[i + n / 2] - T_j[i]))` with `T_j[i] = tables[i * k + j]`, `n = tables.len() / k`.  Group `c` holds the table
/// numbers `group_tables[group_offsets[c]..group_offsets[c + 1]]` (1 to `degree` of them, a table may repeat).
pub fn fr_sumcheck_round(tables: &[Fr], k: usize, group_offsets: &[usize], group_tables: &[u64], group_coeff: &[Fr], degree: usize) -> Result<Vec<Fr>, GpuError> {
    assert!(k >= 1 && tables.len() % (2 * k) == 0 && !group_offsets.is_empty());
    let g = group_offsets.len() - 1;
    assert!(group_coeff.len() == g && *group_offsets.last().unwrap() == group_tables.len());
    let mut out = vec![Fr::zero(); degree + 1];
    check(unsafe {
        bn254_fr_sumcheck_round(std::ptr::null_mut(), tables.as_ptr(), tables.len() / k, k, group_offsets.as_ptr(), group_tables.as_ptr(), group_coeff.as_ptr(), g, degree as c_int, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// `fr_mle_fold` of the `k` index-major tables by `r` and `fr_sumcheck_round` of the folded tables in one pass over them: `(folded, out)` with
/// `folded[i * k + j] = T_j[i] + r * (T_j[i + n / 2] - T_j[i])` (`n / 2 * k` values, `n = tables.len() / k` a multiple of 4) and `out` the
/// `degree + 1` values of the round polynomial over `folded` - what a sumcheck prover does between two challenges.
pub fn fr_sumcheck_fold_round(tables: &[Fr], k: usize, r: &Fr, group_offsets: &[usize], group_tables: &[u64], group_coeff: &[Fr], degree: usize) -> Result<(Vec<Fr>, Vec<Fr>), GpuError> {
    assert!(k >= 1 && tables.len() % (4 * k) == 0 && !group_offsets.is_empty());
    let g = group_offsets.len() - 1;
    assert!(group_coeff.len() == g && *group_offsets.last().unwrap() == group_tables.len());
    let mut folded = vec![Fr::zero(); tables.len() / 2];
    let mut out = vec![Fr::zero(); degree + 1];
    check(unsafe {
        bn254_fr_sumcheck_fold_round(std::ptr::null_mut(), tables.as_ptr(), tables.len() / k, k, r as *const Fr, group_offsets.as_ptr(), group_tables.as_ptr(), group_coeff.as_ptr(), g, degree as c_int,
                                     folded.as_mut_ptr(), out.as_mut_ptr())
    })?;
    Ok((folded, out))
}

/// The quotients of a multilinear opening of the table `a` (`2^z.len()` values) at `z`, in heap order: `out[0] = f(z)` and `out[2^j + i] = q_j[i]`
/// with `f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1})` - from `t = a`, for `j = nv - 1` down to `0`, `q_j[i] = t[i + 2^j] - t[i]` and
/// `t[i] += z[j] * q_j[i]`.  The field work of a multilinear KZG opening.
pub fn fr_mle_quotients(a: &[Fr], z: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert!(z.len() <= 30 && a.len() == 1usize << z.len());
    let mut out = vec![Fr::zero(); a.len()];
    check(unsafe { bn254_fr_mle_quotients(std::ptr::null_mut(), a.as_ptr(), z.len() as c_int, z.as_ptr(), out.as_mut_ptr()) })?;
    Ok(out)
}

/// `out[i] = Poseidon(input[i * arity .. (i + 1) * arity])`: the circomlib / iden3 hash over `Fr` (x^5, `t = arity + 1`, `R_F = 8`,
/// `R_P = 56 / 57 / 56 / 60`), element 0 of the permutation of `[0, x_1, .., x_arity]`; `arity` is 1 to 4.
pub fn fr_poseidon(input: &[Fr], arity: usize) -> Result<Vec<Fr>, GpuError> {
    assert!((1..=4).contains(&arity) && input.len() % arity == 0);
    let n = input.len() / arity;
    let mut out = vec![Fr::zero(); n];
    check(unsafe { bn254_fr_poseidon_batch(std::ptr::null_mut(), input.as_ptr(), arity as c_int, out.as_mut_ptr(), n) })?;
    Ok(out)
}

/// The Poseidon permutation itself on `states.len() / t` states of `t` elements each, `t` 2 to 5.
pub fn fr_poseidon_permute(states: &[Fr], t: usize) -> Result<Vec<Fr>, GpuError> {
    assert!((2..=5).contains(&t) && states.len() % t == 0);
    let mut out = vec![Fr::zero(); states.len()];
    check(unsafe { bn254_fr_poseidon_permute_batch(std::ptr::null_mut(), states.as_ptr(), t as c_int, out.as_mut_ptr(), states.len() / t) })?;
    Ok(out)
}

/// The `n - 1` inner nodes of the binary Poseidon tree over `n = 2^k` leaves, level by level: the `n / 2` parents of the leaves first, the root
/// last; parent `i` of a level is `hash(child[2 i], child[2 i + 1])`.  One leaf gives no node.
pub fn fr_merkle_tree(leaves: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert!(leaves.len().is_power_of_two() && leaves.len() <= 1 << 24);
    let mut nodes = vec![Fr::zero(); leaves.len() - 1];
    check(unsafe { bn254_fr_merkle_tree(std::ptr::null_mut(), leaves.as_ptr(), leaves.len().trailing_zeros() as c_int, nodes.as_mut_ptr()) })?;
    Ok(nodes)
}

/// circomlib's `PoseidonEx(n_inputs, n_outs)` on `input.len() / n_inputs` rows of 1 to 16 inputs: the first `n_outs` elements of the permutation of
/// `[init[i], row..]` at width `n_inputs + 1` (`init`: `None` for zeros, else one element per row), `n_outs` consecutive outputs per row.
pub fn fr_poseidon_ex(input: &[Fr], n_inputs: usize, init: Option<&[Fr]>, n_outs: usize) -> Result<Vec<Fr>, GpuError> {
    assert!((1..=16).contains(&n_inputs) && input.len() % n_inputs == 0 && (1..=n_inputs + 1).contains(&n_outs));
    let n = input.len() / n_inputs;
    assert!(init.map_or(true, |i| i.len() == n));
    let mut out = vec![Fr::zero(); n * n_outs];
    check(unsafe { bn254_fr_poseidon_ex_batch(std::ptr::null_mut(), input.as_ptr(), n_inputs as c_int, init.map_or(std::ptr::null(), |i| i.as_ptr()), n_outs as c_int, out.as_mut_ptr(), n) })?;
    Ok(out)
}

/// One digest per variable-length record `input[offsets[j]..offsets[j + 1]]`: `c = len`, then per block of `rate` elements (the last padded with
/// zeros, an empty record is one block of zeros) `c = permute([c, block..])[0]` at width `rate + 1`.  The framing is this library's own.
pub fn fr_poseidon_chain(input: &[Fr], offsets: &[usize], rate: usize) -> Result<Vec<Fr>, GpuError> {
    assert!((1..=16).contains(&rate) && !offsets.is_empty() && offsets[0] == 0 && *offsets.last().unwrap() == input.len());
    let mut out = vec![Fr::zero(); offsets.len() - 1];
    check(unsafe { bn254_fr_poseidon_chain_batch(std::ptr::null_mut(), input.as_ptr(), offsets.as_ptr(), out.len(), rate as c_int, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `out[i] = a[i] * b[i]` (src/lib.rs:175-179)
pub fn gt_mul_batch(a: &[Gt], b: &[Gt]) -> Result<Vec<Gt>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = a.to_vec();
    check(unsafe { bn254_gt_mul_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len()) })?;
    Ok(out)
}

/// `out[i] = a[i].pow(k[i])` (src/lib.rs:171)
pub fn gt_pow_batch(a: &[Gt], k: &[Fr]) -> Result<Vec<Gt>, GpuError> {
    assert_eq!(a.len(), k.len());
    let mut out = a.to_vec();
    check(unsafe { bn254_gt_pow_batch(std::ptr::null_mut(), a.as_ptr(), k.as_ptr(), out.as_mut_ptr(), a.len()) })?;
    Ok(out)
}

/// `out[i] = a[i] + b[i]` (`sub`: `a[i] - b[i]`), src/lib.rs:103-111 - the crate's own Jacobian limbs
pub fn g1_add_batch(a: &[G1], b: &[G1], sub: bool) -> Result<Vec<G1>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = a.to_vec();
    check(unsafe { bn254_g1_add_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len(), sub as c_int) })?;
    Ok(out)
}

pub fn g2_add_batch(a: &[G2], b: &[G2], sub: bool) -> Result<Vec<G2>, GpuError> {
    assert_eq!(a.len(), b.len());
    let mut out = a.to_vec();
    check(unsafe { bn254_g2_add_batch(std::ptr::null_mut(), a.as_ptr(), b.as_ptr(), out.as_mut_ptr(), a.len(), sub as c_int) })?;
    Ok(out)
}

/// Batch `Decodable` for G2 (src/groups/mod.rs:162-205): `records` holds 129-byte records (what bincode yields for a finite
/// point); `Err(code)` per record carries the crate's error in order of appearance: 1 "integer is not less than modulus",
/// 2 "integer not less than modulus squared", 3 "invalid leading byte", 4 "point is not on the curve", 5 "point is not in the subgroup"
pub fn g2_decode_batch(records: &[u8]) -> Result<Vec<Result<G2, i32>>, GpuError> {
    assert_eq!(records.len() % G2_WIRE_BYTES, 0);
    let n = records.len() / G2_WIRE_BYTES;
    let (mut out, mut status) = (vec![G2::zero(); n], vec![0i32; n]);
    check(unsafe { bn254_g2_decode_batch(std::ptr::null_mut(), records.as_ptr(), out.as_mut_ptr(), status.as_mut_ptr(), n) })?;
    Ok(out.into_iter().zip(status).map(|(p, s)| if s == 0 { Ok(p) } else { Err(s) }).collect())
}

pub fn g1_decode_batch(records: &[u8]) -> Result<Vec<Result<G1, i32>>, GpuError> {
    assert_eq!(records.len() % G1_WIRE_BYTES, 0);
    let n = records.len() / G1_WIRE_BYTES;
    let (mut out, mut status) = (vec![G1::zero(); n], vec![0i32; n]);
    check(unsafe { bn254_g1_decode_batch(std::ptr::null_mut(), records.as_ptr(), out.as_mut_ptr(), status.as_mut_ptr(), n) })?;
    Ok(out.into_iter().zip(status).map(|(p, s)| if s == 0 { Ok(p) } else { Err(s) }).collect())
}

/// The byte layout of a compressed point: x and one sign bit, 32 bytes for G1 and 64 for G2.  Laid out as ark-serialize / gnark-crypto
/// describe; not checked against those libraries here.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum CompressedFormat {
    /// little endian, G2 as c0 then c1, flags in the top two bits of the last byte (bit 7 sign, bit 6 infinity)
    Ark,
    /// big endian, G2 as c1 then c0, flags in the top two bits of the first byte (10 sign 0, 11 sign 1, 01 infinity)
    Gnark,
}

impl CompressedFormat {
    fn code(self) -> c_int { match self { CompressedFormat::Ark => 0, CompressedFormat::Gnark => 1 } }
    pub const fn g1_bytes() -> usize { 32 }
    pub const fn g2_bytes() -> usize { 64 }
}

/// 32 bytes per point, canonical: any Jacobian form of a point gives the same bytes
pub fn g1_compress_batch(p: &[G1], format: CompressedFormat) -> Result<Vec<u8>, GpuError> {
    let mut out = vec![0u8; p.len() * CompressedFormat::g1_bytes()];
    check(unsafe { bn254_g1_compress_batch(std::ptr::null_mut(), p.as_ptr(), format.code(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

pub fn g2_compress_batch(p: &[G2], format: CompressedFormat) -> Result<Vec<u8>, GpuError> {
    let mut out = vec![0u8; p.len() * CompressedFormat::g2_bytes()];
    check(unsafe { bn254_g2_compress_batch(std::ptr::null_mut(), p.as_ptr(), format.code(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

/// `Err(code)` per record, checked in this order: 3 invalid flags, 1 x not below the modulus, 4 no point has this x, 5 not in the subgroup (G2)
pub fn g1_decompress_batch(records: &[u8], format: CompressedFormat) -> Result<Vec<Result<G1, i32>>, GpuError> {
    assert_eq!(records.len() % CompressedFormat::g1_bytes(), 0);
    let n = records.len() / CompressedFormat::g1_bytes();
    let (mut out, mut status) = (vec![G1::zero(); n], vec![0i32; n]);
    check(unsafe { bn254_g1_decompress_batch(std::ptr::null_mut(), records.as_ptr(), format.code(), out.as_mut_ptr(), status.as_mut_ptr(), n) })?;
    Ok(out.into_iter().zip(status).map(|(p, s)| if s == 0 { Ok(p) } else { Err(s) }).collect())
}

pub fn g2_decompress_batch(records: &[u8], format: CompressedFormat) -> Result<Vec<Result<G2, i32>>, GpuError> {
    assert_eq!(records.len() % CompressedFormat::g2_bytes(), 0);
    let n = records.len() / CompressedFormat::g2_bytes();
    let (mut out, mut status) = (vec![G2::zero(); n], vec![0i32; n]);
    check(unsafe { bn254_g2_decompress_batch(std::ptr::null_mut(), records.as_ptr(), format.code(), out.as_mut_ptr(), status.as_mut_ptr(), n) })?;
    Ok(out.into_iter().zip(status).map(|(p, s)| if s == 0 { Ok(p) } else { Err(s) }).collect())
}

// bytes per field element of hash_to_field (L of RFC 9380) and per record of the uniform call: BN254_H2C_FIELD_BYTES, BN254_H2C_UNIFORM_BYTES
const H2C_FIELD_BYTES: usize = 48;
const H2C_UNIFORM_BYTES: usize = 96;

/// map_to_curve of RFC 9380 (Shallue-van de Woestijne, Z = 1) on every 48-byte big-endian integer of `u`, taken mod q: (x, y, 1), never infinity.
/// The map's constants are derived from the RFC's formulas; not checked against gnark-crypto or any other library.
pub fn g1_map_to_curve_batch(u: &[u8]) -> Result<Vec<G1>, GpuError> {
    assert_eq!(u.len() % H2C_FIELD_BYTES, 0);
    let mut out = vec![G1::zero(); u.len() / H2C_FIELD_BYTES];
    check(unsafe { bn254_g1_map_to_curve_batch(std::ptr::null_mut(), u.as_ptr(), out.as_mut_ptr(), out.len()) })?;
    Ok(out)
}

/// hash_to_curve from 96 uniform bytes per record: map(u0) + map(u1), normalised (G1::zero() when the two maps cancel)
pub fn g1_hash_to_curve_uniform_batch(uniform: &[u8]) -> Result<Vec<G1>, GpuError> {
    assert_eq!(uniform.len() % H2C_UNIFORM_BYTES, 0);
    let mut out = vec![G1::zero(); uniform.len() / H2C_UNIFORM_BYTES];
    check(unsafe { bn254_g1_hash_to_curve_uniform_batch(std::ptr::null_mut(), uniform.as_ptr(), out.as_mut_ptr(), out.len()) })?;
    Ok(out)
}

/// hash_to_curve of `n` messages of `msg_len` bytes each, back to back in `msgs` (`msg_len` may be 0), with expand_message_xmd over SHA-256 on
/// the device; `dst` holds 1 .. 255 bytes
pub fn g1_hash_to_curve_batch(msgs: &[u8], msg_len: usize, n: usize, dst: &[u8]) -> Result<Vec<G1>, GpuError> {
    assert_eq!(msgs.len(), n * msg_len);
    let mut out = vec![G1::zero(); n];
    check(unsafe { bn254_g1_hash_to_curve_batch(std::ptr::null_mut(), msgs.as_ptr(), msg_len, dst.as_ptr(), dst.len(), out.as_mut_ptr(), n) })?;
    Ok(out)
}

// the same for G2: an Fq2 element is c0 then c1 (BN254_H2C_G2_FIELD_BYTES), a uniform record u0.c0 | u0.c1 | u1.c0 | u1.c1 (BN254_H2C_G2_UNIFORM_BYTES)
const H2C_G2_FIELD_BYTES: usize = 96;
const H2C_G2_UNIFORM_BYTES: usize = 192;

/// map_to_curve of RFC 9380 over Fq2 (Shallue-van de Woestijne, Z = 1) on every 96-byte element of `u`: (x, y, 1) on the twist, never infinity
/// and NOT in G2 - clear the cofactor before any other use.  The map's constants are derived from the RFC's formulas; neither they nor the
/// outputs are checked against gnark-crypto or any other library.
pub fn g2_map_to_curve_batch(u: &[u8]) -> Result<Vec<G2>, GpuError> {
    assert_eq!(u.len() % H2C_G2_FIELD_BYTES, 0);
    let mut out = vec![G2::zero(); u.len() / H2C_G2_FIELD_BYTES];
    check(unsafe { bn254_g2_map_to_curve_batch(std::ptr::null_mut(), u.as_ptr(), out.as_mut_ptr(), out.len()) })?;
    Ok(out)
}

/// clear(P) = [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P), normalised, for any Jacobian point of the twist (on the curve: the caller's
/// responsibility): a point of G2, G2::zero() for infinity.  Not [2q - r]P; not checked against gnark-crypto or any other library.
pub fn g2_clear_cofactor_batch(p: &[G2]) -> Result<Vec<G2>, GpuError> {
    let mut out = vec![G2::zero(); p.len()];
    check(unsafe { bn254_g2_clear_cofactor_batch(std::ptr::null_mut(), p.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

/// hash_to_curve from 192 uniform bytes per record: clear(map(u0) + map(u1)), normalised (G2::zero() when the two maps cancel)
pub fn g2_hash_to_curve_uniform_batch(uniform: &[u8]) -> Result<Vec<G2>, GpuError> {
    assert_eq!(uniform.len() % H2C_G2_UNIFORM_BYTES, 0);
    let mut out = vec![G2::zero(); uniform.len() / H2C_G2_UNIFORM_BYTES];
    check(unsafe { bn254_g2_hash_to_curve_uniform_batch(std::ptr::null_mut(), uniform.as_ptr(), out.as_mut_ptr(), out.len()) })?;
    Ok(out)
}

/// hash_to_curve into G2 of `n` messages of `msg_len` bytes each, back to back in `msgs` (`msg_len` may be 0), with expand_message_xmd over
/// SHA-256 on the device; `dst` holds 1 .. 255 bytes
pub fn g2_hash_to_curve_batch(msgs: &[u8], msg_len: usize, n: usize, dst: &[u8]) -> Result<Vec<G2>, GpuError> {
    assert_eq!(msgs.len(), n * msg_len);
    let mut out = vec![G2::zero(); n];
    check(unsafe { bn254_g2_hash_to_curve_batch(std::ptr::null_mut(), msgs.as_ptr(), msg_len, dst.as_ptr(), dst.len(), out.as_mut_ptr(), n) })?;
    Ok(out)
}

/// One status per raw point, checked in this order: 1 a coordinate is not below the modulus, 0 for z == 0 (infinity), 4 not on the curve, else 0.
/// G1 has cofactor 1: a point on the curve is in the group.
pub fn g1_validate_batch(p: &[G1]) -> Result<Vec<i32>, GpuError> {
    let mut status = vec![0i32; p.len()];
    check(unsafe { bn254_g1_validate_batch(std::ptr::null_mut(), p.as_ptr(), status.as_mut_ptr(), p.len()) })?;
    Ok(status)
}

/// The same for G2, and 5 for a point of the twist outside the order-r subgroup (the endomorphism subgroup test
/// [u + 1]P + psi([u]P) + psi^2([u]P) == psi^3([2u]P)): the check every pairing, multiplication and verifier here leaves to its caller.
pub fn g2_validate_batch(p: &[G2]) -> Result<Vec<i32>, GpuError> {
    let mut status = vec![0i32; p.len()];
    check(unsafe { bn254_g2_validate_batch(std::ptr::null_mut(), p.as_ptr(), status.as_mut_ptr(), p.len()) })?;
    Ok(status)
}

/// `Option<Fr>` square roots: the root whose canonical integer is not above `(r - 1) / 2`, `None` for a non-residue.
pub fn fr_sqrt(a: &[Fr]) -> Result<Vec<Option<Fr>>, GpuError> {
    let mut out = vec![Fr::zero(); a.len()];
    let mut ok = vec![0i32; a.len()];
    check(unsafe { bn254_fr_sqrt_batch(std::ptr::null_mut(), a.as_ptr(), out.as_mut_ptr(), ok.as_mut_ptr(), a.len()) })?;
    Ok(out.into_iter().zip(ok).map(|(x, k)| if k != 0 { Some(x) } else { None }).collect())
}

/// Baby Jubjub points (`2 n` elements) to circomlib's 32-byte records: `y` little endian, the sign of `x` in the top bit.  No validation.
pub fn bjj_pack_batch(p: &[Fr]) -> Result<Vec<u8>, GpuError> {
    assert_eq!(p.len() % 2, 0);
    let mut out = vec![0u8; 16 * p.len()];
    check(unsafe { bn254_bjj_pack_batch(std::ptr::null_mut(), p.as_ptr(), out.as_mut_ptr(), p.len() / 2) })?;
    Ok(out)
}

/// 32-byte records to points and one status each: 1 `y` is not below r, 4 no point has this `y`, 3 `x == 0` with the sign bit set, else 0.
/// A rejected record gives the identity `(0, 1)`.  No subgroup check.
pub fn bjj_unpack_batch(in32: &[u8]) -> Result<(Vec<Fr>, Vec<i32>), GpuError> {
    assert_eq!(in32.len() % 32, 0);
    let n = in32.len() / 32;
    let mut out = vec![Fr::zero(); 2 * n];
    let mut status = vec![0i32; n];
    check(unsafe { bn254_bjj_unpack_batch(std::ptr::null_mut(), in32.as_ptr(), out.as_mut_ptr(), status.as_mut_ptr(), n) })?;
    Ok((out, status))
}

/// `eddsa_poseidon_verify_batch` on packed keys (32 bytes) and packed signatures (64 bytes: packed `R8`, then `S` little endian): 1 range,
/// 4 a point has no `x`, 3 a non-canonical sign, 6 the equation fails, 0 valid.
pub fn eddsa_poseidon_verify_packed_batch(a32: &[u8], sig64: &[u8], msg: &[Fr]) -> Result<Vec<i32>, GpuError> {
    assert!(a32.len() == 32 * msg.len() && sig64.len() == 64 * msg.len());
    let mut status = vec![0i32; msg.len()];
    check(unsafe { bn254_eddsa_poseidon_verify_packed_batch(std::ptr::null_mut(), a32.as_ptr(), sig64.as_ptr(), msg.as_ptr(), status.as_mut_ptr(), msg.len()) })?;
    Ok(status)
}

/// Grumpkin, `y^2 = x^3 - 17` over `Fr`, the other half of the BN254 curve cycle (prime order q, cofactor 1): a point is two consecutive `Fr`, x
/// then y, affine, infinity `(0, 0)`, so `p` holds `2 n` elements.  One status per raw point, checked in this order: 1 a coordinate is not
/// below r, 4 not on the curve, else 0 (`(0, 0)` is valid).  There is no subgroup status.
pub fn grumpkin_validate_batch(p: &[Fr]) -> Result<Vec<i32>, GpuError> {
    assert_eq!(p.len() % 2, 0);
    let mut status = vec![0i32; p.len() / 2];
    check(unsafe { bn254_grumpkin_validate_batch(std::ptr::null_mut(), p.as_ptr(), status.as_mut_ptr(), p.len() / 2) })?;
    Ok(status)
}

/// `out[i] = p[i] + q[i]`: the complete sum, for points of the curve (not checked).
pub fn grumpkin_add_batch(p: &[Fr], q: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert!(p.len() % 2 == 0 && p.len() == q.len());
    let mut out = vec![Fr::zero(); p.len()];
    check(unsafe { bn254_grumpkin_add_batch(std::ptr::null_mut(), p.as_ptr(), q.as_ptr(), out.as_mut_ptr(), p.len() / 2) })?;
    Ok(out)
}

/// `out[i] = [k[i]] p[i]`; a scalar is 32 bytes, the little-endian integer (any value below 2^256; NOT a Montgomery image), so `k32` holds `32 n` bytes.
pub fn grumpkin_mul_batch(p: &[Fr], k32: &[u8]) -> Result<Vec<Fr>, GpuError> {
    assert!(k32.len() % 32 == 0 && p.len() == 2 * (k32.len() / 32));
    let mut out = vec![Fr::zero(); p.len()];
    check(unsafe { bn254_grumpkin_mul_batch(std::ptr::null_mut(), p.as_ptr(), k32.as_ptr(), out.as_mut_ptr(), k32.len() / 32) })?;
    Ok(out)
}

/// `out[j] = sum of [k[t]] p[t]` over `t` in `[offsets[j], offsets[j+1])`: many independent multi-scalar multiplications in one call.  An
/// empty or cancelling segment gives `(0, 0)`.
pub fn grumpkin_msm_batch(p: &[Fr], k32: &[u8], offsets: &[usize]) -> Result<Vec<Fr>, GpuError> {
    assert!(!offsets.is_empty() && k32.len() == 32 * offsets[offsets.len() - 1] && p.len() == 2 * offsets[offsets.len() - 1]);
    let m = offsets.len() - 1;
    let mut out = vec![Fr::zero(); 2 * m];
    check(unsafe { bn254_grumpkin_msm_batch(std::ptr::null_mut(), p.as_ptr(), k32.as_ptr(), offsets.as_ptr(), m, out.as_mut_ptr()) })?;
    Ok(out)
}

/// Baby Jubjub, the twisted Edwards curve `a x^2 + y^2 = 1 + d x^2 y^2` over `Fr` (a = 168700, d = 168696): a point is two consecutive `Fr`, x then
/// y, affine, so `p` holds `2 n` elements.  One status per raw point, checked in this order: 1 a coordinate is not below r, 4 not on the curve,
/// 5 on the curve but `[l]P != O`, else 0 (the identity `(0, 1)` is valid).
pub fn bjj_validate_batch(p: &[Fr]) -> Result<Vec<i32>, GpuError> {
    assert_eq!(p.len() % 2, 0);
    let mut status = vec![0i32; p.len() / 2];
    check(unsafe { bn254_bjj_validate_batch(std::ptr::null_mut(), p.as_ptr(), status.as_mut_ptr(), p.len() / 2) })?;
    Ok(status)
}

/// `out[i] = p[i] + q[i]`: the complete affine sum, for points of the curve (not checked).
pub fn bjj_add_batch(p: &[Fr], q: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert!(p.len() % 2 == 0 && p.len() == q.len());
    let mut out = vec![Fr::zero(); p.len()];
    check(unsafe { bn254_bjj_add_batch(std::ptr::null_mut(), p.as_ptr(), q.as_ptr(), out.as_mut_ptr(), p.len() / 2) })?;
    Ok(out)
}

/// `out[i] = [k[i]] p[i]` for any point of the curve, cofactor components included; the scalar is the canonical integer of `k[i]`.
pub fn bjj_mul_batch(p: &[Fr], k: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert_eq!(p.len(), 2 * k.len());
    let mut out = vec![Fr::zero(); p.len()];
    check(unsafe { bn254_bjj_mul_batch(std::ptr::null_mut(), p.as_ptr(), k.as_ptr(), out.as_mut_ptr(), k.len()) })?;
    Ok(out)
}

/// `out[i] = Poseidon5(r8[i].x, r8[i].y, a[i].x, a[i].y, msg[i])`: the challenge of EdDSA-Poseidon (circomlib's Poseidon at width 6); no curve check.
pub fn eddsa_poseidon_challenge_batch(a: &[Fr], r8: &[Fr], msg: &[Fr]) -> Result<Vec<Fr>, GpuError> {
    assert!(a.len() == 2 * msg.len() && r8.len() == 2 * msg.len());
    let mut out = vec![Fr::zero(); msg.len()];
    check(unsafe { bn254_eddsa_poseidon_challenge_batch(std::ptr::null_mut(), a.as_ptr(), r8.as_ptr(), msg.as_ptr(), out.as_mut_ptr(), msg.len()) })?;
    Ok(out)
}

/// circomlib's `verifyPoseidon` per row: 1 a word array is not below r or `s` is not below l, 4 `R8` or `A` is not on the curve,
/// 6 `[S]B8 != R8 + [8 hm]A`, 0 valid.  There is no subgroup check: `A = O` with `R8 = [S]B8` verifies, as in circomlib.
pub fn eddsa_poseidon_verify_batch(a: &[Fr], r8: &[Fr], s: &[Fr], msg: &[Fr]) -> Result<Vec<i32>, GpuError> {
    assert!(a.len() == 2 * msg.len() && r8.len() == 2 * msg.len() && s.len() == msg.len());
    let mut status = vec![0i32; msg.len()];
    check(unsafe { bn254_eddsa_poseidon_verify_batch(std::ptr::null_mut(), a.as_ptr(), r8.as_ptr(), s.as_ptr(), msg.as_ptr(), status.as_mut_ptr(), msg.len()) })?;
    Ok(status)
}

/// `q.to_affine().precompute()` for every q (src/groups/mod.rs:557-588; q must not be infinity): 102 coefficients per point, in schedule order
pub fn g2_precompute(q: &[G2]) -> Result<Vec<EllCoeffs>, GpuError> {
    let mut out = vec![EllCoeffs { ell_0: [0; 8], ell_vw: [0; 8], ell_vv: [0; 8] }; q.len() * PREPARED_COEFFS];
    check(unsafe { bn254_g2_precompute(std::ptr::null_mut(), q.as_ptr(), out.as_mut_ptr(), q.len()) })?;
    Ok(out)
}

/// `final_exponentiation(prepared.miller_loop(p[i]))` (src/groups/mod.rs:486-519, 768) against ONE prepared point (`coeffs.len() == 102`) or one
/// per p (`coeffs.len() == 102 * p.len()`)
pub fn pairing_prepared_batch(p: &[G1], coeffs: &[EllCoeffs]) -> Result<Vec<Gt>, GpuError> {
    let shared = coeffs.len() == PREPARED_COEFFS;
    assert!(shared || coeffs.len() == PREPARED_COEFFS * p.len());
    let mut out = vec![Gt::one(); p.len()];
    check(unsafe { bn254_pairing_prepared_batch(std::ptr::null_mut(), p.as_ptr(), coeffs.as_ptr(), shared as c_int, out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

/// G2 points prepared ONCE for many pairings (a verification key): the device-native counterpart of the crate's internal `G2Precomp`
/// (src/groups/mod.rs:472-483, `precompute` :557-588) - the line functions of the Miller loop in the form the kernels consume, resident in GPU
/// memory (33 792 bytes per point) on the default context's device.  Immutable after creation, hence `Sync`.
pub struct PreparedG2(*mut c_void);
unsafe impl Send for PreparedG2 {}
unsafe impl Sync for PreparedG2 {}

impl PreparedG2 {
    /// `q.len() == 1`: one point for every `p`; otherwise point `i` is paired with `p[i]`
    pub fn new(q: &[G2]) -> Result<PreparedG2, GpuError> {
        let mut h = std::ptr::null_mut();
        check(unsafe { bn254_g2_prepare(std::ptr::null_mut(), q.as_ptr(), q.len(), &mut h) })?;
        Ok(PreparedG2(h))
    }
    pub fn len(&self) -> usize { unsafe { bn254_g2_prepared_count(self.0) } }
    pub fn device_bytes(&self) -> usize { unsafe { bn254_g2_prepared_bytes(self.0) } }
    /// `out[i] = bn::pairing(p[i], q)` for a one-point handle, `bn::pairing(p[i], q[i])` otherwise (src/lib.rs:181-183 through
    /// src/groups/mod.rs:486-519: `precompute` happened in `new`)
    pub fn pairing_batch(&self, p: &[G1]) -> Result<Vec<Gt>, GpuError> {
        assert!(self.len() == 1 || p.len() <= self.len());
        let mut out = vec![Gt::one(); p.len()];
        check(unsafe { bn254_pairing_prepared_native_batch(std::ptr::null_mut(), p.as_ptr(), self.0, out.as_mut_ptr(), p.len()) })?;
        Ok(out)
    }
    /// `fold(Gt::one(), |acc, i| acc * bn::pairing(p[i], q[i]))` (shootout/main.rs:11-16) with ONE final exponentiation
    pub fn pairing_product(&self, p: &[G1]) -> Result<Gt, GpuError> {
        assert!(self.len() == 1 || p.len() <= self.len());
        let mut out = Gt::one();
        check(unsafe { bn254_pairing_product_prepared_native(std::ptr::null_mut(), p.as_ptr(), self.0, p.len(), &mut out) })?;
        Ok(out)
    }
    /// `out[j] = fold(Gt::one(), |acc, i| acc * bn::pairing(p[i], q[q_index[i]]))` over the pairs `offsets[j]..offsets[j + 1]`: `pairing_product_batch`
    /// with the G2 side prepared, ONE final exponentiation per segment.  `q_index: None`: pair `i` uses point `i` (a one-point handle: point 0)
    pub fn pairing_product_batch(&self, p: &[G1], q_index: Option<&[usize]>, offsets: &[usize]) -> Result<Vec<Gt>, GpuError> {
        assert!(!offsets.is_empty() && offsets[offsets.len() - 1] == p.len());
        if let Some(qi) = q_index { assert_eq!(qi.len(), p.len()); }
        let mut out = vec![Gt::one(); offsets.len() - 1];
        let qi = q_index.map_or(std::ptr::null(), |q| q.as_ptr());
        check(unsafe { bn254_pairing_product_batch_prepared_native(std::ptr::null_mut(), p.as_ptr(), self.0, qi, offsets.as_ptr(), out.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// `ok[j]` = (product of segment j == `Gt::one()`): a block of Groth16 / EIP-197-style checks against prepared points
    pub fn pairing_check_batch(&self, p: &[G1], q_index: Option<&[usize]>, offsets: &[usize]) -> Result<Vec<bool>, GpuError> {
        Ok(self.pairing_product_batch(p, q_index, offsets)?.into_iter().map(|g| g == Gt::one()).collect())
    }
}
impl Drop for PreparedG2 {
    fn drop(&mut self) { unsafe { bn254_g2_prepared_destroy(self.0) } }
}

/// the crate's `Encodable for Fr` (src/fields/fp.rs:24-36): 32 big-endian bytes per scalar
pub fn fr_encode_batch(k: &[Fr]) -> Result<Vec<u8>, GpuError> {
    let mut out = vec![0u8; k.len() * FR_WIRE_BYTES];
    check(unsafe { bn254_fr_encode_batch(std::ptr::null_mut(), k.as_ptr(), out.as_mut_ptr(), k.len()) })?;
    Ok(out)
}

/// `Decodable for Fr`: `Err(1)` = "integer is not less than modulus"
pub fn fr_decode_batch(records: &[u8]) -> Result<Vec<Result<Fr, i32>>, GpuError> {
    assert_eq!(records.len() % FR_WIRE_BYTES, 0);
    let n = records.len() / FR_WIRE_BYTES;
    let (mut out, mut status) = (vec![Fr::zero(); n], vec![0i32; n]);
    check(unsafe { bn254_fr_decode_batch(std::ptr::null_mut(), records.as_ptr(), out.as_mut_ptr(), status.as_mut_ptr(), n) })?;
    Ok(out.into_iter().zip(status).map(|(k, s)| if s == 0 { Ok(k) } else { Err(s) }).collect())
}

/// fixed-size records `[4][x][y]` (infinity: tag 0 and padding), 65 bytes per G1 point
pub fn g1_encode_batch(p: &[G1]) -> Result<Vec<u8>, GpuError> {
    let mut out = vec![0u8; p.len() * G1_WIRE_BYTES];
    check(unsafe { bn254_g1_encode_batch(std::ptr::null_mut(), p.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

pub fn g2_encode_batch(p: &[G2]) -> Result<Vec<u8>, GpuError> {
    let mut out = vec![0u8; p.len() * G2_WIRE_BYTES];
    check(unsafe { bn254_g2_encode_batch(std::ptr::null_mut(), p.as_ptr(), out.as_mut_ptr(), p.len()) })?;
    Ok(out)
}

/// the crate's own variable-length stream (what `bincode::encode` yields for a sequence of points: infinity is the lone byte 0)
pub fn g1_encode_stream(p: &[G1]) -> Result<Vec<u8>, GpuError> {
    let mut out = vec![0u8; p.len() * G1_WIRE_BYTES];
    let mut written = 0usize;
    check(unsafe { bn254_g1_encode_stream(std::ptr::null_mut(), p.as_ptr(), p.len(), out.as_mut_ptr(), out.len(), &mut written) })?;
    out.truncate(written);
    Ok(out)
}

pub fn g2_encode_stream(p: &[G2]) -> Result<Vec<u8>, GpuError> {
    let mut out = vec![0u8; p.len() * G2_WIRE_BYTES];
    let mut written = 0usize;
    check(unsafe { bn254_g2_encode_stream(std::ptr::null_mut(), p.as_ptr(), p.len(), out.as_mut_ptr(), out.len(), &mut written) })?;
    out.truncate(written);
    Ok(out)
}

/// up to `max_points` points from the crate's stream format; returns the points (a rejected record comes back as `Err(status)`, the decoder
/// goes on with the next record unless `GpuOption::StreamStopAtError` is set) and the number of bytes consumed
pub fn g1_decode_stream(bytes: &[u8], max_points: usize) -> Result<(Vec<Result<G1, i32>>, usize), GpuError> {
    let (mut out, mut status) = (vec![G1::zero(); max_points], vec![0i32; max_points]);
    let (mut count, mut consumed) = (0usize, 0usize);
    check(unsafe { bn254_g1_decode_stream(std::ptr::null_mut(), bytes.as_ptr(), bytes.len(), out.as_mut_ptr(), status.as_mut_ptr(), max_points, &mut count, &mut consumed) })?;
    out.truncate(count); status.truncate(count);
    Ok((out.into_iter().zip(status).map(|(p, s)| if s == 0 { Ok(p) } else { Err(s) }).collect(), consumed))
}

pub fn g2_decode_stream(bytes: &[u8], max_points: usize) -> Result<(Vec<Result<G2, i32>>, usize), GpuError> {
    let (mut out, mut status) = (vec![G2::zero(); max_points], vec![0i32; max_points]);
    let (mut count, mut consumed) = (0usize, 0usize);
    check(unsafe { bn254_g2_decode_stream(std::ptr::null_mut(), bytes.as_ptr(), bytes.len(), out.as_mut_ptr(), status.as_mut_ptr(), max_points, &mut count, &mut consumed) })?;
    out.truncate(count); status.truncate(count);
    Ok((out.into_iter().zip(status).map(|(p, s)| if s == 0 { Ok(p) } else { Err(s) }).collect(), consumed))
}

#[cfg(test)]
mod tests {
    // mirrors shootout/main.rs: the GPU fold equals the CPU fold
    use super::*;
    #[test]
    fn product_matches_cpu_fold() {
        let (mut a, mut b) = (G1::one(), G2::one());
        let c = Fr::from_str("1901").unwrap().inverse().unwrap();
        let d = Fr::from_str("2344").unwrap().inverse().unwrap();
        let (mut ps, mut qs, mut acc) = (vec![], vec![], Gt::one());
        for _ in 0..64 {
            acc = acc * bn::pairing(a, b);
            ps.push(a); qs.push(b);
            a = a * c; b = b * d;
        }
        assert!(pairing_product(&ps, &qs).unwrap() == acc);
        assert!(pairing_batch(&ps, &qs).unwrap().into_iter().fold(Gt::one(), |x, y| x * y) == acc);
    }
}


/// `out[i] = a[i].inverse()` (src/lib.rs:172)
pub fn gt_inverse_batch(a: &[Gt]) -> Result<Vec<Gt>, GpuError> {
    let mut out = a.to_vec();
    check(unsafe { bn254_gt_inverse_batch(std::ptr::null_mut(), a.as_ptr(), out.as_mut_ptr(), a.len()) })?;
    Ok(out)
}

/// All (or some) GPUs of one node behind one handle: independent pairings are sharded by contiguous ranges, the multi-pairing
/// product exchanges ONE 384-byte partial per GPU (RCCL all-gather over xGMI) and runs a single final exponentiation.
pub struct MultiGpu(*mut c_void);
unsafe impl Send for MultiGpu {}
unsafe impl Sync for MultiGpu {}          // the handle locks internally: one multi-device call at a time

impl MultiGpu {
    /// `devices`: HIP device index of every rank, e.g. `&[0, 1, 2, 3, 4, 5, 6, 7]`
    pub fn new(devices: &[i32]) -> Result<MultiGpu, GpuError> {
        let mut h = std::ptr::null_mut();
        check(unsafe { bn254_multi_create(devices.as_ptr(), devices.len() as c_int, &mut h) })?;
        Ok(MultiGpu(h))
    }
    /// the same with the exchange of the product forced: `Some(false)` peer copies, `Some(true)` RCCL (error instead of a fall-back)
    pub fn with_exchange(devices: &[i32], rccl: Option<bool>) -> Result<MultiGpu, GpuError> {
        let mut h = std::ptr::null_mut();
        let kind = match rccl { None => -1, Some(false) => 0, Some(true) => 1 };
        check(unsafe { bn254_multi_create_ex(devices.as_ptr(), devices.len() as c_int, kind, &mut h) })?;
        Ok(MultiGpu(h))
    }
    /// an option on every rank's context
    pub fn set_option(&self, key: GpuOption, value: Option<i64>) -> Result<(), GpuError> {
        check(unsafe { bn254_multi_set_option(self.0, key as c_int, value.unwrap_or(-1) as c_long) })
    }
    /// NUMA node the host thread of `rank` is pinned to during a call (None: not pinned)
    pub fn rank_numa_node(&self, rank: usize) -> Option<i32> {
        let n = unsafe { bn254_multi_rank_numa_node(self.0, rank as c_int) };
        if n < 0 { None } else { Some(n) }
    }
    /// `out[i] = bn::pairing(p[i], q[i])`, 2^20 pairings over 8 GPUs = BASELINE configs[2]
    pub fn pairing_batch(&self, p: &[G1], q: &[G2]) -> Result<Vec<Gt>, GpuError> {
        assert_eq!(p.len(), q.len());
        let mut out = vec![Gt::one(); p.len()];
        check(unsafe { bn254_pairing_batch_multi(self.0, p.as_ptr(), q.as_ptr(), out.as_mut_ptr(), p.len()) })?;
        Ok(out)
    }
    /// the fold of shootout/main.rs:11-16 over all pairs (BASELINE configs[3])
    pub fn pairing_product(&self, p: &[G1], q: &[G2]) -> Result<Gt, GpuError> {
        assert_eq!(p.len(), q.len());
        let mut out = Gt::one();
        check(unsafe { bn254_pairing_product_multi(self.0, p.as_ptr(), q.as_ptr(), p.len(), &mut out) })?;
        Ok(out)
    }
    /// `pairing_product_batch` with the segments sharded over the GPUs (segment j on the GPU whose pair shard holds offsets[j]; no exchange)
    pub fn pairing_product_batch(&self, p: &[G1], q: &[G2], offsets: &[usize]) -> Result<Vec<Gt>, GpuError> {
        assert_eq!(p.len(), q.len());
        assert!(!offsets.is_empty() && offsets[offsets.len() - 1] == p.len());
        let mut out = vec![Gt::one(); offsets.len() - 1];
        check(unsafe { bn254_pairing_product_batch_multi(self.0, p.as_ptr(), q.as_ptr(), offsets.as_ptr(), out.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// `g1_msm_batch` with the segments sharded over the GPUs (segment j on the GPU whose term shard holds offsets[j]; no exchange)
    pub fn g1_msm_batch(&self, p: &[G1], k: &[Fr], offsets: &[usize]) -> Result<Vec<G1>, GpuError> {
        assert_eq!(p.len(), k.len());
        assert!(!offsets.is_empty() && offsets[offsets.len() - 1] == p.len());
        let mut out = vec![G1::zero(); offsets.len() - 1];
        check(unsafe { bn254_g1_msm_batch_multi(self.0, p.as_ptr(), k.as_ptr(), offsets.as_ptr(), out.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }
    pub fn g2_msm_batch(&self, p: &[G2], k: &[Fr], offsets: &[usize]) -> Result<Vec<G2>, GpuError> {
        assert_eq!(p.len(), k.len());
        assert!(!offsets.is_empty() && offsets[offsets.len() - 1] == p.len());
        let mut out = vec![G2::zero(); offsets.len() - 1];
        check(unsafe { bn254_g2_msm_batch_multi(self.0, p.as_ptr(), k.as_ptr(), offsets.as_ptr(), out.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// `g1_msm` with the terms sharded over the GPUs; GPU 0 adds the partial sums (no device-to-device exchange)
    pub fn g1_msm(&self, p: &[G1], k: &[Fr]) -> Result<G1, GpuError> {
        assert_eq!(p.len(), k.len());
        let mut out = G1::zero();
        check(unsafe { bn254_g1_msm_multi(self.0, p.as_ptr(), k.as_ptr(), p.len(), &mut out) })?;
        Ok(out)
    }
    pub fn g2_msm(&self, p: &[G2], k: &[Fr]) -> Result<G2, GpuError> {
        assert_eq!(p.len(), k.len());
        let mut out = G2::zero();
        check(unsafe { bn254_g2_msm_multi(self.0, p.as_ptr(), k.as_ptr(), p.len(), &mut out) })?;
        Ok(out)
    }
}
/// G2 points prepared on the GPUs of a `MultiGpu` (one point: on every GPU; several: sharded like the pairings they will meet)
pub struct MultiPreparedG2<'a> { h: *mut c_void, gpus: &'a MultiGpu }
impl MultiGpu {
    pub fn prepare_g2(&self, q: &[G2]) -> Result<MultiPreparedG2, GpuError> {
        let mut h = std::ptr::null_mut();
        check(unsafe { bn254_g2_prepare_multi(self.0, q.as_ptr(), q.len(), &mut h) })?;
        Ok(MultiPreparedG2 { h, gpus: self })
    }
}
impl<'a> MultiPreparedG2<'a> {
    pub fn len(&self) -> usize { unsafe { bn254_multi_prepared_count(self.h) } }
    /// `out[i] = bn::pairing(p[i], q)` (one prepared point) resp. `bn::pairing(p[i], q[i])` (`p.len() == self.len()`), sharded over the GPUs
    pub fn pairing_batch(&self, p: &[G1]) -> Result<Vec<Gt>, GpuError> {
        let mut out = vec![Gt::one(); p.len()];
        check(unsafe { bn254_pairing_prepared_native_batch_multi(self.gpus.0, p.as_ptr(), self.h, out.as_mut_ptr(), p.len()) })?;
        Ok(out)
    }
    /// the fold of shootout/main.rs:11-16 over the prepared points, sharded: one 384-byte exchange, ONE final exponentiation
    pub fn pairing_product(&self, p: &[G1]) -> Result<Gt, GpuError> {
        let mut out = Gt::one();
        check(unsafe { bn254_pairing_product_prepared_native_multi(self.gpus.0, p.as_ptr(), self.h, p.len(), &mut out) })?;
        Ok(out)
    }
}
impl<'a> Drop for MultiPreparedG2<'a> {
    fn drop(&mut self) { unsafe { bn254_multi_prepared_destroy(self.h) } }
}
impl Drop for MultiGpu {
    fn drop(&mut self) { unsafe { bn254_multi_destroy(self.0) } }
}
