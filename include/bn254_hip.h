/*
 * bn254_hip.h - C ABI of the MI355X-native batched BN254 optimal-ate pairing engine.
 *
 * Drop-in boundary for the `pairing()` hot path of the reference crate zcash-hackworks/bn v0.4.3.  The reference has no
 * FFI of its own: its boundary is the public Rust API, whose types are all #[repr(C)] newtype chains, which fixes the
 * C layouts below (citations are file:line under the reference's src/):
 *
 *   bn_fr  = bn::Fr -> fields::Fr -> U256 -> [u64;4]        lib.rs:15-17, fields/fp.rs:11-13, arith.rs:9-11
 *   bn_g1  = bn::G1 -> G<G1Params>{x,y,z: Fq}               lib.rs:79-81, groups/mod.rs:36-41
 *   bn_g2  = bn::G2 -> G<G2Params>{x,y,z: Fq2{c0,c1}}       lib.rs:122-124, fields/fq2.rs:24-29
 *   bn_gt  = bn::Gt -> Fq12{c0,c1: Fq6{c0,c1,c2: Fq2}}      lib.rs:165-167, fields/fq12.rs:26-31, fields/fq6.rs:42-48
 *
 * Every Fq/Fr is 4 little-endian u64 limbs holding the Montgomery image a*2^256 mod m, always < m (canonical), exactly
 * the bytes the reference keeps in memory.  Points are Jacobian (X/Z^2, Y/Z^3); infinity is z == 0.
 *
 * Semantics replaced:
 *   bn254_pairing_batch    out[i] = bn::pairing(p[i], q[i])                         lib.rs:181-183, groups/mod.rs:764-771
 *   bn254_pairing_product  fold(Gt::one(), |acc,(p,q)| acc * pairing(p,q))          shootout/main.rs:11-16, lib.rs:175-179
 *   bn254_pairing_product_batch  out[j] = that fold over pairs [offsets[j], offsets[j+1])   shootout/main.rs:11-16 per segment, lib.rs:175-183
 *   bn254_pairing_product_batch_prepared_native  the same with the G2 side prepared: pair i against point q_index[i] of a bn254_g2_prepared handle
 *   bn254_g1_mul_batch     out[i] = normalize(p[i] * k[i])                          lib.rs:116-120,88-95, groups/mod.rs:250-270
 *   bn254_g2_mul_batch     same over G2                                             lib.rs:159-163,131-138
 *   bn254_g1_mul_base_batch / bn254_g2_mul_base_batch  out[i] = normalize(base * k[i]): the same with ONE left operand for the whole batch
 *                                                                                    (G::random = G::one() * Fr::random(), groups/mod.rs:220-222)
 *   bn254_g1_msm_batch     out[j] = normalize(fold(G1::zero(), |acc, i| acc + p[i] * k[i])) over terms [offsets[j], offsets[j+1])
 *                                                                                    lib.rs:103-120,88-95, groups/mod.rs:250-311
 *   bn254_g2_msm_batch     same over G2                                             lib.rs:146-163,131-138
 *   bn254_g1_msm / bn254_g2_msm  out[0] = that fold over ALL n terms (one large sum; the bucket method from BN254_OPT_MSM_BUCKET_MIN terms on)
 *   bn254_g1/g2_add_batch  out[i] = a[i] + b[i] / a[i] - b[i] (raw Jacobian limbs)       lib.rs:103-114,146-157, groups/mod.rs:275-347
 *   bn254_g1_normalize_batch / bn254_g2_normalize_batch  out[i] = p[i].normalize() = (x/z^2, y/z^3, 1), infinity as G::zero()
 *                                                                                    lib.rs:88-95,131-138, groups/mod.rs:113-130
 *   bn254_g1_eq_batch / bn254_g2_eq_batch  out[i] = (a[i] == b[i]) as 1 / 0           PartialEq for G<P>, groups/mod.rs:83-109
 *   bn254_fr_add_batch     out[i] = a[i] + b[i] / a[i] - b[i]                            lib.rs:33-47 (Add, Sub, Neg = 0 - b), fields/fp.rs:131-167
 *   bn254_fr_mul_batch     out[i] = a[i] * b[i]                                          lib.rs:49-53, fields/fp.rs:169-177
 *   bn254_fr_inverse_batch out[i] = a[i].inverse(): Option<Fr> as ok[i] = 1, or 0 with Fr::zero()   lib.rs:25, fields/fp.rs:107-115
 *   bn254_fr_pow_batch     out[i] = a[i].pow(e[i])                                       lib.rs:23, fields/mod.rs:35-46
 *   bn254_fr_interpret_batch  out[i] = Fr::interpret(&in[64 i .. 64 i + 64])             lib.rs:27-29, fields/fp.rs:72-74, arith.rs:90-97
 *   bn254_fr_sqrt_batch    out[i] = the square root of a[i] that is not above (r - 1) / 2: Option<Fr> as ok[i] = 1, or 0 with Fr::zero()   no counterpart in the reference
 *   bn254_fr_add_batch_dev / bn254_fr_mul_batch_dev / bn254_fr_inverse_batch_dev / bn254_fr_pow_batch_dev / bn254_fr_interpret_batch_dev /
 *   bn254_fr_sqrt_batch_dev  the same six on device-resident arrays, asynchronous on the caller's stream
 *   bn254_fr_ntt_batch     out[t n + k] = sum_j in[t n + j] s^j w_n^(j k), or the inverse map: the polynomial <-> its evaluations over the subgroup of
 *                          order n = 2^log_n (on the coset s H); no counterpart in the reference - the convention is ark-bn254's root of unity
 *   bn254_fr_ntt_batch_dev the same on device-resident arrays, asynchronous on the caller's stream; bn254_fr_root_of_unity  w_n, on the host
 *   bn254_fr_dot_batch     out[j] = sum of coeff[t] * x[index[t]] over t in [offsets[j], offsets[j+1]): a sparse matrix in CSR form times a vector over Fr
 *                          (lib.rs:33-53 Add and Mul, folded per row); no counterpart in the reference - the witness map of an R1CS
 *   bn254_fr_dot_batch_dev the same on device-resident coeff, index, x and out, asynchronous on the caller's stream
 *   bn254_fr_scan_batch    out[t] = a[t] * out[t-1] + b[t] over the terms of every segment, from init[j]: segmented prefix sums, prefix products, powers and
 *                          Horner's rule over Fr (lib.rs:33-53 Add and Mul, chained per segment); no counterpart in the reference
 *   bn254_fr_scan_batch_dev the same on device-resident a, b, init and out, asynchronous on the caller's stream
 *   bn254_fr_mle_eq        out[i] = prod_j (bit j of i ? z[j] : 1 - z[j]): the table of eq(z, .) over the hypercube of nv variables (lib.rs:33-53 Sub and Mul);
 *                          bn254_fr_mle_fold  out[i] = in[i] + r * (in[i + len/2] - in[i]): binds the most significant variable of a multilinear table;
 *                          bn254_fr_sumcheck_round  the round polynomial of a sum of products of tables at t = 0 .. degree; none has a counterpart in the reference
 *   bn254_fr_mle_eq_dev / bn254_fr_mle_fold_dev / bn254_fr_sumcheck_round_dev  the same three on device-resident tables, asynchronous on the caller's stream
 *   bn254_fr_sumcheck_fold_round  bn254_fr_mle_fold of all the tables of a sumcheck by r and bn254_fr_sumcheck_round of the folded tables in one pass: the step
 *                          of a prover between two challenges; no counterpart in the reference
 *   bn254_fr_sumcheck_fold_round_dev  the same on device-resident tables, in place if asked, asynchronous on the caller's stream
 *   bn254_fr_mle_quotients  out[0] = f(z) and out[2^j + i] = q_j[i], the nv quotient tables of f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1}) for the multilinear
 *                          table f: the field work of a multilinear KZG (PST) opening; no counterpart in the reference
 *   bn254_fr_mle_quotients_dev  the same on a device-resident table, asynchronous on the caller's stream
 *   bn254_fr_poseidon_batch  out[i] = Poseidon(in[i * arity .. (i + 1) * arity)), the circomlib / iden3 instance over Fr (x^5, t = arity + 1, R_F = 8, R_P = 56 / 57 / 56 / 60);
 *                          bn254_fr_poseidon_permute_batch  the permutation itself on n states of t records;  bn254_fr_merkle_tree  every node of the binary
 *                          tree of hash(left, right) over 2^log_n leaves; none has a counterpart in the reference
 *   bn254_fr_poseidon_batch_dev / bn254_fr_poseidon_permute_batch_dev / bn254_fr_merkle_tree_dev  the same three on device-resident records, asynchronous on the caller's stream
 *   bn254_fr_poseidon_ex_batch  circomlib's PoseidonEx(n_inputs, n_outs) with an initialState for 1 .. 16 inputs (t = 2 .. 17): the first n_outs elements
 *                          of permute([init, x_1 .. x_n]);  bn254_fr_poseidon_chain_batch  one digest per variable-length record (CSR offsets), PoseidonEx(rate, 1)
 *                          chained through its initialState under this project's own framing; neither has a counterpart in the reference
 *   bn254_fr_poseidon_ex_batch_dev / bn254_fr_poseidon_chain_batch_dev  the same two on device-resident records, asynchronous on the caller's stream
 *   bn254_g{1,2}_compress_batch / bn254_g{1,2}_decompress_batch  points <-> x and one sign bit (32 / 64 bytes) in the byte layouts ark-serialize and gnark-crypto
 *                          describe; decompression recovers y by a square root on the device and checks curve and subgroup; no counterpart in the reference
 *   bn254_g{1,2}_compress_batch_dev / bn254_g{1,2}_decompress_batch_dev  the same four on device-resident records, asynchronous on the caller's stream
 *   bn254_g1_map_to_curve_batch  out[i] = map_to_curve(u[i] mod q), the Shallue-van de Woestijne map of RFC 9380 for y^2 = x^3 + 3 (Z = 1);
 *                          bn254_g1_hash_to_curve_uniform_batch  out[i] = map(u0) + map(u1) over 96 uniform bytes (hash_to_field with L = 48), normalised;
 *                          bn254_g1_hash_to_curve_batch  the same behind expand_message_xmd over SHA-256 on the device, one message per lane; none has a
 *                          counterpart in the reference
 *   bn254_g1_map_to_curve_batch_dev / bn254_g1_hash_to_curve_uniform_batch_dev / bn254_g1_hash_to_curve_batch_dev  the same three on device-resident records,
 *                          asynchronous on the caller's stream
 *   bn254_g2_map_to_curve_batch  out[i] = map_to_curve(u[i]), the same map over Fq2 for the twist y^2 = x^3 + b' (Z = 1); the result is on the twist
 *                          and NOT in G2;  bn254_g2_clear_cofactor_batch  out[i] = [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P), normalised: a point of G2 for
 *                          any point P of the twist;  bn254_g2_hash_to_curve_uniform_batch  out[i] = clear(map(u0) + map(u1)) over 192 uniform bytes;
 *                          bn254_g2_hash_to_curve_batch  the same behind expand_message_xmd over SHA-256 on the device, one message per lane; none has a
 *                          counterpart in the reference, and neither the constants nor the outputs are checked against gnark-crypto or any other library
 *   bn254_g2_map_to_curve_batch_dev / bn254_g2_clear_cofactor_batch_dev / bn254_g2_hash_to_curve_uniform_batch_dev / bn254_g2_hash_to_curve_batch_dev  the same
 *                          four on device-resident records, asynchronous on the caller's stream
 *   bn254_g1_validate_batch / bn254_g2_validate_batch  status[i] = 0 when the raw record p[i] is a valid point (on the curve and, for G2, in the order-r
 *                          subgroup, by the endomorphism subgroup test), else the wire format's error number; what the Rust type system guarantees for the
 *                          reference's G1 / G2 values and a caller holding raw structs cannot know; no counterpart in the reference
 *   bn254_g1_validate_batch_dev / bn254_g2_validate_batch_dev  the same two on device-resident records, asynchronous on the caller's stream
 *   bn254_bjj_validate_batch / bn254_bjj_add_batch / bn254_bjj_mul_batch  Baby Jubjub, the twisted Edwards curve over Fr: validation of raw points,
 *                          the complete affine sum, out[i] = [k[i]] p[i];  bn254_eddsa_poseidon_challenge_batch  out[i] = Poseidon5(r8.x, r8.y, a.x, a.y,
 *                          msg);  bn254_eddsa_poseidon_verify_batch  circomlib's verifyPoseidon per row; none has a counterpart in the reference
 *   bn254_bjj_validate_batch_dev / bn254_bjj_add_batch_dev / bn254_bjj_mul_batch_dev / bn254_eddsa_poseidon_challenge_batch_dev /
 *   bn254_eddsa_poseidon_verify_batch_dev  the same five on device-resident records, asynchronous on the caller's stream
 *   bn254_bjj_pack_batch / bn254_bjj_unpack_batch  Baby Jubjub points to and from circomlib's 32-byte records (y, and the sign of x in the top bit);
 *                          bn254_eddsa_poseidon_verify_packed_batch  verifyPoseidon on a packed key and a packed 64-byte signature; none has a
 *                          counterpart in the reference
 *   bn254_bjj_pack_batch_dev / bn254_bjj_unpack_batch_dev / bn254_eddsa_poseidon_verify_packed_batch_dev  the same three on device-resident
 *                          records, asynchronous on the caller's stream
 *   bn254_grumpkin_validate_batch / bn254_grumpkin_add_batch / bn254_grumpkin_mul_batch / bn254_grumpkin_msm_batch  Grumpkin, y^2 = x^3 - 17 over Fr, the
 *                          other half of the BN254 curve cycle (order q): validation of raw points, the complete sum, out[i] = [k[i]] p[i] for
 *                          256-bit integers k, and the segmented sum out[j] = sum of [k[t]] p[t] over segment j; none has a counterpart in the
 *                          reference
 *   bn254_grumpkin_validate_batch_dev / bn254_grumpkin_add_batch_dev / bn254_grumpkin_mul_batch_dev / bn254_grumpkin_msm_batch_dev  the same four on
 *                          device-resident records, asynchronous on the caller's stream
 *   bn254_g1_ntt_batch / bn254_g2_ntt_batch  the transform of bn254_fr_ntt_batch with points for data and scalar multiplication for the product:
 *                          out[k] = normalize(sum_j [s^j w_n^(j k)] in[j]), and its inverse; no counterpart in the reference
 *   bn254_g1_ntt_batch_dev / bn254_g2_ntt_batch_dev  the same two on device-resident records, asynchronous on the caller's stream
 *   bn254_g2_precompute    coeffs[i][0..102) = q[i].to_affine().precompute().coeffs   groups/mod.rs:557-588 (Q != infinity)
 *   bn254_pairing_prepared_batch  out[i] = final_exponentiation(prepared.miller_loop(p[i]))   groups/mod.rs:486-519,768
 *   bn254_gt_mul_batch     out[i] = a[i] * b[i]                                     lib.rs:175-179, fields/fq12.rs:295-307
 *   bn254_gt_pow_batch     out[i] = a[i].pow(k[i])                                  lib.rs:171, fields/mod.rs:35-46
 * Outputs are bit-identical to the reference's on the same inputs (pairing values are canonical field elements; scalar
 * multiples are compared after `normalize()` because Jacobian coordinates depend on the addition chain).
 *
 * Error behaviour: the reference path is infallible for valid points (the `expect` at groups/mod.rs:768 cannot fire);
 * a point at infinity in either argument gives Gt::one() (groups/mod.rs:766).  So the only failures are device failures:
 * every function returns 0 on success or a negative BN254_E_* / positive hipError_t code; nothing panics, throws or
 * aborts across this boundary.  Inputs are trusted to be valid subgroup points exactly as the Rust type system guarantees
 * for G1/G2 values; behaviour on other limb patterns is unspecified (but memory safe).  bn254_g{1,2}_validate_batch check raw structs.
 *
 * Sizes: n is limited by device memory only.  Batches are cut internally into sub-launches of at most one machine round, and the
 * context-owned tables (final exponentiation: 4 KB, Gt::pow: 14.8 KB per pairing) are sized for ONE round - 264 MB / 970 MB on an
 * MI355X whatever n is.  Up to 3584 pairings (3328 final exponentiations) per call (the tail of every multi-pairing: exactly one) run one per
 * WAVE instead of one per lane pair: a pairing in 1.0 ms instead of 4.2 ms, a final exponentiation in 0.5 ms instead of 2.0 ms; from
 * there up to 16384 per call a pairing runs on FOUR lanes (2.7 ms); above, on lane pairs (BN254_OPT_* below move the thresholds).
 *
 * Ownership: the caller owns every buffer passed in; the library owns device memory and streams inside a context and keeps
 * no pointer after a call returns.  A context is bound to one GPU.  There is NO CPU fallback: without a usable MI355X the
 * calls fail with BN254_E_NO_DEVICE.
 *
 * Threading (the reference's `pairing` is a pure function and its types are Send + Sync, lib.rs:55-61):
 *   - every HOST-BUFFER entry point is safe to call from any number of threads on the same context, including ctx == NULL
 *     (a process-wide default context per HIP device).  bn254_pairing_batch and bn254_g{1,2}_mul_batch arbitrate per pipeline
 *     slot: two callers with batches of up to one machine round (256 pairings per CU: 2^16 on an MI355X) run concurrently on two
 *     streams (the number of streams the GPU overlaps without loss), further callers and multi-chunk batches queue; every other
 *     entry point serialises its callers on the context (bn254_pairing_product_batch too, except when every segment holds one pair: then
 *     it IS bn254_pairing_batch; likewise bn254_g{1,2}_msm_batch, which are bn254_g{1,2}_mul_batch when every segment holds one term;
 *     bn254_g{1,2}_msm serialise on the context on either route, except for n == 1 below the bucket threshold: bn254_g{1,2}_mul_batch again).
     bn254_g{1,2}_mul_base_batch serialise on the context as well (they hold its mutex for the call: lookup or build of the base's table,
     staging, launches, copy back).
     bn254_g{1,2}_normalize_batch and bn254_g{1,2}_eq_batch serialise on the context in the same way (its mutex for the call).
     bn254_fr_{add,mul,inverse,pow,interpret}_batch serialise on the context in the same way (its mutex for the whole call).
     bn254_fr_ntt_batch serialises on the context in the same way (its mutex for the whole call); bn254_fr_root_of_unity touches no
     context and no device.
     bn254_g{1,2}_ntt_batch serialise on the context in the same way (its mutex for the whole call); bn254_g{1,2}_ntt_batch_dev run under
     the scratch guard like the other _dev entry points that use context-owned scratch.
     bn254_fr_dot_batch serialises on the context in the same way (its mutex for the whole call).
     bn254_fr_scan_batch serialises on the context in the same way (its mutex for the whole call).
     bn254_fr_mle_eq, bn254_fr_mle_fold and bn254_fr_sumcheck_round serialise on the context in the same way (its mutex for the whole call).
     bn254_fr_sumcheck_fold_round serialises on the context in the same way (its mutex for the whole call).
     bn254_fr_mle_quotients serialises on the context in the same way (its mutex for the whole call).
     bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch and bn254_fr_merkle_tree serialise on the context in the same way (its mutex for the whole call).
     bn254_fr_poseidon_ex_batch and bn254_fr_poseidon_chain_batch serialise on the context in the same way (its mutex for the whole call).
     bn254_g{1,2}_compress_batch and bn254_g{1,2}_decompress_batch serialise on the context in the same way (its mutex for the whole call).
     bn254_g1_map_to_curve_batch, bn254_g1_hash_to_curve_uniform_batch and bn254_g1_hash_to_curve_batch serialise on the context in the same way (its
     mutex for the whole call).
     bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch, bn254_g2_hash_to_curve_uniform_batch and bn254_g2_hash_to_curve_batch serialise on the
     context in the same way (its mutex for the whole call).
     bn254_g1_validate_batch and bn254_g2_validate_batch serialise on the context in the same way (its mutex for the whole call).
     bn254_bjj_validate_batch, bn254_bjj_add_batch, bn254_bjj_mul_batch, bn254_eddsa_poseidon_challenge_batch and bn254_eddsa_poseidon_verify_batch
     serialise on the context in the same way (its mutex for the whole call).
     bn254_fr_sqrt_batch, bn254_bjj_pack_batch, bn254_bjj_unpack_batch and bn254_eddsa_poseidon_verify_packed_batch serialise on the context in
     the same way (its mutex for the whole call).
     bn254_grumpkin_validate_batch, bn254_grumpkin_add_batch, bn254_grumpkin_mul_batch and bn254_grumpkin_msm_batch serialise on the context in the
     same way (its mutex for the whole call).
 *     bn254_pairing_product_batch_prepared_native serialises on the context like them; its handle is immutable and shared freely.
 *     Use one context per thread (or bn254_multi_*) for more overlap;
 *     bn254_ctx_set_option is atomic, but set options before concurrent use: a call in flight may run some
 *     of its launches under the old and some under the new setting (same bytes either way);
 *   - the *_dev entry points are asynchronous on the caller's stream.  Context-owned scratch (the final-exponentiation table,
 *     the product workspace) is ordered across streams with events, so calls on different streams of one context are safe
 *     and serialise on that scratch; the caller still owns the ordering of its OWN buffers between streams.
 *     bn254_pairing_product_batch_dev and bn254_g{1,2}_msm_batch_dev read their HOST `offsets` before they return (the launches are planned
 *     from them), and so does bn254_pairing_product_batch_prepared_native_dev (its `d_q_index` is device memory and read by the kernels only);
 *     the term workspace, window tables and work list of bn254_g{1,2}_msm_batch_dev are such context-owned scratch, and so is everything
 *     bn254_g{1,2}_msm_dev keeps (sorted indices, counts, buckets, partial sums, tail terms).  bn254_g{1,2}_msm_dev plans its launches from
 *     upper bounds and reads nothing back; it synchronises the caller's stream only in a call that changes the window width (the tail's
 *     scalars are rebuilt and uploaded then), and briefly on the upload of the tail's work list like bn254_g{1,2}_msm_batch_dev.
 *     bn254_g{1,2}_msm_prepared_dev is bn254_g{1,2}_msm_dev in all of this (the same workspace, its own tail scalars per window width); the
 *     handle it reads is not scratch: it must outlive the work enqueued against it.  bn254_g{1,2}_msm_prepare_dev builds in the context's
 *     workspace under the same ordering.  The host-buffer forms serialise on the context (its mutex for the call).
     The fixed-base tables of bn254_g{1,2}_mul_base_batch_dev are context-owned scratch of the same kind: a table is looked up, built and read
     under the same event ordering, so a slot is never rebuilt while a launch on another stream may still read it.  The call reads its HOST
     `base` before it returns (compared with the cached keys; copied to pinned staging on a miss).  It waits on the host only for the copy of
     the previous miss's base, and - once per context and group - synchronises `stream` when it uploads the scalars the tables are built with.
     bn254_g{1,2}_normalize_batch_dev keep the prefix products of a sub-launch in context-owned scratch under the same event ordering;
     bn254_g{1,2}_eq_batch_dev use no scratch.  Neither reads anything back nor waits on the host.
     bn254_fr_inverse_batch_dev keeps the prefix products of a sub-launch in context-owned scratch under the same event ordering;
     bn254_fr_{add,mul,pow,interpret}_batch_dev use no scratch.  None of the five waits on anything or reads anything back.
     bn254_fr_ntt_batch_dev keeps its twiddle tables and the arrays between its passes in context-owned scratch under the same event
     ordering: a table is built, rebuilt (the shift's) and read only by a stream that has waited for the last launch that may read it.  It
     reads its HOST `shift` before it returns (the few field operations on it run on the host), waits on nothing and reads nothing back.
     bn254_fr_dot_batch_dev reads its HOST `offsets` before it returns (the launches are planned from them; its `d_index` is device memory and
     read by the kernels only); its work list and partial sums are context-owned scratch under the same event ordering.  It waits on the
     host only for the upload of the previous work list that went through the same pinned staging, and reads nothing back.
     bn254_fr_scan_batch_dev reads its HOST `offsets` before it returns in the same way; its work list, the maps of its pieces and their
     carries are context-owned scratch under the same event ordering, and it too waits on the host only for the previous upload through the
     pinned staging and reads nothing back.
     bn254_fr_mle_eq_dev and bn254_fr_mle_fold_dev use no scratch; bn254_fr_mle_fold_dev reads its HOST `r` and bn254_fr_sumcheck_round_dev its HOST
     group description before they return (both travel as kernel arguments: nothing is uploaded).  The partial sums of
     bn254_fr_sumcheck_round_dev are context-owned scratch under the same event ordering.  None of the three waits on anything or reads
     anything back.
     bn254_fr_sumcheck_fold_round_dev reads its HOST `r` and group description before it returns (kernel arguments again); its partial sums are
     the scratch of bn254_fr_sumcheck_round_dev under the same event ordering, so the two serialise on it across streams.  It waits on
     nothing and reads nothing back.
     bn254_fr_mle_quotients_dev reads its HOST `z` before it returns (the challenges of a pass travel as kernel arguments: nothing is
     uploaded).  The working table between its passes is context-owned scratch under the same event ordering - the buffer the partial sums
     of bn254_fr_sumcheck_round_dev use, so the two serialise on it across streams.  It waits on nothing and reads nothing back.
     bn254_fr_poseidon_batch_dev, bn254_fr_poseidon_permute_batch_dev and bn254_fr_merkle_tree_dev use no scratch and no host operand: the levels of a
     tree are launches in stream order that read what the level before wrote into the caller's `nodes`.  None of the three waits on anything
     or reads anything back, so any number of threads may issue them on one context, each on its own stream and buffers.
     bn254_fr_poseidon_ex_batch_dev and bn254_fr_poseidon_chain_batch_dev read the constants of their width from a context-owned table that is derived on
     the host and uploaded with a BLOCKING copy at the first use of the width on the context, under a mutex of its own, and never written again:
     a launch enqueued after that call returned - on any stream, by any thread - finds it in place.  That first call of a width therefore blocks
     for the derivation and the copy (milliseconds); every later call waits on nothing.  bn254_fr_poseidon_ex_batch_dev uses no scratch and no host
     operand.  bn254_fr_poseidon_chain_batch_dev reads its HOST `offsets` before it returns and uploads them through the work-list staging the
     segmented calls share, under the same event ordering, so it serialises with them across streams.  Neither reads anything back.
     bn254_g{1,2}_compress_batch_dev and bn254_g{1,2}_decompress_batch_dev use no scratch and no host operand either, wait on nothing and read
     nothing back (d_status stays on the device): any number of threads may issue them on one context, each on its own stream and buffers.
     bn254_g1_map_to_curve_batch_dev, bn254_g1_hash_to_curve_uniform_batch_dev and bn254_g1_hash_to_curve_batch_dev use no scratch either: one launch
     per sub-launch does the field reduction, both maps, the sum and the normalisation.  bn254_g1_hash_to_curve_batch_dev reads its HOST `dst`
     before it returns (the tag travels as a kernel argument: nothing is uploaded).  None of the three waits on anything or reads anything
     back, so any number of threads may issue them on one context, each on its own stream and buffers.
     bn254_g2_map_to_curve_batch_dev, bn254_g2_clear_cofactor_batch_dev, bn254_g2_hash_to_curve_uniform_batch_dev and bn254_g2_hash_to_curve_batch_dev
     use no scratch either: one launch per sub-launch does the field reduction, both maps, the sum, the cofactor clearing and the
     normalisation.  bn254_g2_hash_to_curve_batch_dev reads its HOST `dst` before it returns.  None of the four waits on anything or reads
     anything back, so any number of threads may issue them on one context, each on its own stream and buffers.
     bn254_g1_validate_batch_dev and bn254_g2_validate_batch_dev use no scratch and no host operand either: one launch per sub-launch compares
     the words with q, checks the curve equation and (G2) runs the subgroup test.  Neither waits on anything or reads anything back (d_status
     stays on the device), so any number of threads may issue them on one context, each on its own stream and buffers.
     bn254_bjj_validate_batch_dev, bn254_bjj_add_batch_dev, bn254_bjj_mul_batch_dev, bn254_eddsa_poseidon_challenge_batch_dev and
     bn254_eddsa_poseidon_verify_batch_dev use no scratch and no host operand either: one launch per sub-launch does all of a record's work - the
     verifier hashes, runs its joint chain and compares in one lane (each lane's window table is its own private memory).  None of the five waits
     on anything or reads anything back, so any number of threads may issue them on one context, each on its own stream and buffers.
     bn254_fr_sqrt_batch_dev, bn254_bjj_pack_batch_dev, bn254_bjj_unpack_batch_dev and bn254_eddsa_poseidon_verify_packed_batch_dev are of the same
     kind: no scratch, no host operand, one launch per sub-launch (the packed verifier unpacks its two points in the lane that verifies), nothing
     waited on or read back, so any number of threads may issue them on one context, each on its own stream and buffers.
     bn254_grumpkin_validate_batch_dev, bn254_grumpkin_add_batch_dev and bn254_grumpkin_mul_batch_dev are of the same kind: no scratch, no host
     operand, one launch per sub-launch (each lane's window table is its own private memory), nothing waited on or read back, so any number of
     threads may issue them on one context, each on its own stream and buffers.  bn254_grumpkin_msm_batch_dev reads its HOST `offsets` before
     it returns and keeps its partial sums in context-owned scratch, bracketed by the scratch event like bn254_fr_dot_batch_dev's: two streams
     on one context serialise on it instead of racing.  It waits on nothing and reads nothing back.
 */
#ifndef BN254_HIP_H
#define BN254_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } bn_fr;                    /* 32 B  */
typedef struct { uint64_t x[4], y[4], z[4]; } bn_g1;        /* 96 B  */
typedef struct { uint64_t x[8], y[8], z[8]; } bn_g2;        /* 192 B: each coordinate = (c0[4], c1[4]) */
typedef struct { uint64_t c[48]; } bn_gt;                   /* 384 B: c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1 */

/* one line-function coefficient of a prepared G2 point: the reference's EllCoeffs {ell_0, ell_vw, ell_vv: Fq2}
   (groups/mod.rs:472-476); a prepared point is 102 of them in schedule order (G2Precomp.coeffs, groups/mod.rs:478-483) */
typedef struct { uint64_t ell_0[8], ell_vw[8], ell_vv[8]; } bn_ell_coeffs;   /* 192 B */
#define BN254_PREPARED_COEFFS 102

typedef struct bn254_ctx bn254_ctx;

enum {
    BN254_OK = 0,
    BN254_E_NO_DEVICE = -1,     /* no HIP device / device index out of range */
    BN254_E_BAD_ARG = -2,       /* null pointer with n > 0, n too large */
    BN254_E_ALLOC = -3,         /* device allocation failed */
    BN254_E_COMM = -4,          /* RCCL / peer exchange of the multi-device product failed */
    BN254_E_INTERNAL = -5       /* an unexpected C++ exception was stopped at the boundary (nothing unwinds across it) */
    /* positive values are hipError_t codes */
};

/* ---- contexts ------------------------------------------------------------------------------------------------------ */
int bn254_device_count(void);
int bn254_ctx_create(int device, bn254_ctx **out);
void bn254_ctx_destroy(bn254_ctx *ctx);
const char *bn254_error_string(int code);
/* Kept for ABI compatibility: 1 = one pairing per lane PAIR (with its one-per-wave and four-lane siblings, chosen by batch size) is the only
   mapping; 0 (one pairing per lane: the test double of rounds 1-4, now tests/testdouble/) is rejected with BN254_E_BAD_ARG. */
int bn254_ctx_set_mapping(bn254_ctx *ctx, int mapping);

/* ---- tunables ---------------------------------------------------------------------------------------------------------
   Every policy of the host side is a per-context option whose default is derived from the device the context is bound to (its
   compute-unit count, `CUs` below); the call paths read nothing from the environment.  value < 0 restores the default;
   bn254_ctx_get_option reports the EFFECTIVE value - or -1 for the four options whose default is decided PER CALL from the batch
   size (BN254_OPT_PRODUCT_CHUNK / _PER_WAVE / _BFLY, BN254_OPT_PIPELINE_CHUNK; likewise BN254_OPT_MSM_WINDOW_BITS) while none is set explicitly.  The size options
   (BN254_OPT_WAVE_PAIRING_MAX, _WAVE_FE_MAX, _QUAD_MAX, _ROUND_PAIRS, _PIPELINE_CHUNK) accept at most 2^22: what one launch addresses
   with 32-bit offsets; a value above is rejected with BN254_E_BAD_ARG (larger batches are cut into sub-launches regardless).  ctx == NULL addresses the default context of the current device.  An option
   may be changed at any time; a call in flight may see the old or the new value between two of its launches - harmless, because
   every option selects between kernels that return the same bytes (the one exception is stated at BN254_OPT_GT_POW_MODE).
   For experiments only, the variables BN254_WAVE_PAIRING_MAX, BN254_WAVE_FE_MAX, BN254_QUAD_MAX, BN254_MILLER_SHARED, BN254_GT_POW_MODE,
   BN254_PRODUCT_CHUNK / _PER_WAVE / _BFLY, BN254_ROUND_PAIRS, BN254_PIPELINE_CHUNK / _SLOTS, BN254_STREAM_STOP_AT_ERROR, BN254_MSM_BUCKET_MIN, BN254_MSM_WINDOW_BITS, BN254_MSM_CHUNK, BN254_MULTI_EXCHANGE (rccl | peer) and
   BN254_MULTI_AFFINITY (0: no thread pinning) are
   read ONCE per process, when the first context is created, and seed the options of every context created afterwards. */
enum {
    BN254_OPT_WAVE_PAIRING_MAX = 1, /* pairings (or Miller loops that only meet a final exponentiation) per call up to which ONE PER WAVE
                                       runs (csrc/bn254_kernels_w.hip).  Default 14 x CUs (3584): where it is level with the four-lane
                                       kernels on 256 CUs (profiles/r04_wave_latency.json), 13 workgroups of 11.5 KB LDS per CU */
    BN254_OPT_WAVE_FE_MAX = 2,      /* the same for final exponentiations.  Default 13 x CUs */
    BN254_OPT_QUAD_MAX = 3,         /* pairings per call up to which (and above the two options before) a pairing is spread over FOUR lanes
                                       instead of two (csrc/bn254_kernels_q.hip): the faster mapping while lane pairs would leave SIMDs
                                       empty.  Default 64 x CUs (16384): half a machine round of lane pairs */
    BN254_OPT_MILLER_SHARED = 4,    /* pairs per lane pair on ONE accumulator in the multi-pairing's Miller loop: 1, 2 or 4; 0 (default):
                                       4 from four machine rounds of pairs on, 2 from two, else 1 */
    BN254_OPT_GT_POW_MODE = 5,      /* Gt::pow chain: 0 (default) Frobenius decomposition - exact for elements whose ORDER DIVIDES r, which
                                       is everything the reference's Gt can hold; 2 one-dimensional cyclotomic chain - exact for ANY
                                       cyclotomic element; 1 the reference's general chain for everything.  THE ONE OPTION THAT CAN
                                       CHANGE RESULTS: only for inputs outside the r-torsion, which the reference's typed API cannot
                                       produce (see bn254_gt_pow_batch) */
    BN254_OPT_PRODUCT_CHUNK = 6,    /* shape of the one-launch Fq12 product tree: values per lane pair (1..4096), */
    BN254_OPT_PRODUCT_PER_WAVE = 7, /* live lane pairs per wave (1..32), */
    BN254_OPT_PRODUCT_BFLY = 8,     /* butterfly levels inside a wave (0..5).  Defaults: by size, profiles/r03p_product_shape_sweep.txt */
    BN254_OPT_ROUND_PAIRS = 9,      /* pairings per launch of the lane-pair kernels ("one machine round").  Default 256 x CUs: two waves
                                       on every SIMD; larger batches run as equal sub-launches of at most this size */
    BN254_OPT_PIPELINE_CHUNK = 10,  /* pairings per chunk of the pipelined host-buffer path.  Default: the sub-launch size */
    BN254_OPT_PIPELINE_SLOTS = 11,  /* chunks in flight, 1..4.  Default 2: the number of streams the GPU overlaps without loss */
    BN254_OPT_STREAM_STOP_AT_ERROR = 12, /* bn254_g{1,2}_decode_stream: 1 = the crate's own behaviour - its Decodable returns Err at the first bad
                                       record (groups/mod.rs:165-175) -: `count` ends WITH the first record whose status is non-zero and
                                       `consumed` behind it (out[] and status[] beyond `count` are unspecified: the batch decoder has
                                       already run over the records that follow); 0 (default): decode every record, report every status */
    BN254_OPT_MSM_BUCKET_MIN = 13,  /* bn254_g{1,2}_msm: terms from which the bucket method runs; below, the one-segment bn254_g{1,2}_msm_batch launches.
                                       0 = always buckets.  Default: the measured crossover, 2^19 for G1 (the value reported) and 2^18 for G2
                                       (profiles/r10_msm_bucket.txt) */
    BN254_OPT_MSM_WINDOW_BITS = 14, /* window width c of the bucket method, 1..16.  Default: by n, the best measured width per size (8 ... 14) */
    BN254_OPT_MSM_CHUNK = 15,       /* terms per pass of the bucket method, 1..2^22 (positions are 32-bit).  Default 2^20 */
    BN254_OPT_COUNT_ = 16
};
int bn254_ctx_set_option(bn254_ctx *ctx, int key, long value);
int bn254_ctx_get_option(bn254_ctx *ctx, int key, long *value);
/* the RAW state of an option: the explicitly set value, or -1 while the default is in effect (what a scoped set / restore must save) */
int bn254_ctx_get_option_raw(bn254_ctx *ctx, int key, long *value);

/* ---- host-buffer entry points (what a binding of the reference's API calls) ------------------------------------------ */
/* ctx == NULL uses a process-wide default context on the current HIP device. */
int bn254_pairing_batch(bn254_ctx *ctx, const bn_g1 *p, const bn_g2 *q, bn_gt *out, size_t n);
int bn254_pairing_product(bn254_ctx *ctx, const bn_g1 *p, const bn_g2 *q, size_t n, bn_gt *out);
/* Batched multi-pairing: m independent products in one call - a block of Groth16 / EIP-197-style pairing checks.  Segments are given in
   CSR form: offsets[0..m] with offsets[0] == 0, non-decreasing, n = offsets[m] pairs, and
       out[j] = fold(Gt::one(), |acc, i| acc * pairing(p[i], q[i])) over i in [offsets[j], offsets[j+1]),   j < m
   (shootout/main.rs:11-16 per segment, lib.rs:175-183), bit-identical to that fold.  An empty segment gives Gt::one(); a pair with a point at
   infinity contributes one (groups/mod.rs:766).  ONE final exponentiation per segment.  Route (the existing thresholds choose it): at most
   BN254_OPT_WAVE_PAIRING_MAX pairs and BN254_OPT_WAVE_FE_MAX segments - Miller loops one per wave, then one wave per segment folds at most 16
   values and exponentiates (two launches); otherwise chunks of at most one machine round (BN254_OPT_ROUND_PAIRS pairs, cut at segment
   boundaries; a longer segment carries its partial product across chunks), a segmented Fq12 fold on lane pairs (pieces of at most 16 values
   per lane pair, ceil(log16 L) levels for a segment of L values) and the batched final exponentiation of the m values.  Every segment of
   length 1: exactly bn254_pairing_batch.  Workspace: one round of Miller values plus 24 bytes of work list per segment and per 16 pairs.
   Made for many short segments: ONE long segment folds on ever fewer lane pairs (5000 pairs: ~0.9 ms of fold) - a caller with a single
   product, or a few thousand-pair ones, is better served by bn254_pairing_product, whose one-launch product tree needs ~0.1 ms.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): offsets == NULL with m > 0, offsets[0] != 0, decreasing offsets,
   n > 2^40, a NULL p / q (n > 0) or out.  m == 0 returns BN254_OK and writes nothing. */
int bn254_pairing_product_batch(bn254_ctx *ctx, const bn_g1 *p, const bn_g2 *q, const size_t *offsets, size_t m, bn_gt *out);
int bn254_g1_mul_batch(bn254_ctx *ctx, const bn_g1 *p, const bn_fr *k, bn_g1 *out, size_t n);
int bn254_g2_mul_batch(bn254_ctx *ctx, const bn_g2 *p, const bn_fr *k, bn_g2 *out, size_t n);
/* Fixed-base scalar multiplication: out[i] = normalize(base[0] * k[i]) for i < n - key and SRS generation ([tau^i] G), G::random
   (G::one() * Fr::random(), groups/mod.rs:220-222), Pedersen / ElGamal-style uses of one or two generators.  Bit-identical to
   bn254_g{1,2}_mul_batch on n copies of `base` with the same k (normalisation makes the image unique).  `base` is ONE point in any Jacobian
   representation; a base at infinity or k[i] == 0 gives G::zero() = (0, 1, 0); G2 as for bn254_g2_mul_batch: an order-r subgroup point.
   How: per base a table of the affine multiples d * 2^(12 w) * base, w < 22, d = 1 .. 2048 (signed 12-bit windows, the fastest of the measured
   8 / 10 / 12; 45 056 entries in the device's 9 x 29-bit limbs: 3 604 480 bytes for G1, 7 208 960 for G2), after which a multiplication is at
   most 22 mixed additions, no doubling, and the normalisation.  The context keeps the tables of the FOUR most recently used bases per group, keyed by the bytes of `base` as passed (another
   Jacobian representation of the same point is another key with an equal table): a hit launches the fixed-base kernel alone, a miss first
   builds the table on the call's stream - the tiled base times the host-known scalars d * 2^(12 w) through the kernel of
   bn254_g{1,2}_mul_batch, then a repack - and evicts the least recently used slot.  Every miss builds, whatever n is: a call with n = 1 and
   a new base costs 1.14 ms (G1) / 2.05 ms (G2) of kernel time against 0.85 / 1.07 ms for bn254_g{1,2}_mul_batch at n = 1 (the build is
   0.93 / 1.80 ms of it), so a caller whose base changes with every call wants bn254_g{1,2}_mul_batch; with the table cached the kernel
   time is a fifth of the general kernel's: 2^20 G1 scalars 2.17 against 11.42 ms, 2^18 G2 scalars 1.50 against 7.15 ms
   (profiles/r11_mul_base.txt).
   Errors (BN254_E_BAD_ARG, checked before any device is touched): a NULL base, k or out with n > 0, n > 2^40.  n == 0 returns BN254_OK and
   writes nothing.  Threading: see above - the host-buffer entry points hold the context's mutex for the call. */
int bn254_g1_mul_base_batch(bn254_ctx *ctx, const bn_g1 *base, const bn_fr *k, bn_g1 *out, size_t n);
int bn254_g2_mul_base_batch(bn254_ctx *ctx, const bn_g2 *base, const bn_fr *k, bn_g2 *out, size_t n);
/* Batched normalisation and projective equality - what `Group::normalize` (lib.rs:88-95, :131-138 over to_affine, groups/mod.rs:113-130) and
   `PartialEq for G<P>` (groups/mod.rs:83-109) do, for points that arrive raw: sums of bn254_g{1,2}_add_batch, points decoded from proofs,
   bn254_g{1,2}_mul_jacobian_dev outputs, anything about to be compared, hashed, serialized or used as a bn254_g{1,2}_mul_base_batch key.
   normalize: out[i] = (x/z^2, y/z^3, 1) in canonical Montgomery limbs; a point with z == 0 gives G::zero() = (0, 1, 0) whatever its x and y
   hold.  Bit-identical to bn254_g{1,2}_mul_batch(p, Fr::one()) on the same input - that identity is the parity definition.  `out` may be
   exactly `p` (partial overlap is outside the contract).  How: one field inversion is shared by a run of 8 consecutive points (Montgomery's
   trick: prefix products of z - one in place of a zero z -, one inversion, a backward pass), 7 products per point and an eighth of an
   inversion instead of a whole GLV / GLS chain; the run length is a constant, the fastest of the measured 1 / 4 / 8 / 16, and the bytes do
   not depend on it.  Kernel time against bn254_g{1,2}_mul_batch_dev with every scalar Fr::one() on the same points
   (profiles/r12_normalize.txt), medians of 5: G1 0.067 against 0.856 ms at n = 1 (12.9 x), 0.113 against 0.935 ms at 2^16 (8.2 x), 0.274
   against 11.15 ms at 2^20 (40.7 x); G2 0.063 against 1.054 ms at n = 1 (16.7 x), 0.125 against 1.214 ms at 2^15 (9.7 x), 0.197 against
   7.08 ms at 2^18 (35.9 x).  Run lengths 1 / 4 / 8 / 16 at the largest size: G1 0.585 / 0.253 / 0.199 / 0.191 ms, G2 0.315 / 0.143 / 0.126 /
   0.192 ms.
   eq: out[i] = 1 when a[i] and b[i] are the same group element, else 0 - both at infinity: 1; exactly one: 0; otherwise
   x1 z2^2 == x2 z1^2 and y1 z2^3 == y2 z1^3 as field elements (two squarings, six products, no inversion).
   Errors (BN254_E_BAD_ARG, checked before any device is touched): a NULL input or output with n > 0, n > 2^40.  n == 0 returns BN254_OK and
   writes nothing.  Threading: see above - the host-buffer entry points hold the context's mutex for the call. */
int bn254_g1_normalize_batch(bn254_ctx *ctx, const bn_g1 *p, bn_g1 *out, size_t n);
int bn254_g2_normalize_batch(bn254_ctx *ctx, const bn_g2 *p, bn_g2 *out, size_t n);
int bn254_g1_eq_batch(bn254_ctx *ctx, const bn_g1 *a, const bn_g1 *b, int32_t *out, size_t n);
int bn254_g2_eq_batch(bn254_ctx *ctx, const bn_g2 *a, const bn_g2 *b, int32_t *out, size_t n);
/* Segmented multi-scalar multiplication: m independent linear combinations in one call - the IC sums of a block of Groth16 checks, a*P + b*Q,
   random linear combinations of checks, aggregate keys.  Segments in CSR form: offsets[0..m] with offsets[0] == 0, non-decreasing,
   n = offsets[m] terms, and
       out[j] = normalize(fold(G::zero(), |acc, i| acc + p[i] * k[i])) over i in [offsets[j], offsets[j+1]),   j < m
   (lib.rs:103-120,88-95 for G1, :146-163,131-138 for G2).  Compared after normalize() for the reason given above for scalar multiples, and
   normalisation makes the image unique: bit-identical to the reference's fold whatever the order of additions.  A sum that is the point at
   infinity (empty segment, all scalars zero, all points at infinity, terms that cancel) is G::zero() = (0, 1, 0).  Inputs as for
   bn254_g{1,2}_mul_batch: trusted subgroup points in any Jacobian representation, canonical Montgomery Fr images.
   How: terms in chunks of one launch of the multiplication kernels (2^20 G1 / 2^19 G2 terms; a segment that crosses a cut carries its partial
   sum), each term by the GLV / GLS chain WITHOUT normalisation into a context-owned workspace, then a segmented fold with the complete
   addition (pieces of at most 4 consecutive values per lane / lane pair, ceil(log4 L) levels for a segment of L terms) whose last level
   normalises: ONE inversion per segment.  Every segment of length 1: exactly bn254_g{1,2}_mul_batch.  Workspace: one chunk of Jacobian
   terms (96 / 192 bytes each), as much again for partial sums, the window tables of bn254_g{1,2}_mul_batch and 24 bytes of work
   list per segment and per 4 terms.
   Made for many short and medium segments (verifier workloads).  There is NO bucket (Pippenger) method here: ONE prover-sized segment
   (2^20 terms) is computed correctly but at the cost of a full scalar-multiplication chain per term, and its fold levels run on ever
   fewer lanes.  One large sum belongs to bn254_g{1,2}_msm below, which has the bucket method.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): offsets == NULL with m > 0, offsets[0] != 0, decreasing offsets,
   n > 2^40, a NULL p / k (n > 0) or out.  m == 0 returns BN254_OK and writes nothing. */
int bn254_g1_msm_batch(bn254_ctx *ctx, const bn_g1 *p, const bn_fr *k, const size_t *offsets, size_t m, bn_g1 *out);
int bn254_g2_msm_batch(bn254_ctx *ctx, const bn_g2 *p, const bn_fr *k, const size_t *offsets, size_t m, bn_g2 *out);
/* One large multi-scalar multiplication: out[0] = normalize(fold(G::zero(), |acc, i| acc + p[i] * k[i])) over all n terms - exactly what
   bn254_g{1,2}_msm_batch return for the one segment offsets = {0, n}, bit for bit (normalisation makes the image unique).  Inputs as there;
   n == 0 or a sum at infinity gives G::zero() = (0, 1, 0).
   Below BN254_OPT_MSM_BUCKET_MIN terms the call IS that one-segment launch sequence.  From there on the bucket (Pippenger) method: the
   canonical integer of every scalar is cut into W = ceil(254 / c) unsigned c-bit digits (BN254_OPT_MSM_WINDOW_BITS), a counting sort groups
   the term indices by (window, digit), and the buckets are summed with the complete addition in levels of at most 16 consecutive entries per
   lane / lane pair - no serial chain depends on the scalars: n equal scalars are n / 16 lanes, then n / 128, ... .  Groups of 16 buckets are
   reduced by running sums to two points each, and these 2 W 2^c / 16 points, with host-known scalars, are one bn254_g{1,2}_msm_batch segment
   that folds, normalises once and writes out.  Calls above BN254_OPT_MSM_CHUNK terms run as several passes into the same buckets.
   Workspace (context-owned), t = min(n, chunk) terms, V = 96 / 192 bytes: 8 W t bytes of (index, key), (4 + V) W 2^c bytes of counts and
   buckets, at most (V + 4) (W t / 7 + 64) bytes of partial sums, (V + 32) W 2^c / 8 bytes of tail terms, and the workspace of the tail.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): a NULL p / k with n > 0, a NULL out, n > 2^40. */
int bn254_g1_msm(bn254_ctx *ctx, const bn_g1 *p, const bn_fr *k, size_t n, bn_g1 *out);
int bn254_g2_msm(bn254_ctx *ctx, const bn_g2 *p, const bn_fr *k, size_t n, bn_g2 *out);
/* out[i] = a[i] + b[i]  (negate_b != 0: a[i] - b[i] = a[i] + (-b[i])): `Add`/`Sub` of lib.rs:103-114,146-157 over
   groups/mod.rs:275-347.  The reference's own formulas and branches (zero operands, equal points), so the Jacobian limbs
   returned are the reference's - no normalization involved.  `Neg` is 0 - b. */
int bn254_g1_add_batch(bn254_ctx *ctx, const bn_g1 *a, const bn_g1 *b, bn_g1 *out, size_t n, int negate_b);
int bn254_g2_add_batch(bn254_ctx *ctx, const bn_g2 *a, const bn_g2 *b, bn_g2 *out, size_t n, int negate_b);
/* prepared-G2 mode: precompute once per Q (must not be infinity), then pair many P against it.  `shared` != 0: ONE coefficient
   set (102 entries) is used for every p[i]; otherwise coeffs holds n sets, set i for p[i]. */
int bn254_g2_precompute(bn254_ctx *ctx, const bn_g2 *q, bn_ell_coeffs *coeffs, size_t n);
int bn254_pairing_prepared_batch(bn254_ctx *ctx, const bn_g1 *p, const bn_ell_coeffs *coeffs, int shared, bn_gt *out, size_t n);
/* NATIVE prepared-G2 mode: the device's own counterpart of the reference's internal G2Precomp (groups/mod.rs:472-483) for callers that pair
   many P against the same Q - a verification key - or re-use a set of Q.  bn254_g2_prepare runs precompute (groups/mod.rs:557-588) ONCE per
   point and keeps the result in device memory behind an opaque handle, in the form the kernels consume: the engine's own schedule (6u+2 in
   non-adjacent form: 88 lines instead of 102), every line normalised by its ell_vw coefficient (a factor in Fq2, which the final
   exponentiation kills) and stored as multiplier operands in the 9 x 29-bit limbs of the device arithmetic - 33 792 bytes per point, a
   function of the point alone.  bn254_pairing_prepared_native_batch then computes
       out[i] = final_exponentiation(prepared.miller_loop(p[i]))  =  bn::pairing(p[i], q)          groups/mod.rs:486-519,764-771
   bit-identical to the reference (the Miller VALUE differs by subfield factors; the reference-image coefficients, for the reference's own
   known answers, are bn254_g2_precompute / bn_ell_coeffs above).  A handle made from ONE point is shared by all p[i]; a handle made from nq
   points pairs p[i] with point q_first + i (q_first + n <= nq; the host-buffer entry point uses q_first = 0).  A point at infinity in either
   argument gives Gt::one() (groups/mod.rs:766).  Calls of up to 12 x CUs pairings (3072) are served by the general path's one-pairing-per-wave kernels
   on the points kept with the handle (1.0 ms instead of the 1.7 ms a lane-pair Miller loop needs however few pairings there are; same bytes;
   BN254_OPT_WAVE_PAIRING_MAX = 0 turns that off).  The handle belongs to the context's device; it is immutable after creation, so any
   number of threads / streams may use it concurrently; destroy it after the last call that uses it has completed. */
typedef struct bn254_g2_prepared bn254_g2_prepared;
#define BN254_PREPARED_NATIVE_LINES 88
#define BN254_PREPARED_NATIVE_BYTES 33792    /* device bytes per prepared point: 88 lines x 2 lanes x 12 x 16 B (a handle holds one more record: the identity) */
int bn254_g2_prepare(bn254_ctx *ctx, const bn_g2 *q, size_t nq, bn254_g2_prepared **out);
void bn254_g2_prepared_destroy(bn254_g2_prepared *prep);
size_t bn254_g2_prepared_count(const bn254_g2_prepared *prep);           /* points in the handle */
size_t bn254_g2_prepared_bytes(const bn254_g2_prepared *prep);           /* device memory it holds */
/* copies the table to the host ([line][16-byte group][2 x point + lane] x 4 u32; for tests and inspection): bytes = BN254_PREPARED_NATIVE_BYTES x count */
int bn254_g2_prepared_export(bn254_ctx *ctx, const bn254_g2_prepared *prep, void *host_table, size_t bytes);
int bn254_pairing_prepared_native_batch(bn254_ctx *ctx, const bn_g1 *p, const bn254_g2_prepared *prep, bn_gt *out, size_t n);
/* the multi-pairing over prepared points: out[0] = fold(Gt::one(), acc * pairing(p[i], point i)) over n pairs (shootout/main.rs:11-16 with the
   G2 side prepared; n <= count, or any n against a handle of ONE point) - what a verifier with fixed G2 points evaluates.  ONE final
   exponentiation for the whole product, and from two machine rounds of pairs on (2 x 256 x CUs) two resp. four pairs share one Miller
   accumulator per lane pair: over native tables a pair has no per-step point state, so the shared loop is the line products plus a quarter of
   the squarings.  n == 0 gives Gt::one(); a point at infinity on either side contributes one (groups/mod.rs:766). */
int bn254_pairing_product_prepared_native(bn254_ctx *ctx, const bn_g1 *p, const bn254_g2_prepared *prep, size_t n, bn_gt *out);
/* Batched multi-pairing over prepared points with per-pair indices: m independent products in one call, every pair naming its prepared point -
   a block of Groth16 checks whose verifying-key points (and, prepared per block, whose proof points) live in ONE handle.  Segments in CSR form
   exactly as for bn254_pairing_product_batch (offsets[0] == 0, non-decreasing, n = offsets[m] pairs; an empty segment gives Gt::one();
   m == 0 returns BN254_OK and writes nothing), and
       out[j] = fold(Gt::one(), |acc, i| acc * pairing(p[i], point q_index[i] of prep)) over i in [offsets[j], offsets[j+1]),   j < m
   (shootout/main.rs:11-16 per segment, lib.rs:175-183, with the G2 side prepared), bit-identical to that fold, ONE final exponentiation per
   segment.  A point at infinity on either side contributes one (groups/mod.rs:766).
   q_index: n entries, each < count.  (size_t on the host; 64-bit words in device memory for the _dev entry point.)  q_index == NULL keeps the
   convention of the other prepared entry points: every pair uses point 0 of a one-point handle, pair i uses point i otherwise (n <= count).
   How: every segment of L pairs is cut into ceil(L / 4) pieces of at most four consecutive pairs; a lane pair runs one piece on ONE Miller
   accumulator over the native tables (the line products of its pairs, a quarter of the squarings - the loop of
   bn254_pairing_product_prepared_native) and writes one un-exponentiated value.  When no segment has more than four pairs (the Groth16
   shape) that value is out[j] and the batched final exponentiation runs in place: nothing is folded.  Otherwise the values go through the
   segmented fold of bn254_pairing_product_batch (chunks of one machine round of VALUES, pieces of at most 16, carry across chunks).
   Calls of at most min(12 x CUs, BN254_OPT_WAVE_PAIRING_MAX) pairs are served by bn254_pairing_product_batch's own kernels on the points kept
   with the handle, gathered by index (same bytes; BN254_OPT_WAVE_PAIRING_MAX = 0 turns that off), as for the other prepared entry points.
   Layout for speed, not for correctness: for a fixed position i inside the pieces, the lane pairs of a wave should meet ADJACENT points or ONE
   point - e.g. a block of checks laid out as [3 + j, 0, 1, 2] over a handle [beta, gamma, delta, B_0 .. B_{m-1}]: pair 0 reads adjacent
   columns, pairs 1-3 are broadcasts.  Arbitrary indices are correct, just slower.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): everything bn254_pairing_product_batch rejects, prep == NULL,
   q_index[i] >= count (the caller gets an error, never a wrong product), n > count with q_index == NULL on a handle of several points; then a
   handle that belongs to another device than the context.  The handle is immutable: any number of threads / streams may share it. */
int bn254_pairing_product_batch_prepared_native(bn254_ctx *ctx, const bn_g1 *p, const bn254_g2_prepared *prep, const size_t *q_index,
                                                const size_t *offsets, size_t m, bn_gt *out);
int bn254_gt_mul_batch(bn254_ctx *ctx, const bn_gt *a, const bn_gt *b, bn_gt *out, size_t n);
/* Gt::pow (lib.rs:171).  a[i] are Gt VALUES - what the reference's type holds: Gt::one, pairing() and products, powers, inverses of
   such (the Fq12 inside Gt is private and Gt has no decoder), all of order r.  On those the device exponentiates through the
   Frobenius decomposition (k = k0 + k1 q + k2 q^2 + k3 q^3 mod r: 68 cyclotomic squarings and 72 products instead of 252 and 64),
   which needs the order to divide r.  An element that is not even cyclotomic is detected and takes the general chain
   (fields/mod.rs:35-46 as written).  bn254_ctx_set_option(ctx, BN254_OPT_GT_POW_MODE, 2) selects the one-dimensional cyclotomic
   chain, exact for ANY cyclotomic element; 1 the general chain for everything.  One window table of 7.4 KB per lane of a sub-launch
   lives in the context.
   The same precondition holds for bn254_g2_mul_batch: the GLS decomposition multiplies correctly on the order-r subgroup of the twist -
   the only G2 values the reference's API can hold (checked decode, groups/mod.rs:178-205); other twist points are outside the contract. */
int bn254_gt_pow_batch(bn254_ctx *ctx, const bn_gt *a, const bn_fr *k, bn_gt *out, size_t n);
/* out[i] = a[i]^-1 in Fq12 (Gt::inverse, lib.rs:172 -> fields/fq12.rs:284-292); a[i] must be non-zero, as every Gt value is */
int bn254_gt_inverse_batch(bn254_ctx *ctx, const bn_gt *a, bn_gt *out, size_t n);
/* Batched scalar-field arithmetic - the crate's Fr (lib.rs:15-53) for ARRAYS of scalars: the powers of tau of a bn254_g{1,2}_mul_base_batch
   call, the products r_j * a_ji of a random linear combination of checks, Lagrange denominators, whatever feeds bn254_g{1,2}_msm*,
   bn254_g{1,2}_mul_base_batch or bn254_gt_pow_batch.  Inputs are canonical Montgomery images (< r), the bytes the reference keeps; outputs
   are canonical, hence unique, hence the reference's bytes whichever algorithm computes them.  A non-canonical input is outside the
   contract but memory safe.  `out` may be exactly `a` or exactly `b` (partial overlap is outside the contract).
   add: a + b, or a - b when negate_b != 0; `Neg` is 0 - b, as for bn254_g1_add_batch.
   inverse: Option<Fr> - ok[i] = 1 and out[i] = a[i]^-1, or ok[i] = 0 and out[i] = Fr::zero() for a[i] == 0; ok may be NULL.  One
   exponentiation by r - 2 is shared by a run of 8 consecutive elements (Montgomery's trick: prefix products - one in place of a zero
   element -, one a^(r-2), a backward pass): 3 products per element and an eighth of an exponentiation; a zero does not disturb its
   neighbours, and the bytes do not depend on the run length.
   pow: a^(canonical integer of e) (fields/mod.rs:35-46 through lib.rs:23) by a fixed, data-independent 2-bit window over the 254 bits of
   the exponent; 0^0 = 1 (the reference's loop starts from one and sees no bit), 0^e = 0 for e > 0.
   interpret: every 64-byte record as a big-endian 512-bit integer hi * 2^256 + lo, reduced mod r by two Montgomery products (lo by R^2,
   hi by R^3) and one addition.
   One element per lane as eight 32-bit words in radix 2^256 (the ABI bytes: nothing is converted), word-serial Montgomery products of
   v_mad_u64_u32, records moved as 16-byte loads and stores (device pointers of the _dev twins: 16-byte aligned).  The run length 8 and
   the 2-bit window are the shipped defaults: tools/time_fr.py times run lengths 1 / 4 / 8 / 16 and windows of 1 / 2 / 4 bits in one
   process (profiles/r13_fr.txt: the 2-bit window is the fastest, a run of 16 is 1.4 x faster than 8).
   Errors (BN254_E_BAD_ARG, checked before any device is touched): a NULL input or output with n > 0 (ok excepted), n > 2^40.  n == 0
   returns BN254_OK and writes nothing.  Batches run as sub-launches of at most 2^22 elements.  Threading: see above - the host-buffer
   entry points hold the context's mutex for the whole call. */
int bn254_fr_add_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *b, bn_fr *out, size_t n, int negate_b);
int bn254_fr_mul_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *b, bn_fr *out, size_t n);
int bn254_fr_inverse_batch(bn254_ctx *ctx, const bn_fr *a, bn_fr *out, int32_t *ok, size_t n);
int bn254_fr_pow_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *e, bn_fr *out, size_t n);
int bn254_fr_interpret_batch(bn254_ctx *ctx, const uint8_t *in, bn_fr *out, size_t n);
/* Option<Fr> square roots: ok[i] = 1 and out[i] the root of a[i] whose canonical integer is not above (r - 1) / 2, or ok[i] = 0 and
   out[i] = Fr::zero() for a non-residue; 0 has the root 0.  ok may be NULL and out may be a, as for bn254_fr_inverse_batch.  r - 1 = 2^28 t:
   one exponentiation by (t - 1) / 2 and a correction by a power of a fixed element of order 2^28, found digit by digit; every lane runs the
   same instruction stream whatever its element holds.  Elements are taken as canonical Montgomery images like everywhere in this family. */
int bn254_fr_sqrt_batch(bn254_ctx *ctx, const bn_fr *a, bn_fr *out, int32_t *ok, size_t n);
/* Number-theoretic transforms over Fr: `count` transforms of n = 2^log_n elements each (log_n 0 .. BN254_NTT_LOG_MAX), transform t in
   records [t n, (t + 1) n), natural order in and out - what moves a polynomial between its coefficients and its evaluations over the
   subgroup H of order n of Fr*, plain and on a coset: the quotient (a b - c) / Z_H of a Groth16 prover, the inverse transform in front of
   a KZG / PLONK commitment by bn254_g1_msm.
   Root: w_n = w_28^(2^(28 - log_n)) with w_28 = 5^((r-1)/2^28) = 19103219067921713944291392827692070036145651957329286315305642004821462161904
   (r - 1 is divisible by 2^28; 5 is a quadratic non-residue, so w_28^(2^27) = r - 1) - the convention of arkworks' ark-bn254.  Every size
   uses this ONE root, so the domains of different sizes nest.  bn254_fr_root_of_unity writes w_n as a Montgomery image (log_n 0 .. 28;
   host only: it touches no context and no device).
   forward (inverse == 0):  out[t n + k] = sum_j in[t n + j] s^j w_n^(j k)              - the polynomial with coefficients `in` at s w_n^k
   inverse (inverse != 0):  out[t n + j] = s^-j n^-1 sum_k in[t n + k] w_n^(-j k)       - the coefficients back from such evaluations
   s is the coset shift: `shift` is ONE element in HOST memory in both forms, read before the call returns (like `base` of
   bn254_g1_mul_base_batch_dev), NULL for s = 1.  Inputs are canonical Montgomery images; every output is canonical, hence unique, hence
   independent of the algorithm.  `out` may be exactly `in` (partial overlap is outside the contract).
   How: a transform is ceil(log_n / T) passes over global memory with T = 9: a workgroup of 256 lanes holds a tile of 2^T elements (16 KiB)
   in LDS, beside the up to 2^(T-1) stage twiddles of its pass (8 KiB), and runs up to T radix-2 stages on it.  A pass is a step of a Stockham autosort, so no pass reverses bits in global memory; the
   stages of a transform are split evenly over its passes (2^20: 7 + 7 + 6, 2^24: 8 + 8 + 8), and a tile of a pass of t < T stages is 2^(T - t) small
   transforms whose rows are runs of adjacent records.  The coset powers and n^-1 are folded into the first and the last pass.  Twiddles
   are factored: w_24^i and w_24^(2^12 i) for i < 2^12 serve every size and both directions (a stage's twiddle is one load - a workgroup copies those of its pass to LDS once -; the twiddle
   between two passes is two loads and one product more per element), and a second pair of the same shape holds the powers of the last
   shift used (rebuilt when the shift changes, or - for an inverse transform, whose pair carries n^-1 - the size or the direction).  Both are built on the device on first use and kept: 512 KiB per context.
   A transform of more than one pass also keeps one array of the size of a group of transforms (up to 2^22 elements, or one larger
   transform: 512 MB at 2^24) per context, two for an odd number of passes in place.  A full table of 16 n bytes was not built or measured.
   Measured on an MI355X (tools/time_ntt.py; the full table is profiles/r14_ntt.txt): one forward transform of 2^20 takes 0.255 ms of
   kernel time and one of 2^24 4.0 ms, about 6 x the device-to-device copies of their passes and 3 - 4 x the time of their Montgomery
   products at the measured multiply-add rate, so neither floor is near.  Tile logs 8 / 9 / 10 / 11 take 0.286 / 0.256 / 0.262 / 0.252 ms
   at 2^20 and 4.33 / 3.76 / 3.75 / 4.24 ms at 2^24.  By the rule that the fastest at 2^20 ships it would be 11 (1.4 % ahead of 9); 9 ships
   instead, because 11 is 13 % slower at 2^24 and needs 80 KiB of LDS per workgroup, more than a kernel gets without asking for it.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): log_n < 0 or > BN254_NTT_LOG_MAX (> 28 for bn254_fr_root_of_unity), a
   NULL `in` or `out` with count > 0 (a NULL `out` of bn254_fr_root_of_unity), count 2^log_n > 2^40, a `shift` that is Fr::zero().
   count == 0 returns BN254_OK and writes nothing.  Calls run as sub-launches of at most 2^22 elements.  Threading: see above - the
   host-buffer entry point holds the context's mutex for the whole call. */
#define BN254_NTT_LOG_MAX 24
int bn254_fr_root_of_unity(int log_n, bn_fr *out);
int bn254_fr_ntt_batch(bn254_ctx *ctx, const bn_fr *in, bn_fr *out, int log_n, size_t count, int inverse, const bn_fr *shift);
/* The same transforms over G1 and G2: points for data, scalar multiplication for the product - what turns the powers tau^i G of a
   reference string into the Lagrange points L_j(tau) G without tau (one inverse transform), and what computes all n openings of a
   polynomial over the domain with a few transforms instead of n multi-scalar multiplications (FK20; bn_amd.kzg.lagrange_srs, open_all).
   `count` transforms of n = 2^log_n points each (log_n 0 .. BN254_GROUP_NTT_LOG_MAX), transform t in records [t n, (t + 1) n), natural
   order in and out, w_n the root of bn254_fr_root_of_unity(log_n):
   forward (inverse == 0):  out[t n + k] = sum_j [s^j w_n^(j k)] in[t n + j]
   inverse (inverse != 0):  out[t n + j] = [n^-1 s^-j] sum_k [w_n^(-j k)] in[t n + k]
   `shift` as for bn254_fr_ntt_batch: ONE element in HOST memory, read before the call returns, NULL for s = 1.
   Inputs are raw points as bn254_g{1,2}_mul_batch take them: any z, z == 0 is the point at infinity whatever x and y hold; the caller
   vouches for curve and subgroup membership.  Outputs are NORMALISED: every record holds the bytes bn254_g{1,2}_normalize_batch give for
   that group element (infinity: (0, 1, 0)), so the bytes do not depend on how the transform is scheduled.  `out` may be exactly `in`
   (partial overlap is outside the contract).
   How: log_n radix-2 Stockham stages in global memory (no bit reversal), one lane per butterfly for G1 and one lane pair for G2: the
   twiddle from the factored root tables of bn254_fr_ntt_batch, ONE GLV / GLS chain left Jacobian, then the sum and the difference by the
   complete addition (equal and opposite operands are ordinary here: a constant input doubles at every stage).  The stage whose twiddles
   are all one runs no chain: n / 2 (log_n - 1) chains per transform.  A shift, or the n^-1 of an inverse, is one further pass of n chains
   with the scalars of the shift tables.  Points stay Jacobian between the stages; the last step is the shared-inversion normalisation.
   Scratch per context: the tables of bn254_fr_ntt_batch, one array of Jacobian points of the size of a group of transforms (up to 2^22
   points: 384 MB for G1, 768 MB for G2), the window tables of one sub-launch (640 B per lane, at most 2^20 lanes) and the prefix products
   of the normalisation.  Measurements: tools/time_group_ntt.py.
   Errors (BN254_E_BAD_ARG, checked before any device is touched, in this order): log_n < 0 or > BN254_GROUP_NTT_LOG_MAX, a NULL `in` or
   `out`, count 2^log_n > 2^40, a `shift` that is Fr::zero().  count == 0 returns BN254_OK and writes nothing. */
#define BN254_GROUP_NTT_LOG_MAX 22
int bn254_g1_ntt_batch(bn254_ctx *ctx, const bn_g1 *in, bn_g1 *out, int log_n, size_t count, int inverse, const bn_fr *shift);
int bn254_g2_ntt_batch(bn254_ctx *ctx, const bn_g2 *in, bn_g2 *out, int log_n, size_t count, int inverse, const bn_fr *shift);
/* Sparse linear maps over Fr: m dot products in one call - a sparse matrix in CSR form times a vector.  The witness map of an R1CS (the rows
   of A, B, C against the assignment z, in front of the quotient of bn254_fr_ntt_batch), the same transposed for a setup
   (u_i(tau) = sum_j A[j,i] L_j(tau)), and, without an index, segmented inner products: a polynomial against a vector of powers, plain sums
   (coeff = Fr::one()), Lagrange interpolation.  Segments in CSR form exactly as for bn254_g1_msm_batch: offsets[0..m] with offsets[0] == 0,
   non-decreasing, n = offsets[m] terms, and
       out[j] = sum over t in [offsets[j], offsets[j+1]) of coeff[t] * x[index[t]],   j < m
   with x of nx elements and index of n entries, each < nx.  index == NULL means x[t]: a plain segmented inner product, and nx must then equal
   n.  An empty segment gives Fr::zero().  Inputs are canonical Montgomery images; every output is canonical, hence unique, hence independent of
   the order in which the terms are added.  `out` may not overlap any input.  `offsets` is HOST memory.
   How: the host cuts every segment into pieces of at most 4 consecutive terms and a lane runs one piece - two 16-byte loads for coeff[t], two
   for x[index[t]], a Montgomery product and an addition per term -, so no lane's chain depends on the data: one row of 2^22 terms is 2^20
   lanes, not one.  A segment of at most 4 terms writes out[j] directly; a longer one writes partial sums to context-owned scratch, which
   fold levels of at most 16 per lane (additions only) reduce to one value: ceil(log16(ceil(L / 4))) levels for a segment of L terms.  The
   work list (16 bytes per piece: one per segment at least, one per 4 terms) is built on the host and uploaded with the call; levels run as
   sub-launches of at most 2^22 lanes.  Measured on an MI355X (tools/time_dot.py, medians of 5, one process; the full table is
   profiles/r15_dot.txt), kernel time for piece lengths 4 / 8 / 16 / 32: 0.251 / 0.276 / 0.312 / 0.322 ms on an R1CS-like call (786 432 rows of
   1..6 terms, every 1024th of 4096: 5.9 M terms gathered from 2^18 elements), 0.205 / 0.222 / 0.183 / 0.136 ms on ONE segment of 2^22 terms
   without an index, 0.127 / 0.143 / 0.166 / 0.125 ms on 2^10 rows of 2^12 terms.  The rule was fixed before measuring - the fastest on the
   R1CS-like call ships -, so the piece length is 4; on the one long segment it is 51 % behind the best there (32), whose partial sums are an
   eighth as many.  The shipped call takes 1.40 / 2.04 / 1.12 x a device-to-device copy of the bytes it must move and 2.4 / 2.8 / 1.8 x
   bn254_fr_mul_batch_dev on as many pre-gathered terms (which sums nothing).  The fan 16 was not swept.  A variant that accumulates
   unreduced products and reduces once per four terms was not built.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): offsets == NULL with m > 0, offsets[0] != 0, decreasing offsets,
   n > 2^40, a NULL coeff / x (n > 0) or out, index == NULL with nx != n, an index[t] >= nx (the caller gets an error, never a wrong sum).
   m == 0 returns BN254_OK and writes nothing.  Threading: see above - the host-buffer entry point holds the context's mutex for the whole call. */
int bn254_fr_dot_batch(bn254_ctx *ctx, const bn_fr *coeff, const uint64_t *index, const bn_fr *x, size_t nx, const size_t *offsets, size_t m, bn_fr *out);
/* Segmented scans over Fr: the first-order linear recurrence, every segment in one call.  Segments in CSR form exactly as for
   bn254_fr_dot_batch: offsets[0..m] with offsets[0] == 0, non-decreasing, n = offsets[m] terms; `out` has n records, one per term.  For the
   terms t of segment j, in order,
       out[t] = a[t] * prev + b[t],   prev = out[t-1], or init[j] at the segment's first term.
   a == NULL: every a[t] is one - segmented prefix sums, and no product is executed.  b == NULL: every b[t] is zero - segmented prefix
   products.  Both NULL: BN254_E_BAD_ARG.  init == NULL: Fr::zero() when b is given, Fr::one() when it is not; otherwise m records.
   flags:
     BN254_SCAN_REVERSE        the recurrence runs from each segment's last term to its first (prev = out[t+1]): the forward scan of the
                               reversed segment, reversed
     BN254_SCAN_EXCLUSIVE      out[t] = prev, the value BEFORE term t is applied: the first term gets init[j], the segment's total is not written
     BN254_SCAN_A_PER_SEGMENT  a has m records and a[j] multiplies every term of segment j: powers (b == NULL, EXCLUSIVE, init one), Horner's
                               rule and the division by X - z (REVERSE, b the coefficients), many polynomials at many points
   Any other bit: BN254_E_BAD_ARG.  Inputs are canonical Montgomery images; every product and sum is canonical, hence the bytes are those of
   the integer recurrence however the work is cut.  An empty segment writes nothing.  `out` may be exactly `a` or exactly `b` (a term is
   read before its output is written) - except `a` with BN254_SCAN_A_PER_SEGMENT, whose m records are not the n of `out`.  `offsets` is HOST
   memory.
   How: a term is the affine map y -> a y + b, and composing such maps is associative, so no lane's chain depends on the data and no
   workgroup waits for another.  The host cuts every segment into pieces of at most P = 32 consecutive terms.  A segment of at most P terms
   is one lane, one pass, straight to out.  A longer one takes: reduce - a lane per piece composes its terms into the piece's map (A, B), two
   products per term (one without b, none without a); up levels - a lane composes at most F = 16 consecutive maps into one, until at most F
   are left; down levels - a lane takes the value in front of its group (at the top init[j]) and walks its at most F maps, leaving the
   value in front of every child; apply - a lane per piece runs the recurrence from the value in front of it, one product per term.  With
   u = max(0, ceil(log16(ceil(L / 32))) - 1) that is 1 + u + (u + 1) + 1 = 2 u + 3 levels for a segment of L > 32 terms, ordered by the stream;
   every level runs as sub-launches of at most 2^22 lanes.  The work list (24 bytes per piece) is built on the host and uploaded with the
   call; maps and carries (96 bytes per piece and per group) are context-owned scratch.  Timings: profiles/r16_scan.txt (tools/time_scan.py).
   Errors (BN254_E_BAD_ARG, checked before any device is touched): a and b both NULL, an unknown flag, offsets == NULL, offsets[0] != 0,
   decreasing offsets, n > 2^40, a NULL out.  m == 0 returns BN254_OK before anything is looked at, n == 0 after these checks; neither touches a
   device.  Threading: see above - the host-buffer entry point holds the context's mutex for the whole call. */
#define BN254_SCAN_REVERSE 1
#define BN254_SCAN_EXCLUSIVE 2
#define BN254_SCAN_A_PER_SEGMENT 4
int bn254_fr_scan_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *b, const bn_fr *init, const size_t *offsets, size_t m, unsigned int flags, bn_fr *out);
/* Multilinear tables and sumcheck rounds over Fr: what Spartan, HyperPlonk, GKR and lookup arguments need of a prover.  A multilinear table of
   nv variables is 2^nv records; the record at index i is the value at the point of the hypercube whose variable j is bit j of i.  Several
   tables of one sumcheck are stored index-major: tables[i * k + j] is table j at index i (in numpy an (n, k, 4) array), so that ONE fold of
   len = n k records folds all k tables in place and a lane of the round kernel finds its k operands in one contiguous run.  Sumcheck round
   s (from 0) binds variable nv - 1 - s, so the evaluation point has point[j] = challenge[nv - 1 - j].  Inputs are canonical Montgomery
   images; every product and sum is canonical, hence the bytes are those of the integer model however the work is cut.
   bn254_fr_mle_eq: out[i] = prod_{j < nv} (bit j of i ? z[j] : 1 - z[j]) for i < 2^nv, the table of eq(z, .); nv == 0 writes Fr::one().  One lane
   per element and nv products per lane whatever the data: no chain depends on it.
   bn254_fr_mle_fold: out[i] = in[i] + r * (in[i + len/2] - in[i]) for i < len/2 - the MOST significant variable is bound to r.  `r` is ONE element
   in HOST memory.  `out` may be exactly `in` (lane i alone reads its two records and writes record i); the upper half is then left as it
   was.  len == 0 returns BN254_OK and writes nothing; an odd len is BN254_E_BAD_ARG.
   bn254_fr_sumcheck_round: with h = n / 2 and g groups in CSR form over group_tables (group_offsets[0] == 0, increasing; group c holds the 1 to
   `degree` table numbers group_tables[group_offsets[c] .. group_offsets[c+1]), each < k; a table may repeat within a group), for t = 0 .. degree
       out[t] = sum_{i < h} sum_{c < g} group_coeff[c] * prod_{j in group c} (T_j[i] + t * (T_j[i + h] - T_j[i])),   T_j[i] = tables[i k + j].
   `out` has degree + 1 records; out[0] + out[1] is the sum over all n indices.  n need not be a power of two.  The group description
   (group_offsets, group_tables, group_coeff) is HOST memory.
   How: the round kernel has ceil(h / 16) lanes; lane l sums the at most P = 16 indices l, l + lanes, .. into degree + 1 accumulators that stay in
   registers (the kernel is compiled once per degree).  Per group and index it walks the factors one at a time: v = T_j[i], d = T_j[i + h] - T_j[i],
   and per t a product by v and v += d - the values at t = 0, 1, .. cost additions only, and no product or interpolated table is ever written
   to memory.  The coefficient is multiplied into the first factor's v and d.  A call of h <= P writes out directly; otherwise the lanes write
   partial sums, laid out [t][lane], to context-owned scratch and sum levels of at most F = 16 per lane (additions only) reduce them:
   ceil(log16(ceil(h / 16))) levels, ordered by the stream, every level as sub-launches of at most 2^22 lanes.  No atomics, no workgroup waits
   for another, no LDS.  Measured on an MI355X (tools/time_mle.py, kernel ms, medians of 5; profiles/r17_mle.txt): four tables of 2^22 entries at
   degree 3 take 0.668 / 0.629 / 0.612 / 0.770 ms at P = 4 / 8 / 16 / 32 - the fastest ships, by a rule fixed before measuring -, which is 1.04 x
   bn254_fr_mul_batch_dev on the 16 products per index the round executes and 2.6 x faster than the same round from existing calls.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): eq - nv outside 0 .. BN254_MLE_VARS_MAX, a NULL out, a NULL z with nv > 0;
   fold - an odd len, len > 2^40, a NULL in, r or out; round - n odd or below 2, k outside 1 .. BN254_SUMCHECK_TABLES_MAX, g outside
   1 .. BN254_SUMCHECK_GROUPS_MAX, degree outside 1 .. BN254_SUMCHECK_DEGREE_MAX, an empty group or one longer than degree, a table number >= k,
   group_offsets[0] != 0, a NULL pointer, n k > 2^40.  Threading: see above - the host-buffer entry points hold the context's mutex for the
   whole call. */
#define BN254_MLE_VARS_MAX 30
#define BN254_SUMCHECK_DEGREE_MAX 4
#define BN254_SUMCHECK_TABLES_MAX 16
#define BN254_SUMCHECK_GROUPS_MAX 16
int bn254_fr_mle_eq(bn254_ctx *ctx, const bn_fr *z, int nv, bn_fr *out);
int bn254_fr_mle_fold(bn254_ctx *ctx, const bn_fr *in, size_t len, const bn_fr *r, bn_fr *out);
int bn254_fr_sumcheck_round(bn254_ctx *ctx, const bn_fr *tables, size_t n, size_t k, const size_t *group_offsets, const uint64_t *group_tables, const bn_fr *group_coeff, size_t g,
                            int degree, bn_fr *out);
/* The fold of one sumcheck round and the round polynomial of the next in ONE pass over the tables: what a prover does between two challenges.
   Conventions are those of the multilinear calls above (index-major tables[i * k + j], the MOST significant variable bound first, groups in
   CSR form in HOST memory, `r` ONE element in HOST memory).  For n a multiple of 4,
       folded  receives the n / 2 * k records bn254_fr_mle_fold(tables, n k, r) writes: folded[i k + j] = T_j[i] + r * (T_j[i + n/2] - T_j[i]),
       out     receives the degree + 1 records bn254_fr_sumcheck_round(folded, n / 2, k, groups .., degree) writes.
   Everything is canonical, so the bytes ARE those of the two calls and of the integer model however the work is cut.  Every one of the k tables
   is folded, also one that no group names.  `folded` may be exactly `tables`, in both forms: rows [n/2, n) are then left as they were.  Any
   other overlap of `folded` with `tables`, and `out` overlapping either, is BN254_E_BAD_ARG.
   How: the round's mapping over the h2 = n / 4 indices of the round that follows the fold - ceil(h2 / P) lanes, lane l takes the indices l,
   l + lanes, .. .  For index i a lane first walks the k tables: it loads the four records of rows i, i + h2, i + 2 h2, i + 3 h2 and stores
   a0 + r (a2 - a0) to row i and a1 + r (a3 - a1) to row i + h2 of `folded` - two products per table, the fold's own; then it runs the
   round's group walk over rows i and i + h2 of `folded`, reading back what it has just written itself.  Rows i and i + h2 belong to that lane
   alone, which is why in place is safe and no lane waits for another.  One launch reads n k records and writes n k / 2 where the two calls
   move 2 n k.  Partial sums and sum levels are the round's own (context-owned scratch, fan 16, sub-launches of at most 2^22 lanes).  No LDS,
   no atomics.  Indices per lane: P = 8 at full size (the fastest of 4 / 8 / 16 on four tables of 2^22 entries at degree 3, a rule fixed before
   measuring), halved down to 4 while ceil(h2 / P) is below compute units * 4 * 64 * 2 lanes - the lanes that give every SIMD the two waves
   these kernels hold -, because a prover walks through every size.
   Measured on an MI355X (tools/time_fold_round.py, kernel ms, medians of 5; profiles/r20_fold_round.txt): four tables of 2^22 entries at
   degree 3 take 0.605 / 0.595 / 0.671 ms at P = 4 / 8 / 16 - the fastest ships -, which is 3.60 x a device-to-device copy of the 1.5 n k records the
   call must move and 1.31 x bn254_fr_mul_batch_dev on the 24 products per index it executes: the product floor is the nearer one.  At that
   size the fusion itself does not pay: bn254_fr_mle_fold_dev in place and bn254_fr_sumcheck_round_dev take 0.545 ms together (0.92 x, ranges
   apart; one table of 2^24 at degree 1: 0.346 against 0.333 ms).  At 2^16 / 2^18 / 2^20 entries, where the piece has shrunk to 4, the call takes
   0.175 / 0.188 / 0.213 ms against 0.393 / 0.406 / 0.433 ms of the two calls (2.24 / 2.16 / 2.03 x) and against 0.312 / 0.324 / 0.330 ms at the fixed
   P = 8, and the kernel time of a whole proof of 20 variables falls from 7.00 to 3.49 ms (2.01 x).  188 / 242 / 238 / 254 registers at degree
   1 / 2 / 3 / 4, no spill, two waves per SIMD.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): n not a multiple of 4 or below 4, a NULL r or folded, everything
   bn254_fr_sumcheck_round rejects for (n / 2, k, groups, degree), n k > 2^40, the overlaps above.  Threading: as bn254_fr_sumcheck_round - the
   host-buffer entry point holds the context's mutex for the whole call. */
int bn254_fr_sumcheck_fold_round(bn254_ctx *ctx, const bn_fr *tables, size_t n, size_t k, const bn_fr *r, const size_t *group_offsets, const uint64_t *group_tables,
                                 const bn_fr *group_coeff, size_t g, int degree, bn_fr *folded, bn_fr *out);
/* The quotients of a multilinear opening: the prover's field work of a multilinear KZG (PST) commitment.  Conventions are those of the
   multilinear calls above: index i is the point whose variable j is bit j of i, the MOST significant variable is bound first, everything is
   canonical, so the bytes are those of the integer model however the work is cut.  For a table `a` of n = 2^nv records and a point z[0 .. nv),
   start with t = a; for j = nv - 1 down to 0, with half = 2^j,
       q_j[i] = t[i + half] - t[i]   and   t[i] = t[i] + z[j] * q_j[i]   for i < half,
   so that f(x) - f(z) = sum_j (x_j - z_j) q_j(x_0 .. x_{j-1}) for the multilinear f with the values a.  `out` has n records in heap order:
   out[0] = f(z), the one record left, and out[2^j + i] = q_j[i] for j < nv, i < 2^j - the layout in which segment [2^j, 2^(j+1)) meets level j of a
   reference string without a copy.  nv == 0 copies the record to out[0].  `z` is HOST memory.  `a` is never written; `out` must NOT overlap `a`
   (aliasing is not supported: a pass still reads `a` while quotients are written).
   How: one launch does rho = 2 levels in registers.  A pass over a table of L records has L / 2^rho lanes; lane i loads the 2^rho records
   i + c L / 2^rho - all before it writes anything -, does rho levels on them, stores its 2^rho - 1 quotient records to their heap positions and its
   one folded record to position i of the working table; neighbouring lanes touch neighbouring records at every load and store.  So rho levels
   cost one read and one write of the level's bytes.  A call is ceil(nv / rho) launches ordered by the stream: the full passes first, the
   remainder of nv mod rho levels last, on the small table; the first pass reads `a` and writes the working table to context-owned scratch
   (2^(nv - rho) records: a quarter of the table), the later ones run in place there; every pass is cut into sub-launches of at most 2^22 lanes.  No LDS, no atomics,
   no workgroup waits on another, and a lane's serial chain is a constant of the plan.  Measured on an MI355X (tools/time_mle_open.py, kernel ms,
   medians of 5; profiles/r19_mle_open.txt): one table of 2^22 records takes 0.224 / 0.158 / 0.177 / 0.233 ms at rho = 1 / 2 / 3 / 4 (52 / 86 / 150 / 265
   registers, none spills) - the fastest ships, by a rule fixed before measuring -, which is 3.97 x a device-to-device copy of the 2 n records
   the call must move and 2.51 x faster than the same quotients from bn254_fr_add_batch_dev and bn254_fr_mle_fold_dev (2 nv launches).
   Errors (BN254_E_BAD_ARG, checked before any device is touched): nv outside 0 .. BN254_MLE_VARS_MAX, a NULL a or out, a NULL z with nv > 0,
   out overlapping a.  Threading: see above - the host-buffer entry point holds the context's mutex for the whole call. */
int bn254_fr_mle_quotients(bn254_ctx *ctx, const bn_fr *a, int nv, const bn_fr *z, bn_fr *out);
/* Poseidon hashes and Merkle trees over Fr: the hash that lives in the field - Semaphore / Tornado style membership trees, circom's
   poseidon.circom, iden3 sparse trees, witness generation for a circuit that hashes, in-circuit Fiat-Shamir.  The instance is circomlib's:
   S-box x^5, state width t = arity + 1 for arity 1 .. 4, R_F = 8 full rounds (four in front, four behind) around R_P = 56 / 57 / 56 / 60 partial rounds
   for t = 2 / 3 / 4 / 5; round constants and the Cauchy matrix from the Grain LFSR of the Poseidon paper (bn_amd/poseidon.py derives them,
   bn_amd/csrc/poseidon_constants.hpp is generated from it; hash(1, 2) = 7853200120776062878684798364095072458815029376092732009249414926327459813530).  One round: s[i] += C[round * t + i]; s[i] = s[i]^5 for every i (full round) or for i = 0 only (partial round);
   new[i] = sum_j M[i][j] * s[j].  hash(x_1 .. x_arity) = permute([0, x_1, .., x_arity])[0].  Inputs are canonical Montgomery images; outputs are
   canonical, hence the bytes are those of the integer model.
   bn254_fr_poseidon_batch: `in` holds n * arity records, row-major; out[i] = hash(in[i * arity], .., in[i * arity + arity - 1]).  `out` must not overlap `in`.
   bn254_fr_poseidon_permute_batch: n states of t records each, t = 2 .. 5; out[i * t .. i * t + t) = permute(in[i * t .. i * t + t)).  `out` may be
   exactly `in` (a lane reads its t records before it writes them); any other overlap is undefined.
   bn254_fr_merkle_tree: with n = 2^log_n leaves, `nodes` receives the n - 1 inner nodes level by level: first the n / 2 parents of the leaves, then
   the n / 4 parents of those, and so on until the root, nodes[n - 2].  Parent i of a level is hash(child[2 i], child[2 i + 1]) (t = 3).
   log_n == 0 writes nothing (the leaf is the root).  `nodes` must not overlap `leaves`.
   How: one lane per permutation, one kernel instance per width; the state stays in registers, the loop over the rounds is not unrolled and
   the constants are addressed by the round counter alone.  The plain schedule (t^2 products per partial round) is what runs.  A tree is one
   launch per level in stream order, every launch cut into sub-launches of at most 2^22 lanes; no workgroup waits for another, no atomics, no
   LDS, no scratch.  The top levels of a tree are single lanes running a chain of about 830 dependent products each.
   Measured on an MI355X (tools/time_poseidon.py, kernel ms, medians of 5; profiles/r18_poseidon.txt): 2^20 hashes of arity 1 / 2 / 3 / 4 take
   4.7968 / 7.1311 / 10.1963 / 15.2952 ms, 0.46 x bn254_fr_mul_batch_dev on the 828 products of the plain schedule at arity 2; ONE hash of arity 2 takes
   0.7967 ms; a tree of 2^20 leaves 20.1076 ms, of which the seven levels of at most 64 hashes take 5.4096 ms.  A matrix row is one product-sum with a
   single reduction (fr.hpp fr_dot) - by a rule fixed before measuring, 7.1201 against 9.5540 ms on 2^20 hashes of arity 2.
   n == 0 returns BN254_OK and writes nothing.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): arity outside 1 .. BN254_POSEIDON_ARITY_MAX; t outside 2 .. 5; log_n outside
   0 .. BN254_MERKLE_LOG_MAX; a NULL pointer with work to do; n * t > 2^40.  Threading: see above - the host-buffer entry points hold the context's
   mutex for the whole call. */
#define BN254_POSEIDON_ARITY_MAX 4
#define BN254_MERKLE_LOG_MAX 24
int bn254_fr_poseidon_batch(bn254_ctx *ctx, const bn_fr *in, int arity, bn_fr *out, size_t n);
int bn254_fr_poseidon_permute_batch(bn254_ctx *ctx, const bn_fr *in, int t, bn_fr *out, size_t n);
int bn254_fr_merkle_tree(bn254_ctx *ctx, const bn_fr *leaves, int log_n, bn_fr *nodes);
/* Wide Poseidon over Fr: the same circomlib instance at every width circomlib's poseidon.circom and circomlibjs define, 1 .. 16 inputs, t = 2 .. 17
   - what iden3 claims, wide record leaves and circuit witness generators call.  R_F = 8; R_P for t = 2 .. 17 is 56, 57, 56, 60, 60, 63, 64, 63, 60, 66,
   60, 65, 70, 60, 64, 68; round constants and the Cauchy matrix from the Grain LFSR exactly as above (bn_amd/csrc/poseidon_wide_table.hpp restates the
   derivation of bn_amd/poseidon.py on the host: the 12 638 constants are derived per width at its first use, not shipped).  Known answers,
   permute([0, 1, .., n])[0]: n = 6 gives 20400040500897583745843009878988256314335038853985262692600694741116813247201 and n = 16 gives
   9989051620750914585850546081941653841776809718687451684622678807385399211877 - the values circomlibjs publishes in its own tests, the external anchor
   of the R_P list and the wide matrix; n = 1 and n = 2 are the answers pinned above; the rows for every other n in tests/poseidon_wide_cases.py are
   this project's own output, regression anchors and not external vectors.  Inputs are canonical Montgomery images; outputs are canonical, hence
   the bytes are those of the integer model.
   bn254_fr_poseidon_ex_batch: circomlib's PoseidonEx(n_inputs, n_outs).  `in` holds n * n_inputs records, row-major; the state of row i is
   [init ? init[i] : 0, in[i * n_inputs], .., in[i * n_inputs + n_inputs - 1]] (t = n_inputs + 1; `init` may be NULL), and out[i * n_outs + j] =
   permute(state)[j] for j < n_outs, 1 <= n_outs <= t.  With init NULL and n_outs 1 this is bn254_fr_poseidon_batch where that is defined.  `out`
   must not overlap `in` or `init`.
   bn254_fr_poseidon_chain_batch: m variable-length records as CSR `offsets` (m + 1 entries, offsets[0] == 0, non-decreasing, HOST memory as for
   bn254_fr_dot_batch); record j is in[offsets[j] .. offsets[j + 1]).  For a record of L elements: c = Fr(L); the record is cut into
   max(1, ceil(L / rate)) blocks of `rate` elements, the last padded with zeros (an empty record is one block of zeros); for each block in order
   c = permute([c, block..])[0] at width rate + 1; out[j] = c.  That is PoseidonEx(rate, 1) chained through its initialState, the way circom code
   hashes long inputs, with the length in the first capacity element.  THIS FRAMING IS THIS PROJECT'S OWN DEFINITION: it is not an additive sponge
   and it is not a format of any other library.  rate = 1 .. 16.  `out` must not overlap `in`.
   How: BN254_POSEIDON_WIDE_LANES lanes (shipped: see below; 4 / 8 / 16 build) share one permutation and never straddle a wave.  Lane g owns the state
   elements g, g + G, ..; the state lives in LDS; a round is add + S-box + publish on the owned elements, then the lane's rows of M s, each row
   ceil(t / 5) product-sums of at most five pairs (fr.hpp fr_dot) joined by additions - every partial result canonical, so the bytes depend neither
   on G nor on the cut.  t is a run-time argument: one kernel per call kind, not per width.  Constants and matrix rows are vector loads from
   the width's device table (a matrix is at most 9 KB and stays in cache; an LDS copy would need a workgroup barrier and the LDS of more
   resident waves).  The phases are ordered with wave-scope means only - no workgroup barrier, no workgroup waits for another, no atomics, no
   scratch: the groups of a wave run different numbers of blocks in the chain call and leave when their record ends.  Sub-launches of at most
   2^22 lanes.
   Measured on an MI355X (tools/time_poseidon_wide.py, kernel ms, medians of 5; profiles/r27_poseidon_wide.txt): the lanes per
   permutation were chosen by a rule fixed before measuring - the smallest median of five interleaved runs of bn254_fr_poseidon_ex_batch_dev on 2^16
   rows of 16 inputs, equal bytes asserted: 4 / 8 / 16 lanes take 16.5068 / 15.4797 / 20.4012 ms, so 8 ship.  2^20 rows of 2 / 4 / 8 / 16 inputs take
   29.4410 / 35.9782 / 88.5153 / 231.2080 ms - 1.84 / 0.93 / 0.75 / 0.53 x bn254_fr_mul_batch_dev on as many products, and 4.11 / 2.37 x
   bn254_fr_poseidon_batch_dev at 2 / 4 inputs (one lane per hash); ONE row takes 0.4445 / 0.5298 / 1.2953 / 3.4050 ms (one lane: 0.8449 / 1.7638 ms at 2 / 4
   inputs).  The chain on 2^16 records of 1 .. 40 elements at rate 16 takes 37.7600 ms.  132 / 140 VGPRs, no spill, 17 408 B of LDS per workgroup.  The
   small calls and the top of a tree are NOT rerouted onto these kernels.
   n == 0 and m == 0 return BN254_OK and write nothing.
   Errors (BN254_E_BAD_ARG, checked before any device is touched): n_inputs or rate outside 1 .. BN254_POSEIDON_EX_INPUTS_MAX; n_outs outside
   1 .. n_inputs + 1; a NULL pointer with work to do (`init` may be NULL); offsets[0] != 0 or offsets decreasing; n * t or the number of elements
   above 2^40; `out` overlapping an input (host-buffer forms).  Threading: see above - the host-buffer entry points hold the context's mutex for
   the whole call. */
#define BN254_POSEIDON_EX_INPUTS_MAX 16
int bn254_fr_poseidon_ex_batch(bn254_ctx *ctx, const bn_fr *in, int n_inputs, const bn_fr *init, int n_outs, bn_fr *out, size_t n);
int bn254_fr_poseidon_chain_batch(bn254_ctx *ctx, const bn_fr *in, const size_t *offsets, size_t m, int rate, bn_fr *out);

/* ---- one node, several GPUs (north_star: independent batches shard across the GPUs; ONE exchange for the multi-pairing) --- */
/* `devices[0..ndev)`: HIP device index of every rank (NULL = 0..ndev-1).  One context and one host thread per rank.  A device may
   be listed more than once (several ranks on one GPU - how the N > 1 path is exercised on a one-GPU box); the exchange of the
   product is an RCCL all-gather when all devices are distinct and RCCL loads, peer copies otherwise (bn254_multi_create_ex
   forces one). */
typedef struct bn254_multi bn254_multi;
enum { BN254_EXCHANGE_AUTO = -1, BN254_EXCHANGE_PEER = 0, BN254_EXCHANGE_RCCL = 1 };
int bn254_multi_create(const int *devices, int ndev, bn254_multi **out);                       /* = _ex(..., BN254_EXCHANGE_AUTO, ...) */
/* exchange: BN254_EXCHANGE_AUTO (RCCL when every rank has its own GPU and RCCL loads, else peer copies), _PEER (never load RCCL),
   _RCCL (fail with BN254_E_COMM instead of falling back) */
int bn254_multi_create_ex(const int *devices, int ndev, int exchange, bn254_multi **out);
/* bn254_ctx_set_option on every rank's context */
int bn254_multi_set_option(bn254_multi *m, int key, long value);
void bn254_multi_destroy(bn254_multi *m);
int bn254_multi_device_count(const bn254_multi *m);
int bn254_multi_exchange_kind(const bn254_multi *m);                 /* BN254_EXCHANGE_* */
/* The host thread that drives a rank (its pageable H2D / D2H copies and launches) is pinned, for the duration of a call, to the CPUs
   of that GPU's NUMA node when the node is known (/sys/bus/pci/devices/<bus id>/numa_node) and the process may run there; the
   caller's own thread is never re-pinned (every rank runs on a worker thread of the call).  Returns that node, or -1 when the rank's thread is not pinned. */
int bn254_multi_rank_numa_node(const bn254_multi *m, int rank);
bn254_ctx *bn254_multi_ctx(bn254_multi *m, int rank);                /* rank's context (owned by m) */
/* out[i] = pairing(p[i], q[i]); rank g owns the contiguous shard [n*g/G, n*(g+1)/G); no exchange (BASELINE configs[2]) */
int bn254_pairing_batch_multi(bn254_multi *m, const bn_g1 *p, const bn_g2 *q, bn_gt *out, size_t n);
/* fold(Gt::one(), acc * pairing(p, q)) over all n pairs (shootout/main.rs:11-16): every rank reduces its shard to one
   un-exponentiated Fq12, ONE all-gather of 384 bytes per rank, world-1 products and a single final exponentiation on rank 0
   (BASELINE configs[3]).  Bit-identical to the fold: the final exponentiation is a homomorphism and Gt values are canonical. */
int bn254_pairing_product_multi(bn254_multi *m, const bn_g1 *p, const bn_g2 *q, size_t n, bn_gt *out);
/* bn254_pairing_product_batch over the ranks: segment j runs on the rank whose pair shard [n*g/G, n*(g+1)/G) holds offsets[j]
   (offsets[j] == n: the last rank), with all of its pairs.  No exchange. */
int bn254_pairing_product_batch_multi(bn254_multi *mh, const bn_g1 *p, const bn_g2 *q, const size_t *offsets, size_t m, bn_gt *out);
/* bn254_g{1,2}_msm_batch over the ranks by the same rule: segment j runs on the rank whose TERM shard [n*g/G, n*(g+1)/G) holds offsets[j]
   (offsets[j] == n: the last rank), with all of its terms.  No exchange. */
int bn254_g1_msm_batch_multi(bn254_multi *mh, const bn_g1 *p, const bn_fr *k, const size_t *offsets, size_t m, bn_g1 *out);
int bn254_g2_msm_batch_multi(bn254_multi *mh, const bn_g2 *p, const bn_fr *k, const size_t *offsets, size_t m, bn_g2 *out);
/* bn254_g{1,2}_msm over the ranks: rank g sums its term shard [n*g/G, n*(g+1)/G) (normalised; an empty shard gives zero), then rank 0 adds
   the G partial sums as one bn254_g{1,2}_msm_batch segment with scalars one.  No device-to-device exchange; same bytes as one device. */
int bn254_g1_msm_multi(bn254_multi *mh, const bn_g1 *p, const bn_fr *k, size_t n, bn_g1 *out);
int bn254_g2_msm_multi(bn254_multi *mh, const bn_g2 *p, const bn_fr *k, size_t n, bn_g2 *out);

/* native prepared-G2 mode over the GPUs of the handle.  ONE point (nq == 1) is prepared on every rank's GPU and n pairings shard like
   bn254_pairing_batch_multi; nq > 1 points are sharded by the same rule ([nq*g/G, nq*(g+1)/G) on rank g) and then pair with exactly n == nq
   points p[i] (point i with p[i]), so that tables and inputs of a shard live on the same GPU.  No exchange. */
typedef struct bn254_multi_prepared bn254_multi_prepared;
int bn254_g2_prepare_multi(bn254_multi *m, const bn_g2 *q, size_t nq, bn254_multi_prepared **out);
void bn254_multi_prepared_destroy(bn254_multi_prepared *prep);
size_t bn254_multi_prepared_count(const bn254_multi_prepared *prep);
int bn254_pairing_prepared_native_batch_multi(bn254_multi *m, const bn_g1 *p, const bn254_multi_prepared *prep, bn_gt *out, size_t n);
/* bn254_pairing_product_multi over prepared points (bn254_pairing_product_prepared_native sharded): every rank folds its shard over its own tables,
   then the ONE 384-byte exchange and the single final exponentiation on rank 0.  n == count for a sharded set, any n against one point. */
int bn254_pairing_product_prepared_native_multi(bn254_multi *m, const bn_g1 *p, const bn254_multi_prepared *prep, size_t n, bn_gt *out);

/* wire format of the crate's Encodable/Decodable impls for G1/G2 (groups/mod.rs:143-205, fields/fp.rs:24-36, fields/fq2.rs:31-53,
   arith.rs:100-159), as fixed-size batch records: [tag][x][y] with tag 4 and big-endian canonical coordinates (Fq2 = the 512-bit
   integer c1*q + c0); infinity is tag 0 followed by zero padding (the crate's stream emits the lone byte 0).  Decoding validates
   what the crate validates, in its order, and reports per record: 0 ok, 1 "integer is not less than modulus", 2 "integer not
   less than modulus squared", 3 "invalid leading byte", 4 "point is not on the curve", 5 "point is not in the subgroup" (G2
   only).  A rejected record decodes to G::zero(). */
#define BN254_FR_WIRE_BYTES 32    /* Fr: big-endian canonical integer (fields/fp.rs:24-36); decode status 0 or 1, rejected -> Fr::zero() */
#define BN254_G1_WIRE_BYTES 65
#define BN254_G2_WIRE_BYTES 129
int bn254_fr_encode_batch(bn254_ctx *ctx, const bn_fr *k, uint8_t *out, size_t n);
int bn254_fr_decode_batch(bn254_ctx *ctx, const uint8_t *in, bn_fr *out, int32_t *status, size_t n);
int bn254_g1_encode_batch(bn254_ctx *ctx, const bn_g1 *p, uint8_t *out, size_t n);
int bn254_g2_encode_batch(bn254_ctx *ctx, const bn_g2 *p, uint8_t *out, size_t n);
int bn254_g1_decode_batch(bn254_ctx *ctx, const uint8_t *in, bn_g1 *out, int32_t *status, size_t n);
int bn254_g2_decode_batch(bn254_ctx *ctx, const uint8_t *in, bn_g2 *out, int32_t *status, size_t n);
/* the crate's own byte stream (what bincode/rustc_serialize produce for a sequence of points, groups/mod.rs:143-205): a point at
   infinity is the lone byte 0, a finite point is 4 + coordinates, so records have variable length.  encode: `written` bytes are
   produced (BN254_E_BAD_ARG if `cap` is too small: `*written` is left as it was, `out` holds the leading whole records that fit in
   `cap` and nothing behind them is written; `cap` equal to the length of the stream is enough).  decode: up to `max_points` points are parsed from `len` bytes; `count` points
   and `consumed` bytes are reported (a truncated trailing record is left unconsumed); status[i] as for the batch decoders.
   DIFFERENCE from the crate: its Decodable returns Err at the first bad record and the caller's stream stops there
   (groups/mod.rs:165-175); this decoder records the status (a bad tag consumes its one byte, a record that fails a check consumes
   its full length), decodes the record to G::zero() and CONTINUES with the next one.  bn254_ctx_set_option(ctx,
   BN254_OPT_STREAM_STOP_AT_ERROR, 1) selects the crate's behaviour: the call stops with the first bad record (count includes it). */
int bn254_g1_encode_stream(bn254_ctx *ctx, const bn_g1 *p, size_t n, uint8_t *out, size_t cap, size_t *written);
int bn254_g2_encode_stream(bn254_ctx *ctx, const bn_g2 *p, size_t n, uint8_t *out, size_t cap, size_t *written);
int bn254_g1_decode_stream(bn254_ctx *ctx, const uint8_t *in, size_t len, bn_g1 *out, int32_t *status, size_t max_points, size_t *count, size_t *consumed);
int bn254_g2_decode_stream(bn254_ctx *ctx, const uint8_t *in, size_t len, bn_g2 *out, int32_t *status, size_t max_points, size_t *count, size_t *consumed);

/* Compressed encodings: x and one sign bit, 32 bytes for G1 and 64 for G2, one record per lane.  Two byte layouts, laid out as ark-serialize /
   gnark-crypto describe; not checked against those libraries here.
     BN254_COMPRESSED_ARK    little-endian integers; G2 is x.c0 then x.c1; the top two bits of the LAST byte are flags: bit 7 = sign(y),
                             bit 6 = infinity (that one flag and zeros everywhere else); both set is invalid
     BN254_COMPRESSED_GNARK  big-endian integers; G2 is x.c1 then x.c0; the top two bits of the FIRST byte: 10 = sign(y) 0, 11 = sign(y) 1,
                             01 = infinity (all other bits zero), 00 = invalid
   sign(y) = 1 iff y > -y as canonical integers; in Fq2 c1 is compared first and c0 only when c1 == 0.
   compress takes any Jacobian point, normalises as bn254_g{1,2}_encode_batch does and writes canonical bytes.  decompress recovers y with one
   (G1) or two (G2) fixed exponentiations by (q - 3) / 4 - the same chain in every lane - and reports status[i] with the numbers of the wire
   format above, checked in this order: 3 = invalid flags or an infinity record with other bits set, 1 = a coordinate component is not below q,
   4 = x^3 + b is not a square, 5 = not in the subgroup (G2 only), 0 = ok.  A rejected record decodes to G::zero(); an accepted one to the bytes
   bn254_g{1,2}_decode_batch gives for the uncompressed record of the same point, so decompress(compress(p)) == decode(encode(p)) and
   compress(decompress(b)) == b for every accepted b.  An unknown format, a NULL pointer with n > 0 or n above the wire format's limit
   (0x7fffffff / 129 records) is BN254_E_BAD_ARG before any device is touched; n == 0 succeeds.  The _dev forms take device pointers (d_status
   too) and enqueue on `stream`: compressed proofs go up once and can feed bn254_pairing_product_batch_dev without coming back. */
#define BN254_COMPRESSED_ARK 0
#define BN254_COMPRESSED_GNARK 1
#define BN254_G1_COMPRESSED_BYTES 32
#define BN254_G2_COMPRESSED_BYTES 64
int bn254_g1_compress_batch(bn254_ctx *ctx, const bn_g1 *p, int format, uint8_t *out, size_t n);
int bn254_g2_compress_batch(bn254_ctx *ctx, const bn_g2 *p, int format, uint8_t *out, size_t n);
int bn254_g1_decompress_batch(bn254_ctx *ctx, const uint8_t *in, int format, bn_g1 *out, int32_t *status, size_t n);
int bn254_g2_decompress_batch(bn254_ctx *ctx, const uint8_t *in, int format, bn_g2 *out, int32_t *status, size_t n);
int bn254_g1_compress_batch_dev(bn254_ctx *ctx, const void *d_p, int format, void *d_out, size_t n, void *stream);
int bn254_g2_compress_batch_dev(bn254_ctx *ctx, const void *d_p, int format, void *d_out, size_t n, void *stream);
int bn254_g1_decompress_batch_dev(bn254_ctx *ctx, const void *d_in, int format, void *d_out, void *d_status, size_t n, void *stream);
int bn254_g2_decompress_batch_dev(bn254_ctx *ctx, const void *d_in, int format, void *d_out, void *d_status, size_t n, void *stream);

/* Hash to G1 (RFC 9380), one record per lane.  The constants below were derived from the RFC's formulas (Z by its find_z_svdw search); they are
   not checked against gnark-crypto or any other library.
     map_to_curve   the Shallue-van de Woestijne map with Z = 1, c1 = g(Z) = 4, c2 = -Z / 2, c3 = sqrt(-g(Z) 3 Z^2) with sgn0(c3) = 0,
                    c4 = -4 g(Z) / (3 Z^2), computed in the RFC's order; sgn0(a) is the canonical integer of a mod 2 (not the y > -y rule of the
                    compressed encodings), inv0(0) = 0, zero counts as a square.  u[i] is 48 big-endian bytes, any value below 2^384, taken
                    mod q.  out[i] = (x, y, 1) in canonical Montgomery words; the map never gives the point at infinity.
     uniform        record i is 96 bytes: u0 = bytes [0, 48), u1 = bytes [48, 96) (hash_to_field with L = 48).  out[i] = map(u0) + map(u1) by the
                    complete addition - equal points double - normalised: (x, y, 1), or G::zero() = (0, 1, 0) when the two maps cancel.
                    The cofactor is 1: nothing is cleared.
     messages       n messages of msg_len bytes each, back to back; record i is hash_to_curve(msg i) with the 96 uniform bytes from
                    expand_message_xmd(msg, dst, 96) over SHA-256, computed on the device.  msg_len == 0 is allowed (msgs may then be NULL).
                    Messages of different lengths go through the uniform call after a host-side expansion.  `dst` is a HOST pointer in both
                    forms (1 .. BN254_H2C_DST_MAX bytes; the RFC's rule for hashing longer tags is not built).
   A NULL pointer with work to do, dst_len == 0 or dst_len > BN254_H2C_DST_MAX, msg_len > 2^20, n > 2^40 or n * msg_len > 2^40 is
   BN254_E_BAD_ARG before any device is touched; n == 0 succeeds.  Calls run as sub-launches of at most 2^22 records.  The _dev forms take
   device pointers (dst excepted) and enqueue on `stream`: the points can feed bn254_g1_mul_batch_dev or bn254_pairing_product_batch_dev without
   coming back.  Threading: see above. */
#define BN254_H2C_FIELD_BYTES 48
#define BN254_H2C_UNIFORM_BYTES 96
#define BN254_H2C_DST_MAX 255
int bn254_g1_map_to_curve_batch(bn254_ctx *ctx, const uint8_t *u, bn_g1 *out, size_t n);
int bn254_g1_hash_to_curve_uniform_batch(bn254_ctx *ctx, const uint8_t *uniform, bn_g1 *out, size_t n);
int bn254_g1_hash_to_curve_batch(bn254_ctx *ctx, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, bn_g1 *out, size_t n);
int bn254_g1_map_to_curve_batch_dev(bn254_ctx *ctx, const void *d_u, void *d_out, size_t n, void *stream);
int bn254_g1_hash_to_curve_uniform_batch_dev(bn254_ctx *ctx, const void *d_uniform, void *d_out, size_t n, void *stream);
int bn254_g1_hash_to_curve_batch_dev(bn254_ctx *ctx, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out, size_t n, void *stream);

/* Hash to G2 (RFC 9380) and cofactor clearing, one record per lane.  The constants were derived from the RFC's formulas (Z by its find_z_svdw
   search over Fq2, which gives Z = 1 as for G1) and the clearing is the one step the RFC defines no suite for: NEITHER THE CONSTANTS NOR THE
   OUTPUTS ARE CHECKED AGAINST gnark-crypto OR ANY OTHER LIBRARY.
     map_to_curve   the Shallue-van de Woestijne map over Fq2 for the twist y^2 = x^3 + b', b' = 3 / (9 + i): Z = 1, c1 = g(Z) = 1 + b', c2 = -1 / 2,
                    c3 = sqrt(-g(Z) 3 Z^2) with sgn0(c3) = 0, c4 = -4 g(Z) / (3 Z^2), in the RFC's order.  sgn0(a) = sign_0 | (zero_0 & sign_1) on the
                    canonical integers of (c0, c1); inv0(0) = 0; is_square is the character of the norm and zero counts as a square.  u[i] is 96
                    bytes: c0 then c1, each 48 big-endian bytes, any value below 2^384, taken mod q.  out[i] = (x, y, 1) in canonical Montgomery
                    words, never the point at infinity.
                    *** THE RESULT IS ON THE TWIST BUT NOT IN G2 ***: the twist has the 254-bit cofactor 2q - r.  Do not hand it to a pairing, to
                    bn254_g2_mul_batch (GLS, valid on the order-r subgroup only) or to an encoder; clear the cofactor first.
     clear_cofactor p[i] is any Jacobian point of the twist - being on the curve is the CALLER's responsibility, Z = 0 counts as infinity.
                    out[i] = clear(P) = [u]P + psi([3u]P) + psi^2([u]P) + psi^3(P), u = 4965661367192848881,
                    psi(X, Y, Z) = (conj(X) gx, conj(Y) gy, conj(Z)) (Fuentes-Castaneda, Knapp, Rodriguez-Henriquez, section 6.1), normalised:
                    (x, y, 1) in G2, or G2::zero() = (0, 1, 0) for infinity.  This is NOT [2q - r]P - the formula is part of the interface; on a point
                    Q of G2 it is [k]Q with k = u + 3u lambda + u lambda^2 + lambda^3 mod r, lambda = 6u^2.  [u]P is plain double-and-add with the
                    complete addition, never the GLS multiplication.  out may be exactly p.
     uniform        record i is 192 bytes: u0.c0 | u0.c1 | u1.c0 | u1.c1 (hash_to_field with L = 48, m = 2).  out[i] = clear(map(u0) + map(u1)),
                    normalised; G2::zero() when the two maps cancel.
     messages       n messages of msg_len bytes each, back to back; record i is hash_to_curve(msg i) with the 192 uniform bytes from
                    expand_message_xmd(msg, dst, 192) over SHA-256, computed on the device.  msg_len == 0 is allowed (msgs may then be NULL).
                    Messages of different lengths go through the uniform call after a host-side expansion.  `dst` is a HOST pointer in both forms
                    (1 .. BN254_H2C_DST_MAX bytes).
   Argument rules and error codes as for G1: a NULL pointer with work to do, dst_len == 0 or dst_len > BN254_H2C_DST_MAX, msg_len > 2^20, n > 2^40
   or n * msg_len > 2^40 is BN254_E_BAD_ARG before any device is touched; n == 0 succeeds.  Calls run as sub-launches of at most 2^22 records.
   The _dev forms take device pointers (dst excepted) and enqueue on `stream`.  Threading: see above. */
#define BN254_H2C_G2_FIELD_BYTES 96
#define BN254_H2C_G2_UNIFORM_BYTES 192
int bn254_g2_map_to_curve_batch(bn254_ctx *ctx, const uint8_t *u, bn_g2 *out, size_t n);
int bn254_g2_clear_cofactor_batch(bn254_ctx *ctx, const bn_g2 *p, bn_g2 *out, size_t n);
int bn254_g2_hash_to_curve_uniform_batch(bn254_ctx *ctx, const uint8_t *uniform, bn_g2 *out, size_t n);
int bn254_g2_hash_to_curve_batch(bn254_ctx *ctx, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, bn_g2 *out, size_t n);
int bn254_g2_map_to_curve_batch_dev(bn254_ctx *ctx, const void *d_u, void *d_out, size_t n, void *stream);
int bn254_g2_clear_cofactor_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_out, size_t n, void *stream);
int bn254_g2_hash_to_curve_uniform_batch_dev(bn254_ctx *ctx, const void *d_uniform, void *d_out, size_t n, void *stream);
int bn254_g2_hash_to_curve_batch_dev(bn254_ctx *ctx, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out, size_t n, void *stream);

/* Validation of raw points, one record per lane: what every other entry point TRUSTS its caller to have done.  p[i] is any 96 / 192 bytes:
   (x, y, z) as canonical Montgomery words, any z.  status[i] takes the numbers of the wire format above, checked in the order of the
   compressed decoders:
     1   a coordinate (G2: a component of one) is not below q - the words are compared as they stand, before any field arithmetic
     0   z == 0: the point at infinity, whatever x and y hold
     4   Y^2 != X^3 + b Z^6 (b = 3 for G1, b' = 3 / (9 + i) for G2): not on the curve
     5   (G2 only) on the twist but not in the order-r subgroup.  The twist has the 254-bit cofactor 2q - r, and a pairing check against a point
         outside the subgroup means nothing.  G1 has cofactor 1: on the curve is in the group.
     0   otherwise: a valid point
   Membership of G2 is the endomorphism subgroup test [u + 1]P + psi([u]P) + psi^2([u]P) == psi^3([2u]P), u = 4965661367192848881,
   psi(X, Y, Z) = (conj(X) gx, conj(Y) gy, conj(Z)) - the criterion gnark-crypto's bn254 uses; exact: it accepts a point of the twist if and only
   if [r]P == 0.  [u]P is plain double-and-add with the complete addition, never the GLS multiplication (bn254_g2_mul_batch by r is WRONG off
   the subgroup, where psi is not the scalar lambda).  The decoders of the wire format and of the compressed encodings run the same test.
   Nothing is written but status; a record is never changed.  A NULL pointer with work to do or n > 2^40 is BN254_E_BAD_ARG before any device
   is touched; n == 0 succeeds.  Calls run as sub-launches of at most 2^22 records.  The _dev forms take device pointers (d_status too: int32_t
   per record) and enqueue on `stream`.  Threading: see above. */
int bn254_g1_validate_batch(bn254_ctx *ctx, const bn_g1 *p, int32_t *status, size_t n);
int bn254_g2_validate_batch(bn254_ctx *ctx, const bn_g2 *p, int32_t *status, size_t n);
int bn254_g1_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream);
int bn254_g2_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream);

/* Baby Jubjub and EdDSA-Poseidon, one record per lane.  Baby Jubjub is the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over Fr - THIS
   library's scalar field - with a = 168700 and d = 168696: the curve circomlib, iden3 and the Hermez-style rollups sign on.  Identity O = (0, 1),
   -(x, y) = (-x, y), order 8 l with l = 2736030358979909402780800718157159386076813972158567259200215660948447373041 (251 bits); the base point
   B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
   16950150798460657717958625567821834550301663161624707787222815936182638968203) has order l.  a is a square mod r and d is not, so the unified
   addition law is complete: no exceptional inputs, doubling is the same formula.  A POINT is two consecutive bn_fr, x then y, canonical
   Montgomery words, affine: p[2 i] and p[2 i + 1].  Scalars and messages are bn_fr like everywhere else; a scalar's value is the canonical
   integer of the element.
   bn254_bjj_validate_batch: status[i] for the raw record p[i], any 64 bytes, checked in this order:
     1   a coordinate is not below r - the words are compared as they stand, before any field arithmetic
     4   a x^2 + y^2 != 1 + d x^2 y^2: not on the curve
     5   on the curve but [l]P != O: a component in the cofactor-8 part
     0   otherwise: a valid point; O is one
   Nothing is written but status; a record is never changed.
   bn254_bjj_add_batch: out[i] = p[i] + q[i], the complete affine sum, defined for points of the curve - like the G1 calls it trusts its caller.
   out may be p or q.
   bn254_bjj_mul_batch: out[i] = [k[i]] p[i] for ANY point of the curve, cofactor components included, and any k in [0, r); affine; out may be p.
   (8 l is above r: [8 l]P is [8]([l]P).)  One fixed-window chain of complete additions over the bits of the integer k, one inversion per lane.
   bn254_eddsa_poseidon_challenge_batch: out[i] = Poseidon5(r8[i].x, r8[i].y, a[i].x, a[i].y, msg[i]) - circomlib's Poseidon at width t = 6
   (R_F = 8, R_P = 60), element 0 of permute([0, ...]); plain field elements in, one bn_fr out, NO curve check.  The hash half of the verifier,
   for signers and witness generators.  The public Poseidon calls above still stop at arity BN254_POSEIDON_ARITY_MAX.
   bn254_eddsa_poseidon_verify_batch: circomlib's verifyPoseidon for the signature (r8[i], s[i]) on msg[i] under the key a[i]; status[i], checked
   in this order, every row on its own:
     1   a word array of a, r8, s or msg is not below r, or the integer of s is not below l
     4   R8 or A is not on the curve
     6   [S]B8 != R8 + [8 hm]A with hm the challenge above.  The scalar is the INTEGER 8 hm, not its value reduced mod l
     0   valid
   There is NO subgroup check, as there is none in circomlib: A = O, or A of small order, with R8 = [S]B8 verifies.  Check keys with
   bn254_bjj_validate_batch where that matters.  One lane hashes, forms [8]A and runs one joint doubling chain for [S]B8 - [hm]([8]A), compared
   with R8 without an inversion.
   All five: a NULL pointer with work to do or n > 2^40 is BN254_E_BAD_ARG before any device is touched; n == 0 succeeds.  Calls run as
   sub-launches of at most 2^22 records.  The _dev forms take device pointers (d_status too: int32_t per record), enqueue on `stream`, use no
   host round trip and read nothing back.  Threading: see above. */
int bn254_bjj_validate_batch(bn254_ctx *ctx, const bn_fr *p, int32_t *status, size_t n);
int bn254_bjj_add_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *q, bn_fr *out, size_t n);
int bn254_bjj_mul_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *k, bn_fr *out, size_t n);
int bn254_eddsa_poseidon_challenge_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *r8, const bn_fr *msg, bn_fr *out, size_t n);
int bn254_eddsa_poseidon_verify_batch(bn254_ctx *ctx, const bn_fr *a, const bn_fr *r8, const bn_fr *s, const bn_fr *msg, int32_t *status, size_t n);
int bn254_bjj_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream);
int bn254_bjj_add_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, void *d_out, size_t n, void *stream);
int bn254_bjj_mul_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, void *d_out, size_t n, void *stream);
int bn254_eddsa_poseidon_challenge_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_r8, const void *d_msg, void *d_out, size_t n, void *stream);
int bn254_eddsa_poseidon_verify_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_r8, const void *d_s, const void *d_msg, void *d_status, size_t n, void *stream);
/* Packed points and signatures, the form keys and signatures travel in (circomlib's packPoint / packSignature).  A packed point is 32 bytes:
   the canonical integer of y, little endian, with bit 7 of byte 31 set iff the canonical integer of x is above (r - 1) / 2.  A packed
   signature is 64 bytes: the packed R8, then the integer S as 32 little-endian bytes (its top bit is no flag).
   bn254_bjj_pack_batch: out32[32 i ..] = the record of p[i].  No validation: words not below r give unspecified bytes, never a fault.
   bn254_bjj_unpack_batch: out[i] and status[i] for the record in32[32 i ..], any 32 bytes, checked in this order:
     1   the integer of y (the sign bit cleared) is not below r
     4   x^2 = (1 - y^2) / (a - d y^2) is not a square: no point has this y
     3   x == 0 and the sign bit is set: a non-canonical encoding of (0, 1) or (0, -1)
     0   otherwise: out[i] is the point with this y whose x has this sign
   A rejected record gives O = (0, 1).  There is NO subgroup check, as there is none in circomlib: bn254_bjj_validate_batch is there for that.
   One square root of a ratio per record and no inversion (bn254_fr_sqrt_batch's).
   bn254_eddsa_poseidon_verify_packed_batch: bn254_eddsa_poseidon_verify_batch on the packed key a32[32 i ..] and the packed signature
   sig64[64 i ..], msg as there; status[i], checked in this order, every row on its own:
     1   a y is not below r, the integer S is not below l, or the words of msg are not below r
     4   a point has no x
     3   a non-canonical sign, in either point
     6   [S]B8 != R8 + [8 hm]A
     0   valid
   One launch: a lane unpacks its two points and runs the hash and the joint chain of the unpacked verifier.
   All three: a NULL pointer with work to do or n > 2^40 is BN254_E_BAD_ARG before any device is touched; n == 0 succeeds; sub-launches of at
   most 2^22 records.  The _dev forms take device pointers (16-byte aligned; d_status int32_t per record), enqueue on `stream`, use no host
   round trip and read nothing back.  Threading: see above. */
int bn254_bjj_pack_batch(bn254_ctx *ctx, const bn_fr *p, uint8_t *out32, size_t n);
int bn254_bjj_unpack_batch(bn254_ctx *ctx, const uint8_t *in32, bn_fr *out, int32_t *status, size_t n);
int bn254_eddsa_poseidon_verify_packed_batch(bn254_ctx *ctx, const uint8_t *a32, const uint8_t *sig64, const bn_fr *msg, int32_t *status, size_t n);
int bn254_bjj_pack_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_out32, size_t n, void *stream);
int bn254_bjj_unpack_batch_dev(bn254_ctx *ctx, const void *d_in32, void *d_out, void *d_status, size_t n, void *stream);
int bn254_eddsa_poseidon_verify_packed_batch_dev(bn254_ctx *ctx, const void *d_a32, const void *d_sig64, const void *d_msg, void *d_status, size_t n, void *stream);

/* Grumpkin, one record per lane.  Grumpkin is the curve y^2 = x^3 - 17 over Fr - THIS library's scalar field - whose order is q, the base field
   modulus of BN254: the two curves form a cycle.  q is prime, so the cofactor is 1 and there is no subgroup to check.  The generator is
   G = (1, 17631683881184975370165255887551781615748388533673675138860), the square root of -16 that is not above (r - 1) / 2.
   A POINT is two consecutive bn_fr, x then y, canonical Montgomery words, affine: p[2 i] and p[2 i + 1], 64 bytes, the layout of the Baby
   Jubjub calls.  Infinity is (0, 0): -17 is a non-residue mod r, so no point of the curve has x = 0.  -(x, y) = (x, -y).
   A SCALAR is 32 bytes, the little-endian integer k: k32[32 i ..].  Any value below 2^256 is accepted and the result is [k]P for that integer,
   which equals [k mod q]P.  It is NOT a Montgomery image and not a bn_fr: the scalar field of this curve is Fq, and this header has no Fq type.
   bn254_grumpkin_validate_batch: status[i] for the raw record p[i], any 64 bytes, checked in this order:
     1   a coordinate is not below r - the words are compared as they stand, before any field arithmetic
     4   y^2 != x^3 - 17 and the record is not (0, 0): not on the curve
     0   otherwise: a point of the curve; O = (0, 0) is one
   Nothing is written but status; a record is never changed.  There is no subgroup status: the cofactor is 1.
   bn254_grumpkin_add_batch: out[i] = p[i] + q[i] by the complete projective formulas of Renes-Costello-Batina for a = 0: no exceptional inputs,
   p[i] == q[i], O and p[i] == -q[i] included.  Defined for points of the curve - like the G1 calls it trusts its caller; an off-curve record gives
   garbage, never a fault.  out may be p or q.
   bn254_grumpkin_mul_batch: out[i] = [k32[i]] p[i]; out may be p.  One fixed-window chain (4 bits a window) of complete additions over all 256
   bits of k, the same instruction stream whatever the scalar, and one inversion per lane.
   bn254_grumpkin_msm_batch: out[j] = sum over t in [offsets[j], offsets[j+1]) of [k32[t]] p[t], affine.  offsets: a HOST array of m + 1 size_t in
   both forms, as for bn254_fr_dot_batch: offsets[0] == 0, never decreasing, offsets[m] terms in all.  An empty segment and a sum that cancels
   give (0, 0).  out must not overlap the inputs.  One lane per term runs the chain; segments of more than one term are then added in fold
   levels of at most 16 partial sums per lane, one inversion per segment.
   All four: a NULL pointer with work to do or n > 2^40 (offsets[m] > 2^40) is BN254_E_BAD_ARG before any device is touched, and so are offsets
   that do not start at 0 or that decrease; n == 0 (m == 0) succeeds.  Calls run as sub-launches of at most 2^22 records.  The _dev forms take
   device pointers (16-byte aligned; d_status int32_t per record), enqueue on `stream`, use no host round trip and read nothing back.
   Threading: see above. */
int bn254_grumpkin_validate_batch(bn254_ctx *ctx, const bn_fr *p, int32_t *status, size_t n);
int bn254_grumpkin_add_batch(bn254_ctx *ctx, const bn_fr *p, const bn_fr *q, bn_fr *out, size_t n);
int bn254_grumpkin_mul_batch(bn254_ctx *ctx, const bn_fr *p, const uint8_t *k32, bn_fr *out, size_t n);
int bn254_grumpkin_msm_batch(bn254_ctx *ctx, const bn_fr *p, const uint8_t *k32, const size_t *offsets, size_t m, bn_fr *out);
int bn254_grumpkin_validate_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_status, size_t n, void *stream);
int bn254_grumpkin_add_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, void *d_out, size_t n, void *stream);
int bn254_grumpkin_mul_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k32, void *d_out, size_t n, void *stream);
int bn254_grumpkin_msm_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k32, const size_t *offsets, size_t m, void *d_out, void *stream);

/* ---- device-resident entry points (inputs/outputs already in HBM; `stream` is a hipStream_t or NULL) ------------------ */
/* Same layouts (array of structs) in device memory.  Asynchronous on `stream`; the caller synchronises. */
int bn254_pairing_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, void *d_out, size_t n, void *stream);
/* the two halves of a pairing, for the multi-pairing product: Miller loop only (infinity -> one), then final exponentiation */
int bn254_miller_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, void *d_f, size_t n, void *stream);
int bn254_final_exp_batch_dev(bn254_ctx *ctx, const void *d_f, void *d_out, size_t n, void *stream);
/* d_out[0] = product of d_in[0..n) in Fq12 (lib.rs:175-179 semantics; order-independent because Fq12 is commutative) */
int bn254_gt_product_dev(bn254_ctx *ctx, const void *d_in, size_t n, void *d_out, void *stream);
/* d_out[0] = final_exponentiation(d_in[0] * ... * d_in[m-1]), m >= 1: the tail of a sharded multi-pairing - the ranks' partial
   products after their exchange, then the ONE final exponentiation (fq12.rs:41-88 behind the fold of shootout/main.rs:11-16).
   Up to 16 values it is a single wave-cooperative launch (one Fq12 spread over a wave, ~0.5 ms instead of 2.9 ms); more go through
   the one-launch product tree first. */
int bn254_gt_product_final_exp_dev(bn254_ctx *ctx, const void *d_in, size_t m, void *d_out, void *stream);
/* local part of a sharded multi-pairing: un-exponentiated product of the Miller values of n pairs -> one Fq12 */
int bn254_miller_product_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, size_t n, void *d_partial, void *stream);
/* bn254_pairing_product_batch on device-resident p, q, out; `offsets` (m+1 entries) is HOST memory (the launches are planned from it) and
   may be freed on return */
int bn254_pairing_product_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_q, const size_t *offsets, size_t m, void *d_out, void *stream);
/* bn254_g{1,2}_msm_batch on device-resident p, k, out (m points); `offsets` (m+1 entries) is HOST memory and may be freed on return */
int bn254_g1_msm_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, const size_t *offsets, size_t m, void *d_out, void *stream);
int bn254_g2_msm_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, const size_t *offsets, size_t m, void *d_out, void *stream);
/* bn254_g{1,2}_msm on device-resident p, k (n terms) and out (ONE point), ordered on `stream`.  The bucket route plans from upper bounds: no
   count is read back; the call synchronises `stream` only when it changes the window width (see Threading above) */
int bn254_g1_msm_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, size_t n, void *d_out, void *stream);
int bn254_g2_msm_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, size_t n, void *d_out, void *stream);
/* ---- multi-scalar multiplication against PREPARED bases: a prover multiplies fresh scalars against the same points, proof after proof (a
   proving key, an SRS).  bn254_g{1,2}_msm_prepare takes n raw points (any z; z == 0 is infinity) once and returns a handle that owns, in
   device memory, the affine multiples 2^(c w) P_i for w < W = ceil(254 / c) - entry (w, i) at index w * n + i, one 80-byte record for G1
   (9 + 9 limbs of x and y, a flag word that is not zero for the point at infinity, a zero word) and two for G2 (component c0, then c1) -
   and the n normalised points.  window_bits: 0 for the default of the size, or 3 .. 16.  A handle of zero points is legal.
   bn254_g{1,2}_msm_prepared: out[0] = normalize(sum over i < n of P[first + i] * k[i]) - THE BYTES bn254_g{1,2}_msm returns for the same
   points and scalars; n == 0 gives G::zero() = (0, 1, 0).  Below the crossover (BN254_OPT_MSM_BUCKET_MIN when it is set - 0 forces the
   bucket route -, else this route's own default per group) the call is the one-segment bn254_g{1,2}_msm_batch on the handle's points; from
   there on every (term, window) pair falls into ONE set of 2^(c-1) buckets by its signed digit, level 0 of the accumulation is a mixed
   addition from a record, and the reduction and its tail shrink by 2 W against bn254_g{1,2}_msm.  Chunks of BN254_OPT_MSM_CHUNK terms.
   BN254_E_BAD_ARG, before any device work and whatever `ctx` is: NULL pointers with n > 0 (out: always), first + n > count, a handle of
   the other group, window_bits out of range, W * n >= 2^31.  The handle is a plain pointer here; its layout is private to the library.
   The _dev forms take device-resident points / scalars / out and are asynchronous on `stream` like bn254_g{1,2}_msm_dev (prepare_dev
   allocates the handle's memory, which synchronises with the device).  A handle belongs to the device of the context that made it. */
int bn254_g1_msm_prepare(bn254_ctx *ctx, const bn_g1 *p, size_t n, int window_bits, void **out);
int bn254_g2_msm_prepare(bn254_ctx *ctx, const bn_g2 *p, size_t n, int window_bits, void **out);
int bn254_g1_msm_prepare_dev(bn254_ctx *ctx, const void *d_p, size_t n, int window_bits, void **out, void *stream);
int bn254_g2_msm_prepare_dev(bn254_ctx *ctx, const void *d_p, size_t n, int window_bits, void **out, void *stream);
void bn254_msm_prepared_destroy(void *prep);
size_t bn254_msm_prepared_count(const void *prep);
size_t bn254_msm_prepared_bytes(const void *prep);            /* device memory: table and points */
int bn254_msm_prepared_group(const void *prep);               /* 1 or 2 (0 for NULL) */
int bn254_msm_prepared_window_bits(const void *prep);
/* for tests: the table as W * count entries of 80 (G1) / 160 (G2) bytes; `bytes` must be exactly that */
int bn254_msm_prepared_export(bn254_ctx *ctx, const void *prep, void *host_table, size_t bytes);
int bn254_g1_msm_prepared(bn254_ctx *ctx, const void *prep, size_t first, const bn_fr *k, size_t n, bn_g1 *out);
int bn254_g2_msm_prepared(bn254_ctx *ctx, const void *prep, size_t first, const bn_fr *k, size_t n, bn_g2 *out);
int bn254_g1_msm_prepared_dev(bn254_ctx *ctx, const void *prep, size_t first, const void *d_k, size_t n, void *d_out, void *stream);
int bn254_g2_msm_prepared_dev(bn254_ctx *ctx, const void *prep, size_t first, const void *d_k, size_t n, void *d_out, void *stream);
int bn254_g2_precompute_dev(bn254_ctx *ctx, const void *d_q, void *d_coeffs, size_t n, void *stream);
int bn254_miller_prepared_dev(bn254_ctx *ctx, const void *d_p, const void *d_coeffs, int shared, void *d_f, size_t n, void *stream);
/* native prepared-G2 mode on device-resident inputs.  bn254_g2_prepare_dev allocates the handle's table (that part synchronises with the
   device) and enqueues the precompute kernel on `stream`; the other two are asynchronous like the rest of this section.
   bn254_miller_prepared_native_dev returns the un-exponentiated Miller values (only meaningful in front of a final exponentiation). */
int bn254_g2_prepare_dev(bn254_ctx *ctx, const void *d_q, size_t nq, bn254_g2_prepared **out, void *stream);
int bn254_miller_prepared_native_dev(bn254_ctx *ctx, const void *d_p, const bn254_g2_prepared *prep, size_t q_first, void *d_f, size_t n, void *stream);
int bn254_pairing_prepared_native_batch_dev(bn254_ctx *ctx, const void *d_p, const bn254_g2_prepared *prep, size_t q_first, void *d_out, size_t n, void *stream);
/* local part of a multi-pairing over prepared points: un-exponentiated product of the Miller values of p[i] against point q_first + i -> one
   Fq12 (the counterpart of bn254_miller_product_dev; bn254_gt_product_final_exp_dev or bn254_final_exp_batch_dev finishes it) */
int bn254_miller_product_prepared_native_dev(bn254_ctx *ctx, const void *d_p, const bn254_g2_prepared *prep, size_t q_first, size_t n, void *d_partial, void *stream);
/* bn254_pairing_product_batch_prepared_native on device-resident p, q_index (n 64-bit words, or NULL) and out; `offsets` (m+1 entries) is HOST
   memory (the launches are planned from it) and may be freed on return.  d_q_index cannot be read on the host, so it is NOT checked: an index
   >= count is outside the contract, but memory safe - the kernels map it to the identity record the table ends with (the small route: to the
   point at infinity), so that pair contributes the factor one. */
int bn254_pairing_product_batch_prepared_native_dev(bn254_ctx *ctx, const void *d_p, const bn254_g2_prepared *prep, const void *d_q_index,
                                                    const size_t *offsets, size_t m, void *d_out, void *stream);
int bn254_gt_mul_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
int bn254_gt_pow_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_k, void *d_out, size_t n, void *stream);
int bn254_gt_inverse_batch_dev(bn254_ctx *ctx, const void *d_a, void *d_out, size_t n, void *stream);
int bn254_g1_mul_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, void *d_out, size_t n, void *stream);
int bn254_g2_mul_batch_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, void *d_out, size_t n, void *stream);
/* bn254_g{1,2}_mul_base_batch on device-resident k and out (n records), asynchronous on `stream`; `base` is HOST memory (ONE point), read
   before the call returns (the caller may overwrite it at once) */
int bn254_g1_mul_base_batch_dev(bn254_ctx *ctx, const bn_g1 *base, const void *d_k, void *d_out, size_t n, void *stream);
int bn254_g2_mul_base_batch_dev(bn254_ctx *ctx, const bn_g2 *base, const void *d_k, void *d_out, size_t n, void *stream);
/* bn254_g{1,2}_normalize_batch / bn254_g{1,2}_eq_batch on device-resident points (n records; d_out of eq: n int32), asynchronous on
   `stream`.  normalize: d_out may be exactly d_p; its prefix products are context-owned scratch (see Threading). */
int bn254_g1_normalize_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_out, size_t n, void *stream);
int bn254_g2_normalize_batch_dev(bn254_ctx *ctx, const void *d_p, void *d_out, size_t n, void *stream);
int bn254_g1_eq_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
int bn254_g2_eq_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
/* bn254_fr_{add,mul,inverse,pow,interpret}_batch on device-resident arrays (n records of 32 bytes; d_in of interpret: 64 n bytes; d_ok of
   inverse: n int32, or NULL), asynchronous on `stream`.  d_out may be exactly d_a or d_b.  inverse keeps its prefix products in
   context-owned scratch (see Threading); the others use none. */
int bn254_fr_add_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n, int negate_b, void *stream);
int bn254_fr_mul_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
int bn254_fr_inverse_batch_dev(bn254_ctx *ctx, const void *d_a, void *d_out, void *d_ok, size_t n, void *stream);
int bn254_fr_pow_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_e, void *d_out, size_t n, void *stream);
int bn254_fr_interpret_batch_dev(bn254_ctx *ctx, const void *d_in, void *d_out, size_t n, void *stream);
int bn254_fr_sqrt_batch_dev(bn254_ctx *ctx, const void *d_a, void *d_out, void *d_ok, size_t n, void *stream);
/* bn254_fr_ntt_batch on device-resident arrays (count 2^log_n records of 32 bytes, 16-byte aligned), asynchronous on `stream`; d_out may
   be exactly d_in; `shift` is HOST memory (one element or NULL), read before the call returns.  Tables and the arrays between the passes
   are context-owned scratch (see Threading). */
int bn254_fr_ntt_batch_dev(bn254_ctx *ctx, const void *d_in, void *d_out, int log_n, size_t count, int inverse, const bn_fr *shift, void *stream);
/* bn254_g{1,2}_ntt_batch on device-resident arrays (count 2^log_n records of 96 / 192 bytes, 16-byte aligned), asynchronous on `stream`;
   d_out may be exactly d_in; `shift` is HOST memory (one element or NULL), read before the call returns.  Tables, the array between the
   stages, window tables and prefix products are context-owned scratch (see Threading). */
int bn254_g1_ntt_batch_dev(bn254_ctx *ctx, const void *d_in, void *d_out, int log_n, size_t count, int inverse, const bn_fr *shift, void *stream);
int bn254_g2_ntt_batch_dev(bn254_ctx *ctx, const void *d_in, void *d_out, int log_n, size_t count, int inverse, const bn_fr *shift, void *stream);
/* bn254_fr_dot_batch on device-resident coeff (n records of 32 bytes, 16-byte aligned), d_index (n 64-bit words, or NULL), x (nx records) and
   out (m records); `offsets` (m+1 entries) is HOST memory (the launches are planned from it) and may be freed on return.  d_index cannot be
   read on the host, so it is NOT checked: an index >= nx is outside the contract, but memory safe - the kernel compares it before it loads
   anything through it, so that term contributes zero.  Work list and partial sums are context-owned scratch (see Threading). */
int bn254_fr_dot_batch_dev(bn254_ctx *ctx, const void *d_coeff, const void *d_index, const void *d_x, size_t nx, const size_t *offsets, size_t m, void *d_out,
                           void *stream);
/* bn254_fr_scan_batch on device-resident a, b (n records of 32 bytes, 16-byte aligned; with BN254_SCAN_A_PER_SEGMENT a has m), init (m records,
   or NULL) and out (n records; may be exactly d_a or d_b as above); `offsets` (m+1 entries) is HOST memory - the only thing the call reads:
   the launches are planned from it - and may be freed on return.  It waits for nothing and reads nothing back.  Work list, maps and
   carries are context-owned scratch (see Threading). */
int bn254_fr_scan_batch_dev(bn254_ctx *ctx, const void *d_a, const void *d_b, const void *d_init, const size_t *offsets, size_t m, unsigned int flags, void *d_out,
                            void *stream);
/* bn254_fr_mle_eq / bn254_fr_mle_fold / bn254_fr_sumcheck_round on device-resident records of 32 bytes, 16-byte aligned, asynchronous on `stream`:
   d_z (nv records) and d_out (2^nv); d_in (len records) and d_out (len / 2; may be exactly d_in); d_tables (n k records) and d_out (degree + 1).
   `r` of the fold and the group description of the round are HOST memory, read before the call returns, and may be freed then.  None
   waits for anything or reads anything back; the partial sums of the round are context-owned scratch (see Threading). */
int bn254_fr_mle_eq_dev(bn254_ctx *ctx, const void *d_z, int nv, void *d_out, void *stream);
int bn254_fr_mle_fold_dev(bn254_ctx *ctx, const void *d_in, size_t len, const bn_fr *r, void *d_out, void *stream);
int bn254_fr_sumcheck_round_dev(bn254_ctx *ctx, const void *d_tables, size_t n, size_t k, const size_t *group_offsets, const uint64_t *group_tables, const bn_fr *group_coeff,
                                size_t g, int degree, void *d_out, void *stream);
/* bn254_fr_sumcheck_fold_round on device-resident records of 32 bytes, 16-byte aligned, asynchronous on `stream`: d_tables holds n k records,
   d_folded n / 2 * k (it may be exactly d_tables: the call then runs in place and rows [n/2, n) are left as they were), d_out degree + 1.  `r`
   and the group description are HOST memory, read before the call returns.  Scratch and ordering are bn254_fr_sumcheck_round_dev's. */
int bn254_fr_sumcheck_fold_round_dev(bn254_ctx *ctx, const void *d_tables, size_t n, size_t k, const bn_fr *r, const size_t *group_offsets, const uint64_t *group_tables,
                                     const bn_fr *group_coeff, size_t g, int degree, void *d_folded, void *d_out, void *stream);
/* bn254_fr_mle_quotients on device-resident records of 32 bytes, 16-byte aligned, asynchronous on `stream`: d_a and d_out hold 2^nv records each and
   must not overlap; d_a is never written.  `z` (nv records) is HOST memory, read before the call returns, and may be freed then.  The call
   waits for nothing and reads nothing back; the working table between its passes is context-owned scratch (see Threading). */
int bn254_fr_mle_quotients_dev(bn254_ctx *ctx, const void *d_a, int nv, const bn_fr *z, void *d_out, void *stream);
/* bn254_fr_poseidon_batch / bn254_fr_poseidon_permute_batch / bn254_fr_merkle_tree on device-resident records of 32 bytes, 16-byte aligned, asynchronous on
   `stream`: d_in (n * arity records) and d_out (n); d_in and d_out (n * t each; d_out may be exactly d_in); d_leaves (2^log_n) and d_nodes
   (2^log_n - 1).  No host operand, no scratch; none waits for anything or reads anything back. */
int bn254_fr_poseidon_batch_dev(bn254_ctx *ctx, const void *d_in, int arity, void *d_out, size_t n, void *stream);
int bn254_fr_poseidon_permute_batch_dev(bn254_ctx *ctx, const void *d_in, int t, void *d_out, size_t n, void *stream);
int bn254_fr_merkle_tree_dev(bn254_ctx *ctx, const void *d_leaves, int log_n, void *d_nodes, void *stream);
/* bn254_fr_poseidon_ex_batch / bn254_fr_poseidon_chain_batch on device-resident records of 32 bytes, 16-byte aligned, asynchronous on `stream`: d_in
   (n * n_inputs records), d_init (n, or NULL) and d_out (n * n_outs); d_in (offsets[m] records) and d_out (m).  d_out must overlap no input (not
   checked).  `offsets` (m + 1 entries) is HOST memory, read before the call returns, and may be freed then.  The first call of a width on a
   context blocks while the width's constants are derived and copied to the device (see Threading); otherwise neither waits for anything or
   reads anything back. */
int bn254_fr_poseidon_ex_batch_dev(bn254_ctx *ctx, const void *d_in, int n_inputs, const void *d_init, int n_outs, void *d_out, size_t n, void *stream);
int bn254_fr_poseidon_chain_batch_dev(bn254_ctx *ctx, const void *d_in, const size_t *offsets, size_t m, int rate, void *d_out, void *stream);
/* raw Jacobian result of the reference's MSB-first double-and-add (what G::random produces, groups/mod.rs:220-222):
   used to generate benchmark inputs with z != 1 on the device */
int bn254_g1_mul_jacobian_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, void *d_out, size_t n, void *stream);
int bn254_g2_mul_jacobian_dev(bn254_ctx *ctx, const void *d_p, const void *d_k, void *d_out, size_t n, void *stream);

/* synthetic benchmark inputs, generated in HBM (mirrors benches/api.rs: G::random = one * Fr::random):
   d_out[j] = Montgomery image of (the 512-bit SplitMix64 draw of stream 2*(lo+j)+which, seeded `seed`) mod r - the distribution of
   arith.rs:195-198; equal to bn_amd.distributed.synthetic_scalars word for word (d_out: 16-byte aligned, like the records of the Fr
   _dev entry points).  bn254_tile_dev repeats one record n times. */
int bn254_synthetic_scalars_dev(bn254_ctx *ctx, uint64_t seed, uint64_t lo, size_t n, int which, void *d_out, void *stream);
int bn254_tile_dev(bn254_ctx *ctx, const void *d_record, size_t record_bytes, size_t n, void *d_out, void *stream);

/* ---- measurement ----------------------------------------------------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by hipEvents on its own stream; bn254_kernel_stats then reports the
   accumulated duration and launch count per kernel since the last reset (this is what bench.py's roofline uses). */
int bn254_profile_enable(bn254_ctx *ctx, int on);
int bn254_profile_reset(bn254_ctx *ctx);
/* kernel: "miller", "miller_shared", "miller_wave", "miller_quad", "pairing_wave", "final_exp", "final_exp_wave", "final_exp_quad", "exp_by_neg_z", "gt_product", "gt_tail", "gt_segment", "gt_tail_seg", "g1_mul", "g2_mul", "gt_mul", "gt_pow", "g2_precompute", "miller_prepared", "g2_prepare_native", "miller_native", "miller_native_shared", "miller_native_seg", "g2_gather", "wire_encode", "wire_decode", "fr_add", "fr_mul", "fr_inverse", "fr_pow", "fr_interpret", "gt_inverse", "g1_add", "g2_add", "g1_msm_mul", "g1_msm_fold", "g2_msm_mul", "g2_msm_fold", "g1_msm_digits", "g1_msm_bucket", "g1_msm_reduce", "g2_msm_digits", "g2_msm_bucket", "g2_msm_reduce", "g1_mul_base", "g2_mul_base", "g1_base_table", "g2_base_table", "g1_normalize", "g2_normalize", "g1_eq", "g2_eq".
   of bn254_fr_dot_batch: "fr_dot" (the pieces: products and sums), "fr_dot_fold" (the levels over the partial sums);
   of bn254_fr_scan_batch: "fr_scan" (the apply level, direct segments among it), "fr_scan_reduce" (the maps of the pieces), "fr_scan_up", "fr_scan_down" (the levels over the maps);
   of bn254_fr_mle_eq, bn254_fr_mle_fold and bn254_fr_sumcheck_round: "fr_mle_eq", "fr_mle_fold", "fr_sumcheck_round" (the lanes over the indices), "fr_sumcheck_sum" (the levels over the partial sums);
   of bn254_fr_mle_quotients: "fr_mle_quotients" (one scope per pass, or per sub-launch of it);
   of bn254_fr_sumcheck_fold_round: "fr_sumcheck_fold_round" (the lanes over the indices; the levels over its partial sums run under the round's scope for them);
   of bn254_fr_poseidon_batch, bn254_fr_poseidon_permute_batch and bn254_fr_merkle_tree: "fr_poseidon", "fr_poseidon_permute", "fr_merkle_level" (one scope per level, or per sub-launch of it);
   of bn254_fr_poseidon_ex_batch and bn254_fr_poseidon_chain_batch: "fr_poseidon_ex", "fr_poseidon_chain" (one scope per sub-launch);
   of bn254_g{1,2}_compress_batch and bn254_g{1,2}_decompress_batch: "g1_compress", "g2_compress", "g1_decompress", "g2_decompress" (one scope per sub-launch);
   of bn254_g1_map_to_curve_batch, bn254_g1_hash_to_curve_uniform_batch and bn254_g1_hash_to_curve_batch: "g1_map_to_curve", "g1_hash_to_curve", "g1_hash_to_curve_msg" (one scope per sub-launch);
   of bn254_g2_map_to_curve_batch, bn254_g2_clear_cofactor_batch, bn254_g2_hash_to_curve_uniform_batch and bn254_g2_hash_to_curve_batch: "g2_map_to_curve", "g2_clear_cofactor", "g2_hash_to_curve", "g2_hash_to_curve_msg" (one scope per sub-launch);
   of bn254_g1_validate_batch and bn254_g2_validate_batch: "g1_validate", "g2_validate" (one scope per sub-launch);
   of bn254_bjj_{validate,add,mul}_batch and bn254_eddsa_poseidon_{challenge,verify}_batch: "bjj_validate", "bjj_add", "bjj_mul", "eddsa_poseidon_challenge", "eddsa_poseidon_verify" (one scope per sub-launch);
   of bn254_fr_sqrt_batch, bn254_bjj_{pack,unpack}_batch and bn254_eddsa_poseidon_verify_packed_batch: "fr_sqrt", "bjj_pack", "bjj_unpack", "eddsa_poseidon_verify_packed" (one scope per sub-launch);
   of bn254_grumpkin_{validate,add,mul,msm}_batch: "grumpkin_validate", "grumpkin_add", "grumpkin_mul", "grumpkin_msm", "grumpkin_msm_fold" (one scope per sub-launch; the segmented sum: per sub-launch of a level);
   of bn254_g{1,2}_ntt_batch: "g1_ntt", "g2_ntt" (the stages, one scope per sub-launch), "g1_ntt_scale", "g2_ntt_scale" (the pass of a shift or of an inverse), "g1_ntt_normalize", "g2_ntt_normalize" (the normalisation that ends a call);
   of bn254_g{1,2}_msm_prepare and bn254_g{1,2}_msm_prepared: "g1_msmp_table", "g2_msmp_table" (a handle's build: one scope per window; its normalisations run under "g*_normalize"), "g1_msmp_digits", "g1_msmp_bucket", "g1_msmp_reduce", "g2_msmp_digits", "g2_msmp_bucket", "g2_msmp_reduce" (the bucket route of a call; its tail and the small route run under "g*_msm_mul" and "g*_msm_fold");
   and, of bn254_fr_ntt_batch: "ntt" (the passes), "ntt_table" (the builds of the twiddle tables).
   Synchronises and consumes the recorded events (totals accumulate until bn254_profile_reset). */
int bn254_kernel_stats(bn254_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches);
/* issue-rate ceiling of v_mad_u64_u32 (the 32x32+64 multiply-accumulate every field product is built from) at
   `waves_per_simd` resident waves: G lane-MACs per second over the whole chip and the kernel's duration.  bench.py prints it
   as the same-run `roofline.peak`. */
int bn254_ubench_mac32(bn254_ctx *ctx, int waves_per_simd, int iters, double *gmac_per_s, double *ms);
/* the same on operands of `operand_bits` random bits (1..32): the multiplier's rate depends on its data (profiles/r04_ubench_mad_data_dependence.txt);
   29 = the engine's own limbs, which is what bench.py prices `roofline.peak_at_kernel_occupancy` with */
int bn254_ubench_mac32_ex(bn254_ctx *ctx, int waves_per_simd, int iters, int operand_bits, double *gmac_per_s, double *ms);
/* d_out[i] = d_in[i].exp_by_neg_z() as the reference writes it (fields/fq12.rs:229-246), for ANY Fq12: the one function of the path
   whose known answer (fields/mod.rs:171-201) lies OFF the cyclotomic subgroup, where the result depends on the operation sequence.
   The engine's own exponentiation by u (shorter signed-digit chain, equal on every value a pairing produces) is not reachable with
   such an input; this entry point runs the reference's sequence so that its test vector can be checked on the device. */
int bn254_exp_by_neg_z_dev(bn254_ctx *ctx, const void *d_in, void *d_out, size_t n, void *stream);
/* the wave-cooperative machine on one wave: milliseconds for `iters` runs of program `which` (0 cyclotomic squaring, 1 Fq12
   product, 2 slot copy, 3 Frobenius map, 4 whole final exponentiation, 5 a fused run of five squarings) - the per-phase costs quoted in DESIGN.md */
int bn254_wave_ubench(bn254_ctx *ctx, int which, int iters, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* BN254_HIP_H */
