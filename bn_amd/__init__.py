"""bn_amd - MI355X-native batched BN254 optimal-ate pairing engine (HIP/gfx950) behind the API surface of the
reference crate zcash-hackworks/bn (`Fr`, `G1`, `G2`, `Gt`, `pairing`; src/lib.rs).

Everything computes on the GPU through libbn254_hip.so (C ABI: include/bn254_hip.h).  There is no CPU fallback: importing is
cheap, but any computation without the built library and a HIP device raises.
"""
from .engine import Engine, MultiEngine, PreparedG2 as PreparedG2Handle, PreparedMSM, FR_BYTES, G1_WORDS, G2_WORDS, GT_WORDS  # noqa: F401
from .api import Fr, G1, G2, Gt, PreparedG2, pairing, pairing_batch, pairing_product, pairing_product_batch, pairing_check_batch, g1_msm_batch, g2_msm_batch, g1_msm, g2_msm, g1_msm_prepare, g2_msm_prepare, g1_mul_base, g2_mul_base, g1_normalize_batch, g2_normalize_batch, g1_eq_batch, g2_eq_batch, fr_add_batch, fr_sub_batch, fr_neg_batch, fr_mul_batch, fr_pow_batch, fr_inverse_batch, fr_sqrt_batch, fr_interpret_batch, fr_ntt, fr_ntt_batch, g1_ntt, g2_ntt, g1_ntt_batch, g2_ntt_batch, fr_dot_batch, fr_scan_batch, fr_mle_eq, fr_mle_fold, fr_sumcheck_round, fr_sumcheck_fold_round, fr_mle_quotients, fr_poseidon_batch, fr_poseidon_permute_batch, fr_poseidon_ex_batch, fr_poseidon_chain_batch, fr_merkle_tree, g1_compress_batch, g2_compress_batch, g1_decompress_batch, g2_decompress_batch, DecodeError, g1_map_to_curve_batch, g1_hash_to_curve_batch, g2_map_to_curve_batch, g2_clear_cofactor_batch, g2_hash_to_curve_batch, g1_validate_batch, g2_validate_batch, bjj_validate_batch, bjj_add_batch, bjj_mul_batch, eddsa_poseidon_challenge_batch, eddsa_poseidon_verify_batch, bjj_pack_batch, bjj_unpack_batch, eddsa_poseidon_verify_packed_batch, grumpkin_validate_batch, grumpkin_add_batch, grumpkin_mul_batch, grumpkin_msm_batch  # noqa: F401
from . import groth16  # noqa: F401
from . import poly  # noqa: F401
from . import kzg  # noqa: F401
from . import mle  # noqa: F401
from . import sumcheck  # noqa: F401
from . import mkzg  # noqa: F401
from . import poseidon  # noqa: F401
from . import merkle  # noqa: F401
from . import hash_to_curve  # noqa: F401
from . import bls  # noqa: F401
from . import bls_minpk  # noqa: F401
from . import babyjub  # noqa: F401
from . import eddsa  # noqa: F401
from . import grumpkin  # noqa: F401
from . import pedersen  # noqa: F401
from . import ipa  # noqa: F401
