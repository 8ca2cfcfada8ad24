#!/bin/bash
# kernel experiments: build_variants/lib_<name>.so from the working tree with extra hipcc flags, then
#   BN254_LIB_PATH=build_variants/lib_<name>.so python bench.py --full --no-cpu-baseline --no-host-api
# Only the units named in UNITS are recompiled with the flags (default: the lane-pair kernel file, where most experiments are);
# the other objects come from the last regular build (bn_amd/csrc/build/).
# (the two chains of the compressed encodings' square roots: UNITS=bn254_wire tools/build_variant.sh sqrt_plain -DBN254_SQRT_WINDOW=0, ... sqrt_window -DBN254_SQRT_WINDOW=1)
# (the two forms of hash-to-curve's inv0: UNITS=bn254_hash tools/build_variant.sh inv0_fermat -DBN254_H2C_INV0=0, ... inv0_cand -DBN254_H2C_INV0=1)
# (the two membership tests of the G2 decoders: UNITS=bn254_wire tools/build_variant.sh subgroup_chain -DBN254_G2_SUBGROUP_ENDO=0, ... subgroup_endo -DBN254_G2_SUBGROUP_ENDO=1)
# (the joint window of the EdDSA-Poseidon verifier: UNITS=bn254_babyjub tools/build_variant.sh eddsa_w1 -DBN254_EDDSA_WINDOW=1, ... eddsa_w2 -DBN254_EDDSA_WINDOW=2)
# (the two forms of the square root in Fr: UNITS="bn254_fr_sqrt bn254_babyjub" tools/build_variant.sh fr_sqrt_form0 -DBN254_FR_SQRT_FORM=0, ... fr_sqrt_form1 -DBN254_FR_SQRT_FORM=1)
# (the lanes per permutation of the wide Poseidon kernels: UNITS=bn254_poseidon_wide tools/build_variant.sh psdw_g4 -DBN254_POSEIDON_WIDE_LANES=4, ... psdw_g8 ...=8, ... psdw_g16 ...=16)
# (the window of [k]P on Grumpkin: UNITS=bn254_grumpkin tools/build_variant.sh grk_w4 -DBN254_GRUMPKIN_MUL_WINDOW=4, ... grk_w5 -DBN254_GRUMPKIN_MUL_WINDOW=5; its workgroups of 512 lanes: ... grk_b512 -DBN254_GRUMPKIN_BLOCK=512)
# usage: [UNITS="bn254_kernels_b bn254_kernels_mul"] tools/build_variant.sh NAME [extra hipcc flags...]
set -e
cd "$(dirname "$0")/.."
mkdir -p build_variants
name=$1; shift
B=bn_amd/csrc/build
UNITS=${UNITS:-bn254_kernels_b}
objs=""
for u in bn254_hip bn254_seg bn254_wire bn254_kernels_b bn254_kernels_mul bn254_kernels_w bn254_kernels_q bn254_multi bn254_measure bn254_fr bn254_fr_sqrt bn254_ntt bn254_group_ntt bn254_dot bn254_scan bn254_mle bn254_poseidon bn254_poseidon_wide bn254_hash bn254_hash_g2 bn254_validate bn254_babyjub bn254_grumpkin; do
  if [[ " $UNITS " == *" $u "* ]]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -mllvm -amdgpu-dpp-combine=false "$@" -c bn_amd/csrc/$u.hip -o build_variants/${u}_$name.o &
    objs="$objs build_variants/${u}_$name.o"
  else
    objs="$objs $B/$u.o"
  fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -ldl -lpthread -o build_variants/lib_$name.so
rm -f build_variants/*_$name.o
echo built build_variants/lib_$name.so
