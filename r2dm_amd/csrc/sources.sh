# Sourced by build.sh and scripts/build_variant.sh: the translation units of libr2dm_hip.so, the headers they depend on and the flags each gets.
R2DM_SOURCES="conv_mfma conv_bf16x3 conv_f16x2 proj_f16x2 conv_direct norm resample attention embed posterior latent metrics render projection pointcloud pointnet rangenet postproc completion geometry voxel emd features cache plan forward engine ops_abi kernel_abi"
R2DM_HEADERS="common.h conv_epilogue.h conv_bf16x3.h f16x2.h wave_ops.h gn_math.h engine.h ../../include/r2dm_hip.h"
R2DM_FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-inline-asm"
# flags of source $1 beyond R2DM_FLAGS (the engine's host files -- plan, forward, engine, ops_abi, kernel_abi -- get none)
r2dm_extra_flags() {
  local extra=""
  case $1 in conv_bf16x3*|conv_f16x2|proj_f16x2|pointnet|rangenet|postproc) extra="-fno-slp-vectorize";; esac  # packed f32 VALU next to MFMAs is an anti-lever
  # Round 5: NO packed-fp32 instruction selection in the kernels that share CUs and whose packed instructions would take SGPR operands (attention, in_conv /
  # out_conv, the FIR resamplers, the posterior): a v_pk_mul / v_pk_fma_f32 with an SGPR-pair source read wrong values in lanes 48-63 whenever the wave shared its
  # CU with an LDS-holding workgroup of ANOTHER PROCESS (profiles/r05_coresidency.txt: the root of the "wrong next to a second process" family).  Costs nothing
  # (attention 77 -> 74 us, out_conv 54 -> 53 us, step +-0: scripts/jobs/j374.sh).  tests/test_host.py checks the built code objects.  (The host pass of hipcc
  # does not know the feature and says so on stderr: build.sh filters that.)
  case $1 in attention|conv_direct|resample|posterior|latent|norm|embed|metrics|render|projection|pointcloud|pointnet|rangenet|postproc|completion|geometry|voxel|emd|features|cache) extra="$extra -Xclang -target-feature -Xclang -packed-fp32-ops";; esac
  echo "$extra"
}
