// Kernel selection of the convolution launches: which kernel, which instantiation and what
// launch shape a ConvArgs / WgradArgs request runs on. The launchers (launch_conv_nt,
// launch_conv_wgrad) switch over the plan and decide nothing themselves; everything else that
// needs to know what will run (BN-statistics rows, masked stores, split counts) reads the plan.
//
// Both functions are pure: no HIP call, no static state, no allocation. Pointers are read for
// null-ness only, with one exception: the skinny narrow-N kernel loads its weights in 16-byte
// chunks, so the weight pointer's low four bits are part of its precondition.
#pragma once
#include "conv_args.h"

// element types as seg_common.h's SegDType (kept apart: this unit includes no ROCm header)
enum { CONV_SEL_F32 = 0, CONV_SEL_BF16 = 1, CONV_SEL_F16 = 2 };

enum ConvNtKernel {
  NT_INVALID = 0,
  NT_MFMA,        // conv_nt_kernel (conv.hip): any dtype, fp32 or storage-type output
  NT_V2,          // conv_nt_v2_kernel (conv_v2.hip): 16-bit LDS-DMA tile kernel
  NT_V2_DUAL,     //   ... with the K-concatenated second GEMM (Co <= 128)
  NT_PATCH,       // conv_nt_patch_kernel: small-channel 3 x 3 on input patches
  NT_PATCH_S2D,   // conv_nt_patch_s2d_kernel: the space-to-depth stem
  NT_PP,          // conv_nt_pp_kernel (conv_pp.hip): 256 x 256 ping-pong, Co > 128
  NT_SKINNY_N,    // skinny_narrow_n_kernel (skinny.hip): Co <= 16
  NT_SKINNY_K,    // skinny_narrow_k_kernel: C <= 16
};

struct ConvNtPlan {
  int kernel;      // ConvNtKernel
  int bm, bn;      // output tile: rows (pixels) x columns (channels)
  int st;          // MFMA / V2 / PATCH: the transposed stride ST (1, 2); PP: its ST (0 dense 1x1
                   // rows, 1, 2, 4 dense rows + second GEMM); SKINNY_K: the padded K (8, 16)
  int persist;     // PP: PERSIST (0 one tile per workgroup, 1 tile loop, 3 tile loop with the
                   // residual by LDS-DMA); the grid of 1 and 3 is clamped to the CU count
  int tap8;        // V2: the tap mode T8 (2 for the space-to-depth stem)
  int small;       // V2 / V2_DUAL: the 128-row tile of the narrow (Co <= 64) layers
  int generic;     // MFMA: the unaligned gather
  int out_f32;     // MFMA: fp32 output of a 16-bit conv
  int stat_rows;   // rows one BN-statistics partial covers (bn_stats_finalize's tile_rows)
  int omask;       // the launch stores through ConvArgs::omask
  long wgs;        // workgroups, before the persistent clamp
  int lds;         // dynamic LDS bytes
  const char* reason;   // NT_INVALID: why
};

ConvNtPlan conv_nt_plan(int dtype, int out_f32, const ConvArgs& a);

// Dynamic LDS bytes of the kernels below: the plan reports them and each launcher static_asserts
// its own constant against them, so the description cannot drift from the launch.
//   conv_nt_v2_kernel: a ring of 2 (BN 256) or 3 stages of (BM + BN) 128-byte rows, or the
//   epilogue staging of BM rows if that is larger
constexpr int conv_nt_v2_lds(int bm, int bn) {
  const int ring = (bn == 256 ? 2 : 3) * (bm + bn) * 128, epi = bm * (64 + 4) * 4;
  return ring > epi ? ring : epi;
}
constexpr int CONV_NT_PATCH_LDS = 384 * 128 + 3 * 64 * 128;   // one patch buffer + 3 weight stages
constexpr int CONV_NT_PATCH_S2D_LDS = 256 * (64 + 4) * 4;     // the epilogue staging
constexpr int CONV_NT_PP_LDS = 2 * 4 * 128 * 128;             // two K-tile buffers of four half-tiles
//   conv_wgrad_v2_kernel: 3 stages (2 at 256 x 256) of 64 pixels x (BM + BN) 16-bit values
constexpr int conv_wgrad_v2_lds(int bm, int bn) {
  return (bm == 256 && bn == 256 ? 2 : 3) * 64 * (bm + bn) * 2;
}
constexpr int CONV_WGRAD_PP_LDS = 2 * 4 * 64 * 256;
constexpr int CONV_WGRAD_PATCH_LDS = 3 * 40 * 1024;           // three stages of 40 1-KB DMA pieces

enum ConvWgradKernel {
  WG_INVALID = 0,
  WG_MFMA,    // conv_wgrad_kernel (conv.hip)
  WG_V2,      // conv_wgrad_v2_kernel (conv_v2.hip), tile bm x bn
  WG_PP,      // conv_wgrad_pp_kernel (conv_pp.hip), 256 x 256
  WG_PATCH,   // conv_wgrad_patch_kernel (wgrad_patch.hip), 64 x 64-channel blocks
};

struct ConvWgradPlan {
  int kernel;        // ConvWgradKernel
  int bm, bn;        // tile: output channels x (tap, input channel) columns
  int generic;       // MFMA: the unaligned gather
  int fast;          // PP: row decode (0 any Wo, 1 Wo >= 64, 2 strip order)
  long tiles;        // workgroups per split of the kernel that runs
  long split_tiles;  // the tile count the split heuristic divides its workgroup target by
  int lds;           // dynamic LDS bytes
  const char* reason;
};

// force_bm, force_bn: 0 = the heuristic tile; 64 / 128 / 256 forces that tile of the 16-bit v2 /
// ping-pong kernels (tuning tools, and the folded conv3 weight gradient's 256 x 256)
ConvWgradPlan conv_wgrad_plan(int dtype, const WgradArgs& a, int force_bm = 0, int force_bn = 0);
