// Implicit-GEMM convolutions on CDNA4 MFMA (gfx950). No im2col buffer is ever built: the
// A-operand gather computes each source pixel (with TF padding / dilation / stride) while
// staging tiles into LDS.
//
//   forward : y[p][co]  = sum_{kh,kw,ci} x[src(p,kh,kw)][ci] * w[co][kh][kw][ci]
//   dgrad   : dx[p][ci] = sum_{kh,kw,co} dy[src_t(p,kh,kw)][co] * wT[ci][kh][kw][co]
//             (wT = spatially flipped, transposed weights; stride>1 uses the divisibility
//              gather of a transposed conv)
//   wgrad   : dw[co][kh][kw][ci] = sum_p dy[p][co] * x[src(p,kh,kw)][ci]   (split-K slabs)
#pragma once
#include "seg_common.h"
#include "conv_args.h"
#include "conv_select.h"

// host launchers (conv.hip); return hipError_t. Each computes the plan of its arguments
// (conv_select.h) and launches the kernel it names; an invalid plan is hipErrorInvalidValue.
// force_bm / force_bn: conv_wgrad_plan's forced tile
hipError_t launch_conv_nt(int dtype, int out_f32, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_wgrad(int dtype, const WgradArgs& a, hipStream_t s, int force_bm = 0,
                             int force_bn = 0);
hipError_t launch_splitk_reduce(const float* part, int splits, long split_stride, long n,
                                float* out, int accumulate, hipStream_t s);
// all layers' flips in one launch: table of FlipJob (device), prefix = the job's first tile;
// total = flip tiles over all jobs
struct FlipJob { const void* w; void* wt; int co, k, ci; long prefix; };
long flip_tiles(int co, int k, int ci);
hipError_t launch_weight_flip_batched(int dtype, const FlipJob* jobs, int njobs, long total,
                                      hipStream_t s);
hipError_t launch_weight_flip_transpose(int dtype, const void* w, void* wt, int co, int kh, int kw,
                                        int ci, hipStream_t s);
int conv_nt_mtiles(long M);  // upper bound on BN-stat partial tiles (128-row tiles)

// 7x7 / 2 stem (3 channels) in 16-bit storage as a 4x4 / 1 VALID conv over a space-to-depth
// image: X'[n][i][j][(dh*2 + dw)*3 + c] = x[n][2i + dh - pad_h][2j + dw - pad_w][c] (channels
// 12..15 zero), Hs = Ho + 3, Ws = Wo + 3; w'[co][a][b][(dh*2 + dw)*3 + c] = w[co][2a+dh][2b+dw][c]
// (zero past the 7x7 kernel), K = 4 * 4 * 16 = 256 (tap mode, tap8 = 2)
//   images f32 [N][H][W][3] -> s2d [N][Hs][Ws][16]
hipError_t launch_cast_s2d(int dtype, const float* src, void* dst, int N, int H, int W, int Hs, int Ws,
                           int pad_h, int pad_w, hipStream_t s);
//   s2d [N][Hs][Ws][16] -> [N][H][W][8] (channels 0..2 the image, 3..7 zero): parity tests' view
hipError_t launch_unshuffle_s2d(const void* src, void* dst, int N, int H, int W, int Hs, int Ws,
                                int pad_h, int pad_w, hipStream_t s);
//   weights 16-bit [Co][7][7][3] -> [Co][256]
hipError_t launch_stem_s2d_weights(const bf16_t* w, bf16_t* wp, int co, hipStream_t s);
//   split-K slabs [splits][co_pad][256] of the s2d weight gradient -> fp32 [co][7][7][3]
hipError_t launch_splitk_reduce_s2d(const float* part, int splits, long split_stride, int co,
                                    float* out, hipStream_t s);
