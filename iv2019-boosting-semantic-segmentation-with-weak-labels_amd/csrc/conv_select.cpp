// Kernel selection (conv_select.h). Host-only and pure; every shape precondition of the
// convolution kernels lives in this file.
#include "conv_select.h"

#include <algorithm>

namespace {

constexpr long LIM31 = 1L << 31;    // 32-bit pixel indices / buffer offsets
constexpr int BK = 64;              // 16-bit K-step of the tile kernels (128-B LDS rows)
constexpr int PT_H = 8, PT_W = 32;  // the patch kernels' output tile

bool half(int dt) { return dt == CONV_SEL_BF16 || dt == CONV_SEL_F16; }
long cdiv(long a, long b) { return (a + b - 1) / b; }
long pixels(const ConvArgs& a) { return (long)a.N * a.Ho * a.Wo; }

// dense 1 x 1 rows: the output pixel is the input pixel
bool dense_1x1(const ConvArgs& a) {
  return a.st == 1 && a.KH == 1 && a.KW == 1 && a.sf == 1 && a.pad_h == 0 && a.pad_w == 0 &&
         a.H == a.Ho && a.W == a.Wo;
}

// ---- the 16-bit tile kernels (conv_v2.hip): C % 64 == 0, ld / Co multiples of 8 ----
bool nt_v2_ok(const ConvArgs& a) {
  if (a.tap8)   // tap mode (the space-to-depth stem): taps of C = 8 * tap8 channels (tap8 = 2),
                // weights [Co][ldw >= ceil(KH*KW*C/64)*64]
    return a.tap8 == 2 && a.st == 1 && a.C == 16 && a.ldx == 16 && a.Co <= 64 && (a.Co % 8) == 0 &&
           (a.ldy % 8) == 0 && a.ldw >= (a.KH * a.KW * a.C + BK - 1) / BK * BK && (a.ldw % 8) == 0 &&
           !a.r && !a.r2 && pixels(a) < LIM31;
  return (a.st == 1 || a.st == 2) && (a.C % BK) == 0 && (a.ldx % 8) == 0 && (a.ldw % 8) == 0 &&
         (a.Co % 8) == 0 && (a.ldy % 8) == 0 && (!a.r || a.ldr % 8 == 0) &&
         (!a.r2 || a.ldr2 % 8 == 0) && pixels(a) < LIM31;   // 32-bit pixel decode
}

// the stem's patch kernel: the s2d tap mode with 64 output channels on whole 8 x 32 tiles
bool nt_patch_s2d_ok(const ConvArgs& a) {
  return a.tap8 == 2 && a.C == 16 && a.ldx == 16 && a.Co == 64 && a.KH == 4 && a.KW == 4 &&
         a.sf == 1 && a.pad_h == 0 && a.pad_w == 0 && a.dil == 1 && a.ldw >= 256 && a.ldw % 8 == 0 &&
         a.H == a.Ho + 3 && a.W == a.Wo + 3 && a.Ho % PT_H == 0 && a.Wo % PT_W == 0 && a.ldy % 8 == 0 &&
         !a.r && !a.r2;
}

// the patch kernel's shapes (measured against the v2 gather in
// profiles/r02_ab_v19_patch_stem.txt)
bool nt_patch_ok(const ConvArgs& a) {
  return !a.tap8 && a.st == 1 && a.sf == 1 && a.dil == 1 && a.KH == 3 && a.KW == 3 &&
         (a.C == 64 || a.C == 128) && (a.Co == 64 || a.Co == 128) && a.ldw == 9 * a.C &&
         a.H == a.Ho && a.W == a.Wo && a.Ho % PT_H == 0 && a.Wo % PT_W == 0 &&
         a.pad_h >= 0 && a.pad_h <= 2 && a.pad_w >= 0 && a.pad_w <= 2 &&
         a.ldx % 8 == 0 && a.ldy % 8 == 0;
}

// K-concatenated second GEMM on output tiles of <= 128 channels (dense 1x1 rows only)
bool nt_v2_dual_ok(const ConvArgs& a) {
  return a.x2 && a.st == 1 && a.sf == 1 && a.KH == 1 && a.KW == 1 && a.pad_h == 0 && a.pad_w == 0 &&
         a.H == a.Ho && a.W == a.Wo && a.Co <= 128 && a.C2 % BK == 0 && a.ldx2 % 8 == 0 &&
         a.ldw2 % 8 == 0 && !a.r && !a.r2 && !a.stats && !a.tap8;
}

// ping-pong (conv_pp.hip): the v2 preconditions, Co > 128, operands of < 2^31 bytes (32-bit
// buffer offsets), kernels up to 4 x 4 (tap validity bits); 16-byte epilogue stores
bool nt_pp_ok(const ConvArgs& a) {
  return !a.tap8 && a.Co > 128 && a.Co % 8 == 0 && a.ldy % 8 == 0 &&
         a.KH <= 4 && a.KW <= 4 && nt_v2_ok(a) &&
         (long)a.N * a.H * a.W * a.ldx * 2 < LIM31 && (long)a.Co * a.ldw * 2 < LIM31 &&
         pixels(a) < LIM31 &&
         (!a.x2 || (dense_1x1(a) && a.C % 64 == 0 && a.C2 % 64 == 0 && a.ldx2 % 8 == 0 &&
                    a.ldw2 % 8 == 0 && (long)a.N * a.H * a.W * a.ldx2 * 2 < LIM31 &&
                    (long)a.Co * a.ldw2 * 2 < LIM31 && !a.r && !a.r2));
}

// launches that apply ConvArgs::omask: 16-bit dense 1x1 ping-pong, one tile per workgroup (the
// identity units' conv1 data gradient with its residual; a projection unit's K-concatenated
// conv1 + shortcut data gradient; decrease_fdims' data gradient into block4)
bool nt_omask_ok(int dtype, const ConvArgs& a) {
  return half(dtype) && !a.tap8 && dense_1x1(a) && a.Co > 128 && nt_pp_ok(a) && a.ldm >= a.Co / 8;
}

// skinny 1x1 convs (skinny.hip): N <= 16 (the logits convs, with BN partials per 128 rows) or
// K <= 16 (their data gradients), 16-bit storage; taken where the tile kernels cannot run
constexpr int SK_THREADS = 256, SK_ROWS = 128;
bool nt_skinny_ok(int dtype, int out_f32, const ConvArgs& a) {
  if (!half(dtype) || out_f32 || a.KH != 1 || a.KW != 1 || a.sf != 1 || a.st != 1 || a.pad_h ||
      a.pad_w || a.r || a.r2 || a.tap8)
    return false;
  if (a.Co <= 16)   // narrow N: 16-B pixel and weight loads, 4-channel stores inside ldy
    return a.C % 32 == 0 && a.C <= 512 && a.ldx % 8 == 0 && a.ldy >= (a.Co + 3) / 4 * 4 &&
           a.ldy % 4 == 0 && a.ldw % 8 == 0 && ((uintptr_t)a.w & 15) == 0;
  // narrow K (data gradient of a narrow conv): no BN statistics; the weight table (K x Co fp32)
  // fits the block's LDS
  return a.C <= 16 && a.ldx % 8 == 0 && a.ldx >= (a.C <= 8 ? 8 : 16) && a.Co % 8 == 0 &&
         a.ldy % 8 == 0 && SK_THREADS % (a.Co / 8) == 0 && a.Co / 8 <= SK_THREADS && a.Co <= 1024 &&
         !a.stats;
}

ConvNtPlan nt_invalid(const char* why) {
  ConvNtPlan p{};
  p.reason = why;
  return p;
}

// conv_nt_v2_kernel<E, BN, WMW, WNW, STAGES, ST, T8, BM, DU>: BN 256 runs 2 stages, 128 and
// 64 run 3; LDS = max(the stage ring, the epilogue staging of BM rows)
ConvNtPlan nt_v2(const ConvArgs& a, int kernel, int bn, int bm, int st, int tap8) {
  ConvNtPlan p{};
  p.kernel = kernel; p.bm = bm; p.bn = bn; p.st = st; p.tap8 = tap8; p.small = bm == 128;
  p.stat_rows = bm;
  p.wgs = cdiv(pixels(a), bm) * cdiv(a.Co, bn);
  p.lds = conv_nt_v2_lds(bm, bn);
  return p;
}

ConvNtPlan nt_pp(const ConvArgs& a) {
  ConvNtPlan p{};
  p.kernel = NT_PP; p.bm = 256; p.bn = 256;
  const long M = pixels(a);
  p.st = dense_1x1(a) ? (a.x2 ? 4 : 0) : a.st;
  // dense 1 x 1 rows, one residual: the residual tile by LDS-DMA (32-bit offsets into it)
  if (p.st == 0 && a.r && !a.r2 && M * a.ldr * 2 < LIM31) p.persist = 3;
  else p.persist = (a.r || a.r2 || a.omask) ? 0 : 1;
  // one partial per wave row (128 rows). Forward launches carry no residual; for a launch with
  // one the answer stays the 256 rows conv_nt_stat_rows gave before this unit existed (no caller
  // asks for statistics and a residual together)
  p.stat_rows = (a.r || a.r2) ? 256 : 128;
  p.omask = a.omask != nullptr;
  p.wgs = cdiv(M, 256) * cdiv(a.Co, 256);
  p.lds = CONV_NT_PP_LDS;
  return p;
}

// the 16-bit tile kernels of a request nt_v2_ok admits
ConvNtPlan nt_tile_plan(const ConvArgs& a) {
  // 128-row tiles, two workgroups per CU, for the narrow (Co <= 64) layers -- the stem and
  // block1: short reductions whose one-tile-per-CU 256-row launches were latency-bound (stem
  // forward 287 -> 241 us, block1 1x1 / 3x3 layers 4-18 % faster). (Measured and rejected: 128 x
  // 128 tiles with a 64 KB ring, two workgroups per CU, for short reductions K <= 512 -- 10-20 %
  // slower than 256-row tiles on the C2 1x1 layers.)
  const int bm_narrow = a.Co <= 64 ? 128 : 256;
  if (a.tap8) {
    if (a.x2) return nt_invalid("second GEMM: not in tap mode");
    if (nt_patch_s2d_ok(a)) {
      ConvNtPlan p{};
      p.kernel = NT_PATCH_S2D; p.bm = 256; p.bn = 64; p.st = 1; p.tap8 = 2; p.stat_rows = 256;
      p.wgs = (long)a.N * (a.Ho / PT_H) * (a.Wo / PT_W);
      p.lds = CONV_NT_PATCH_S2D_LDS;
      return p;
    }
    return nt_v2(a, NT_V2, 64, bm_narrow, 1, 2);
  }
  if (a.x2) {
    // K-concatenated second GEMM: ping-pong when the output has more than 128 channels, else
    // the v2 dual
    if (a.Co > 128) return nt_pp_ok(a) ? nt_pp(a) : nt_invalid("second GEMM: shape not on the ping-pong path");
    if (!nt_v2_dual_ok(a)) return nt_invalid("second GEMM: dense 1x1 rows, no residual or statistics");
    return a.Co > 64 ? nt_v2(a, NT_V2_DUAL, 128, 256, 1, 0) : nt_v2(a, NT_V2_DUAL, 64, 128, 1, 0);
  }
  if (nt_patch_ok(a)) {
    // 64-channel output tiles with one patch buffer fit 72 KB and 110 VGPRs: two workgroups
    // per CU hide each other's barrier and fragment-read latency (a 128-channel tile at two
    // per CU needs <= 128 VGPRs and spilled); Co = 128 runs as two such tiles per patch, the
    // 128-channel input as two chunks with the patch reloaded between them
    ConvNtPlan p{};
    p.kernel = NT_PATCH; p.bm = 256; p.bn = 64; p.st = 1; p.stat_rows = 256;
    p.wgs = (long)a.N * (a.Ho / PT_H) * (a.Wo / PT_W) * (a.Co / 64);
    p.lds = CONV_NT_PATCH_LDS;
    return p;
  }
  if (a.Co > 128) return nt_pp_ok(a) ? nt_pp(a) : nt_v2(a, NT_V2, 256, 256, a.st, 0);
  if (a.Co > 64) return nt_v2(a, NT_V2, 128, 256, a.st, 0);
  return nt_v2(a, NT_V2, 64, bm_narrow, a.st, 0);
}

}  // namespace

ConvNtPlan conv_nt_plan(int dtype, int out_f32, const ConvArgs& a) {
  if (a.omask && out_f32) return nt_invalid("omask: no fp32-output launch applies it");
  if (a.omask && !nt_omask_ok(dtype, a)) return nt_invalid("omask: 16-bit dense 1x1 ping-pong launches only");
  if (a.x2 && (a.r || a.r2)) return nt_invalid("second GEMM: no residual");
  if (half(dtype) && !out_f32 && nt_v2_ok(a)) return nt_tile_plan(a);
  if (a.x2) return nt_invalid("second GEMM: 16-bit tile kernels only");
  if (a.tap8) return nt_invalid("tap mode: 16-bit tile kernels only");
  const long M = pixels(a);
  ConvNtPlan p{};
  if (nt_skinny_ok(dtype, out_f32, a)) {
    p.stat_rows = SK_ROWS;
    if (a.Co <= 16) {
      p.kernel = NT_SKINNY_N; p.bm = SK_ROWS; p.bn = 16;
      p.wgs = cdiv(M, SK_ROWS);
      return p;
    }
    // ~4 blocks per CU: every block stages the weight table once, so the grid stays small and
    // each thread walks many rows
    const int per = SK_THREADS / (a.Co / 8);
    p.kernel = NT_SKINNY_K; p.bm = 4 * per; p.bn = a.Co; p.st = a.C <= 8 ? 8 : 16;
    p.wgs = std::min<long>(1024, cdiv(M, 4L * per));
    p.lds = (p.st / 2) * a.Co * 4;
    return p;
  }
  // conv_nt_kernel<T, TO, BM, BN, G>: 128 x 128 tiles, 128 x 64 for Co <= 64 and for the generic
  // gather (channels or strides that are no multiple of the K-step / a 16-byte chunk)
  const int bk = half(dtype) ? 64 : 32, epc = half(dtype) ? 8 : 4;
  p.kernel = NT_MFMA; p.st = a.st; p.out_f32 = out_f32 != 0; p.stat_rows = 128;
  p.generic = (a.C % bk) != 0 || (a.ldx % epc) != 0 || (a.ldw % epc) != 0;
  p.bm = 128; p.bn = (p.generic || a.Co <= 64) ? 64 : 128;
  p.wgs = cdiv(M, p.bm) * cdiv(a.Co, p.bn);
  return p;
}

// ------------------------------------------------------------------------------------------
// weight gradient
// ------------------------------------------------------------------------------------------
namespace {

long wg_pixels(const WgradArgs& a) { return (long)a.N * a.Ho * a.Wo; }

bool wg_v2_ok(const WgradArgs& a) {
  return (a.C % 8) == 0 && (a.ldx % 8) == 0 && (a.Co % 8) == 0 && (a.lddy % 8) == 0 &&
         wg_pixels(a) < LIM31 &&
         (!a.dy2 || (a.Co1 % 8 == 0 && a.Co1 < a.Co && a.lddy2 % 8 == 0));
}

// 256 x 256 ping-pong tiles with operands < 2^31 bytes (32-bit buffer offsets)
bool wg_pp_ok(const WgradArgs& a) {
  const long P = wg_pixels(a);
  return (a.C % 8) == 0 && (a.ldx % 8) == 0 && (a.Co % 8) == 0 && (a.lddy % 8) == 0 &&
         P * a.lddy * 2 < LIM31 && (long)a.N * a.H * a.W * a.ldx * 2 < LIM31 &&
         (!a.dy2 || (a.Co1 % 256 == 0 && a.Co1 < a.Co && a.lddy2 % 8 == 0 && P * a.lddy2 * 2 < LIM31));
}

// small-channel 3 x 3 stride-1 weight gradient on input patches (wgrad_patch.hip): SAME (pad =
// dilation <= 4), output rows in 64-pixel strips, 64-channel blocks of both Co and C (at most
// 128 each: the wider layers keep the ping-pong 256 x 256 tiles), operands < 2^31 bytes
bool wg_patch_ok(const WgradArgs& a) {
  return a.KH == 3 && a.KW == 3 && a.sf == 1 && a.dil >= 1 && a.dil <= 4 && a.pad_h == a.dil &&
         a.pad_w == a.dil && a.H == a.Ho && a.W == a.Wo && a.Wo % 64 == 0 && a.C % 64 == 0 &&
         a.Co % 64 == 0 && a.C <= 128 && a.Co <= 128 && a.ldx % 8 == 0 && a.lddy % 8 == 0 &&
         (long)a.N * a.H * a.W * a.ldx * 2 < LIM31 && wg_pixels(a) * a.lddy * 2 < LIM31;
}

// tile (BM co x BN cols): the largest the extents fill -- 256 x 256 (wave tiles 128 x 64)
// keeps LDS fragment traffic below the MFMA time and halves L2 re-reads vs 128 x 256 -- then
// halved (larger side first) while tiles x pixel splits would leave fewer than 128 workgroups
// (small outputs such as 256 x 256 1x1 convs: 1 tile x 64 splits = 64 workgroups otherwise).
// 128, the side stream's workgroup target: halving down to 256 workgroups (round 5) gave
// block2 / head 1 x 1 layers 128 x 128 tiles where 128 x 256 / 256 x 128 now run at the same
// workgroup count with half the operand re-reads: step +0.53 % (three interleaved pairs,
// profiles/r06_s30_wgrad_tile_target.txt; 64: +0.27 %)
void wg_v2_tile(int Co, int Ncol, long P, int* bm, int* bn) {
  int m = Co <= 64 ? 64 : (Co <= 128 ? 128 : 256);
  int n = Ncol <= 64 ? 64 : (Ncol <= 128 ? 128 : 256);
  const long maxs = std::min<long>(256, std::max<long>(1, P / 2048));
  auto blocks = [&]() { return (long)((Co + m - 1) / m) * ((Ncol + n - 1) / n) * maxs; };
#ifndef WG_TILE_TARGET
#define WG_TILE_TARGET 128
#endif
  while (blocks() < WG_TILE_TARGET) {
    if (m >= n && m > 64) m /= 2;
    else if (n > 64) n /= 2;
    else break;
  }
  *bm = m;
  *bn = n;
}

}  // namespace

ConvWgradPlan conv_wgrad_plan(int dtype, const WgradArgs& a, int force_bm, int force_bn) {
  const int Ncol = a.KH * a.KW * a.C;
  const long P = wg_pixels(a);
  const bool forced = force_bm || force_bn;
  ConvWgradPlan p{};
  // The split heuristic's tile count. Where the 16-bit patch / v2 / ping-pong kernels run it is
  // the launched kernel's; for the fp32/MFMA kernel it stays the count the splits were tuned
  // with (the v2 tile choice when C % 8 == 0, else 64- or 128-row x 128-column tiles), not that
  // kernel's own 64-column generic tiles: split counts fix the summation order
  {
    int bm = a.Co <= 64 ? 64 : 128, bn = 128;
    if (a.C % 8 == 0) wg_v2_tile(a.Co, Ncol, P, &bm, &bn);
    p.split_tiles = cdiv(a.Co, bm) * cdiv(Ncol, bn);
  }
  auto invalid = [&p](const char* why) { p.kernel = WG_INVALID; p.reason = why; return p; };
  auto tile_ok = [](int t) { return t == 64 || t == 128 || t == 256; };
  if (forced && !(tile_ok(force_bm) && tile_ok(force_bn))) return invalid("forced tile: 64, 128 or 256 each way");
  if (forced && !(half(dtype) && wg_v2_ok(a))) return invalid("forced tile: shape not on the 16-bit v2 path");
  if (a.dy2 && !(half(dtype) && a.KH == 1 && a.KW == 1 && wg_v2_ok(a)))
    return invalid("second dy source: 16-bit 1x1 on the v2 path only");
  if (half(dtype) && !forced && wg_patch_ok(a)) {
    p.kernel = WG_PATCH; p.bm = 64; p.bn = 64;
    p.tiles = p.split_tiles = (long)(a.Co / 64) * (a.C / 64);
    p.lds = CONV_WGRAD_PATCH_LDS;
    return p;
  }
  if (half(dtype) && wg_v2_ok(a)) {
    p.bm = force_bm; p.bn = force_bn;
    if (!forced) wg_v2_tile(a.Co, Ncol, P, &p.bm, &p.bn);
    p.tiles = cdiv(a.Co, p.bm) * cdiv(Ncol, p.bn);
    if (p.bm == 256 && p.bn == 256 && wg_pp_ok(a)) {
      p.kernel = WG_PP;
      // strip order where the rows split into whole 64-pixel K-tiles and the pixel rows repeat
      // across taps (KH > 1); 1x1 layers read every x row once, raster order is as good there
      p.fast = ((a.Wo % 64) == 0 && a.KH > 1) ? 2 : (a.Wo >= 64 ? 1 : 0);
      p.lds = CONV_WGRAD_PP_LDS;
      return p;
    }
    p.kernel = WG_V2;
    p.lds = conv_wgrad_v2_lds(p.bm, p.bn);
    return p;
  }
  // conv_wgrad_kernel<T, BM, BN, G>: 16-byte dy rows; generic = the unaligned x gather
  const int epc = half(dtype) ? 8 : 4;
  if (a.Co % epc != 0 || a.lddy % epc != 0) return invalid("dy rows are not 16-byte aligned");
  p.kernel = WG_MFMA;
  p.generic = (a.C % epc) != 0 || (a.ldx % epc) != 0;
  p.bm = a.Co <= 64 ? 64 : 128; p.bn = p.generic ? 64 : 128;
  p.tiles = cdiv(a.Co, p.bm) * cdiv(Ncol, p.bn);
  return p;
}
