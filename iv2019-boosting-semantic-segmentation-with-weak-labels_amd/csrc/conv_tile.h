// Internal to the conv kernel files (conv.hip, conv_v2.hip, conv_pp.hip, wgrad_patch.hip): the
// device-side pieces the tile kernels share, one definition each -- the LDS row swizzle, the
// LDS-DMA issue and its counted wait, the XCD-aware block -> tile map, and the epilogue of the
// 16-bit 16 x 16 MFMA tile kernels (conv_nt_v2_kernel, the patch kernels): the full-tile BN
// partial statistics and the store staged through LDS.
#pragma once
#include "conv.h"

// 128-byte LDS rows of eight 16-B chunks: chunk ch of row `row` sits at chunk swz(row, ch), so
// the 16-lane ds_read_b128 fragment reads are conflict-free
__device__ __forceinline__ int swz(int row, int ch) { return ch ^ ((row >> 1) & 7); }

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else static_assert(N < 0, "unsupported vmcnt");
}

// LDS-DMA: 16 B per lane from `src` to the wave's 1 KB at lds_wave_base (lane order)
__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// XCD-aware bijective remap of a 1-D grid of nwg tiles: blocks are dealt round-robin over the 8
// XCDs; block bid gets a tile from its XCD's contiguous run, so tiles that are neighbours (share
// an operand panel) share an L2
__device__ __forceinline__ int xcd_tile(int bid, int nwg) {
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// ---- epilogue of the 512-thread 16 x 16 x 32 MFMA tile kernels ----
constexpr int EPI_COLS = 64;           // staged-store chunk width (fp32 columns)
constexpr int EPI_LD = EPI_COLS + 4;   // padded fp32 staging row

// where a lane's accumulators acc[FM][FN] (f32x4_t) sit in the block tile: the waves are laid
// out (wm, wn) over wave tiles of WM rows x WN columns; element k of fragment (i, j)
template <int WM, int WN>
struct AccLane {
  int wm, wn, lr, lq;   // wave row / column, lane & 15, lane >> 4
  __device__ __forceinline__ int row(int i, int k) const { return wm * WM + i * 16 + lq * 4 + k; }
  __device__ __forceinline__ int col(int j) const { return wn * WN + j * 16 + lr; }
};

// BN partial statistics of a full tile, one pass over the accumulators: per lane and column,
// (sum, M2) of its 4 * FM rows from (sum, sum of squares); then Chan merges of equal-count groups
// over the lane groups (shfl 16, 32) and the WMW waves (LDS), fixed order. One (sum, M2) per
// tile and column at a.stats (ConvNtPlan::stat_rows). GUARD_CO: the tile may reach past Co.
// Leaves the LDS free (ends with a barrier).
template <int BN, int WMW, bool GUARD_CO, int WM, int WN, int FM, int FN>
__device__ __forceinline__ void tile_stats_full(const ConvArgs& a, const f32x4_t (&acc)[FM][FN], char* smem,
                                                const AccLane<WM, WN>& L, int tile, int n0) {
  float2* red2 = (float2*)smem;     // [WMW][BN] (sum, M2)
  constexpr float NL = (float)(4 * FM);   // rows per lane
  float sj[FN], mj[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    float sm = 0.f, sq = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x = acc[i][j][k];
        sm += x;
        sq = __builtin_fmaf(x, x, sq);
      }
    sj[j] = sm;
    mj[j] = fmaxf(sq - sm * sm * (1.f / NL), 0.f);
  }
  float n = NL;
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {   // lanes holding other rows of the same column
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const float s2 = __shfl_xor(sj[j], o, 64), m2 = __shfl_xor(mj[j], o, 64);
      const float d = (s2 - sj[j]) / n;
      mj[j] = mj[j] + m2 + d * d * (0.5f * n);
      sj[j] += s2;
    }
    n *= 2.f;
  }
  if (L.lq == 0)   // one lane per column after the merges
#pragma unroll
    for (int j = 0; j < FN; ++j) red2[L.wm * BN + L.col(j)] = make_float2(sj[j], mj[j]);
  __syncthreads();
  if (L.wm == 0 && L.lq == 0) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int c = L.col(j);
      float2 t = red2[c];
      float nt = (float)WM;
#pragma unroll
      for (int w = 1; w < WMW; ++w) {
        const float2 u = red2[w * BN + c];
        const float d = u.x / (float)WM - t.x / nt;
        t.y = t.y + u.y + d * d * (nt * (float)WM / (nt + (float)WM));
        t.x += u.x;
        nt += (float)WM;
      }
      if (!GUARD_CO || n0 + c < a.Co)
        *(float2*)(a.stats + 2 * ((size_t)tile * a.Co + n0 + c)) = t;
    }
  }
  __syncthreads();
}

// Coalesced stores of the BM x BN tile: the fp32 accumulators staged through LDS EPI_COLS
// columns at a time, the residuals (a.r, a.r2) added, one 16-byte store per lane and 8 outputs.
// pix(row, m) gives tile row `row`'s output pixel m and whether it exists (a constant true
// costs nothing); GUARD_CO: the tile may reach past Co (Co % 8 == 0 on these paths).
template <typename E, int BM, int BN, bool GUARD_CO, int WM, int WN, int FM, int FN, typename Pix>
__device__ __forceinline__ void tile_store_staged(const ConvArgs& a, const f32x4_t (&acc)[FM][FN], char* smem,
                                                  const AccLane<WM, WN>& L, int n0, Pix pix) {
  float* stage = (float*)smem;
  E* Y = (E*)a.y;
  const E* R1 = (const E*)a.r;
  const E* R2 = (const E*)a.r2;
  const int tid = threadIdx.x;
  const int s_rl = tid >> 3, s_cc = tid & 7;   // store phase: row lane (0..63), 8-col chunk
#pragma unroll
  for (int pass = 0; pass < BN / EPI_COLS; ++pass) {
    const int cbase = pass * EPI_COLS;
    if (L.wn * WN + WN > cbase && L.wn * WN < cbase + EPI_COLS) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int col = L.col(j);
        if (col >= cbase && col < cbase + EPI_COLS) {
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) stage[L.row(i, k) * EPI_LD + (col - cbase)] = acc[i][j][k];
        }
      }
    }
    __syncthreads();
    const int n = n0 + cbase + s_cc * 8;
    if (!GUARD_CO || n < a.Co) {
#pragma unroll
      for (int rr = 0; rr < BM / 64; ++rr) {
        const int row = s_rl + 64 * rr;
        long m;
        if (pix(row, m)) {
          const float* sp = stage + row * EPI_LD + s_cc * 8;
          const float4 v0 = *(const float4*)sp, v1 = *(const float4*)(sp + 4);
          float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
          if (R1) {
            float u[8];
            Vec8<E>::load(R1 + (size_t)m * a.ldr + n, u);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += u[e];
          }
          if (R2) {
            float u[8];
            Vec8<E>::load(R2 + (size_t)m * a.ldr2 + n, u);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += u[e];
          }
          store8_nt(Y + (size_t)m * a.ldy + n, v);
        }
      }
    }
    __syncthreads();
  }
}
