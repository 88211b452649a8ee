// Mean-field CRF kernels (see crf.h).
//
// The step kernel tiles the DILATION LATTICE, not the image: a workgroup owns the pixels
// (ry + d * ly, rx + d * lx) of one residue class (ry, rx) mod d for a TH x TW tile of lattice
// coordinates (ly, lx). The neighbours (dy * d, dx * d) of those pixels are the lattice cells
// (ly + dy, lx + dx), so the staged halo is r lattice cells whatever the dilation (r * d = 20
// pixels costs what r = 5 costs), and every staged cell is read by (2r + 1)^2 - 1 threads. A
// pixel's CT probabilities are contiguous in memory (96 B / 280 B), so a lattice row with d > 1
// still loads whole pixels. Cells outside the image are staged as zeros: k * 0 adds exactly
// nothing to the fp32 message, which is "contributes nothing" without a branch per neighbour.
//
// LDS image: [TH + 2r][TW + 2r] cells of S floats: Q^t (CT), the image (3), padding up to S with
// S / 4 odd, so that the 16 lanes of a tile row, S floats apart, start their 16-byte reads on 16
// different 4-bank slots. A thread forms k_ij once per neighbour from the image part and uses it
// for the CT fused multiply-adds on that cell's probabilities, which it reads as vectors.
// Tile: 16 x 16 where the image fits 160 KiB, else 8 x 16 (Vistas at r >= 4).
#include "crf.h"
#include "decision_head.h"

namespace {

using namespace decision_head;

constexpr size_t CRF_LDS_MAX = 160 * 1024;
constexpr int CRF_DECIDE_THREADS = 256;

// widest vector a pixel's CT floats split into when pixels are CT floats apart and the base is
// 16-byte aligned
constexpr int crf_vec(int ct) { return ct % 4 == 0 ? 4 : ct % 2 == 0 ? 2 : 1; }
// floats per staged cell: CT + 3 rounded up to a multiple of 4 whose quarter is odd
constexpr int crf_stride(int ct) {
  int s = (ct + 3 + 3) / 4 * 4;
  return (s / 4) % 2 ? s : s + 4;
}
constexpr size_t crf_lds(int ct, int r, int th, int tw) {
  return (size_t)(th + 2 * r) * (tw + 2 * r) * crf_stride(ct) * sizeof(float);
}

template <int V> struct VecOf;
template <> struct VecOf<4> { using type = float4; };
template <> struct VecOf<2> { using type = float2; };
template <> struct VecOf<1> { using type = float; };

template <int V>
__device__ __forceinline__ void load_vec(float* dst, const float* src) {
  using T = typename VecOf<V>::type;
  const T v = *reinterpret_cast<const T*>(src);
  if constexpr (V == 4) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; }
  else if constexpr (V == 2) { dst[0] = v.x; dst[1] = v.y; }
  else dst[0] = v;
}

// one head of the update: v = P * exp(m - max m), Q = v / sum v; a sum that is not >= 1e-30f
// (underflow, NaN) keeps P
template <int N>
__device__ __forceinline__ void mean_field_head(float* m, const float* p) {
  float mx = m[0];
#pragma unroll
  for (int c = 1; c < N; ++c) mx = fmaxf(mx, m[c]);
  float z = 0.f;
#pragma unroll
  for (int c = 0; c < N; ++c) { m[c] = p[c] * __expf(m[c] - mx); z += m[c]; }
  if (z >= 1e-30f) {
    const float rz = 1.f / z;
#pragma unroll
    for (int c = 0; c < N; ++c) m[c] = m[c] * rz;
  } else {
#pragma unroll
    for (int c = 0; c < N; ++c) m[c] = p[c];
  }
}

template <int C1, int C2, int C3, int TH, int TW>
__global__ __launch_bounds__(TH * TW) void crf_step_kernel(CrfStepArgs a) {
  constexpr int CT = C1 + C2 + C3;
  constexpr int V = crf_vec(CT);
  constexpr int U = CT / V;            // vectors per pixel
  constexpr int S = crf_stride(CT);
  constexpr int THREADS = TH * TW;
  using Vec = typename VecOf<V>::type;
  extern __shared__ float4 crf_lds4[];
  float* lds = reinterpret_cast<float*>(crf_lds4);

  const int r = a.r, d = a.d;
  const int CH = TH + 2 * r, CW = TW + 2 * r;
  const int HL = (a.H + d - 1) / d, WL = (a.W + d - 1) / d;   // lattice size of class (0, 0)
  const int tiles_x = (WL + TW - 1) / TW, tiles_y = (HL + TH - 1) / TH;
  int b = blockIdx.x;
  const int lx0 = (b % tiles_x) * TW; b /= tiles_x;
  const int ly0 = (b % tiles_y) * TH; b /= tiles_y;
  const int rx = b % d; b /= d;
  const int ry = b % d;
  const int n = b / d;
  const size_t px0 = (size_t)n * a.H * a.W;

  // stage Q^t and the image: any halo size, any tile size (the loops run over the cells, not the
  // threads). STAGE loads are issued before their LDS stores so that a thread has that many in
  // flight, not one; cell / CW in float is exact here (cell < 2^11, and (cell + 0.5) / CW is at
  // least 0.5 / 26 away from an integer).
  constexpr int STAGE = 4;
  const float inv_cw = 1.f / (float)CW;
  const int cells = CH * CW;
  auto pixel_of = [&](int cell) -> long {   // the pixel's index in the image, or -1 outside
    const int cy = (int)(((float)cell + 0.5f) * inv_cw), cx = cell - cy * CW;
    const int y = ry + d * (ly0 + cy - r), x = rx + d * (lx0 + cx - r);
    return (y >= 0 && y < a.H && x >= 0 && x < a.W) ? (long)y * a.W + x : -1;
  };
  for (int i0 = threadIdx.x; i0 < cells * U; i0 += THREADS * STAGE) {
    Vec v[STAGE];
    int at[STAGE];
#pragma unroll
    for (int b = 0; b < STAGE; ++b) {
      const int i = i0 + b * THREADS;
      v[b] = Vec{};
      at[b] = -1;
      if (i < cells * U) {
        const int cell = i / U, u = i - cell * U;
        at[b] = cell * S + u * V;
        const long px = pixel_of(cell);
        if (px >= 0) v[b] = *reinterpret_cast<const Vec*>(a.q + (px0 + px) * CT + u * V);
      }
    }
#pragma unroll
    for (int b = 0; b < STAGE; ++b)
      if (at[b] >= 0) *reinterpret_cast<Vec*>(lds + at[b]) = v[b];
  }
  for (int i0 = threadIdx.x; i0 < cells * 3; i0 += THREADS * STAGE) {
    float v[STAGE];
    int at[STAGE];
#pragma unroll
    for (int b = 0; b < STAGE; ++b) {
      const int i = i0 + b * THREADS;
      v[b] = 0.f;
      at[b] = -1;
      if (i < cells * 3) {
        const int cell = i / 3, c = i - cell * 3;
        at[b] = cell * S + CT + c;
        const long px = pixel_of(cell);
        if (px >= 0) v[b] = a.img[(px0 + px) * 3 + c];
      }
    }
#pragma unroll
    for (int b = 0; b < STAGE; ++b)
      if (at[b] >= 0) lds[at[b]] = v[b];
  }
  __syncthreads();

  const int ty = threadIdx.x / TW, tx = threadIdx.x - ty * TW;
  const int y = ry + d * (ly0 + ty), x = rx + d * (lx0 + tx);
  if (y >= a.H || x >= a.W) return;   // no barrier below

  const float* ctr = lds + ((ty + r) * CW + tx + r) * S;
  const float i0 = ctr[CT], i1 = ctr[CT + 1], i2 = ctr[CT + 2];
  float m[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) m[c] = 0.f;
  // One row of the neighbourhood at a time, the row's 2r + 1 cells unrolled (r is 1..5: five
  // bodies), so that the LDS reads of several neighbours are in flight together instead of one
  // neighbour's round trips in a chain. The centre runs with the others: its table entries are 0,
  // k = 0, and 0 * Q adds exactly nothing.
  auto rows = [&](auto rw) {
    constexpr int RW = decltype(rw)::value, R = RW / 2;
    int o = 0;
    for (int dy = -R; dy <= R; ++dy) {
      const float* row = ctr + (dy * CW - R) * S;
#pragma unroll
      for (int j = 0; j < RW; ++j, ++o) {
        const float* nb = row + j * S;
        const float e0 = i0 - nb[CT], e1 = i1 - nb[CT + 1], e2 = i2 - nb[CT + 2];
        const float dist = e0 * e0 + e1 * e1 + e2 * e2;
        const float k = __fmaf_rn(a.ga[o], __expf(-dist * a.inv2b), a.gs[o]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float q[V];
          load_vec<V>(q, nb + u * V);
#pragma unroll
          for (int v = 0; v < V; ++v) m[u * V + v] = __fmaf_rn(k, q[v], m[u * V + v]);
        }
      }
    }
  };
  switch (r) {
    case 1: rows(std::integral_constant<int, 3>{}); break;
    case 2: rows(std::integral_constant<int, 5>{}); break;
    case 3: rows(std::integral_constant<int, 7>{}); break;
    case 4: rows(std::integral_constant<int, 9>{}); break;
    default: rows(std::integral_constant<int, 11>{}); break;
  }

  const size_t px = px0 + (size_t)y * a.W + x;
  {
    float p[CT];
#pragma unroll
    for (int u = 0; u < U; ++u) load_vec<V>(p + u * V, a.p + px * CT + u * V);
    mean_field_head<C1>(m, p);
    mean_field_head<C2>(m + C1, p + C1);
    mean_field_head<C3>(m + C1 + C2, p + C1 + C2);
  }
  store_ct<CT>(a.out + px * CT, m, 1.f);
}

// decisions of a full-resolution probability tensor: the nearest source pixel of every output
// pixel, then the decision head on its CT values
template <int C1, int C2, int C3>
__global__ __launch_bounds__(CRF_DECIDE_THREADS) void crf_decisions_kernel(CrfDecideArgs a, LossTables t) {
  constexpr int CT = C1 + C2 + C3;
  constexpr int V = crf_vec(CT);
  const long total = (long)a.N * a.Ho * a.Wo;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(id % a.Wo);
    const int yo = (int)((id / a.Wo) % a.Ho);
    const int n = (int)(id / ((long)a.Wo * a.Ho));
    const int h = nn_src(yo, a.H, a.Ho), w = nn_src(xo, a.W, a.Wo);
    const float* src = a.q + (((size_t)n * a.H + h) * a.W + w) * CT;
    float v[CT];
#pragma unroll
    for (int u = 0; u < CT / V; ++u) load_vec<V>(v + u * V, src + u * V);
    a.out[id] = decide<C1, C2, C3>(v, t, a.map, a.replace_voids);
  }
}

template <int C1, int C2, int C3, int TH, int TW>
void launch_step_tile(const CrfStepArgs& a, hipStream_t s) {
  constexpr int CT = C1 + C2 + C3;
  auto kern = crf_step_kernel<C1, C2, C3, TH, TW>;
  const size_t lds = crf_lds(CT, a.r, TH, TW);
  // above 64 KiB the dynamic size has to be allowed per function (no allocation, no sync)
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return;   // the sticky error is what dispatch_heads returns
  const long HL = (a.H + a.d - 1) / a.d, WL = (a.W + a.d - 1) / a.d;
  const long blocks = (long)a.N * a.d * a.d * ((HL + TH - 1) / TH) * ((WL + TW - 1) / TW);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(TH * TW), lds, s, a);
}

// 16 x 16 where it fits the LDS, else 8 x 16
template <int CT>
constexpr bool crf_big_tile(int r) { return crf_lds(CT, r, 16, 16) <= CRF_LDS_MAX; }

}  // namespace

size_t crf_step_lds_bytes(const LossTables& t, int r) {
  size_t bytes = 0;
  (void)decision_head::dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    constexpr int CT = c1 + c2 + c3;
    bytes = crf_big_tile<CT>(r) ? crf_lds(CT, r, 16, 16) : crf_lds(CT, r, 8, 16);
  });
  return bytes;
}

hipError_t launch_crf_step(const CrfStepArgs& a, const LossTables& t, hipStream_t s) {
  if ((long)a.N * a.H * a.W <= 0) return hipSuccess;
  if (a.r < 1 || a.r > CRF_MAX_RADIUS || a.d < 1 || a.d > CRF_MAX_DILATION) return hipErrorInvalidValue;
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    constexpr int CT = c1 + c2 + c3;
    static_assert(crf_lds(CT, CRF_MAX_RADIUS, 8, 16) <= CRF_LDS_MAX, "the small tile must always fit");
    if (crf_big_tile<CT>(a.r)) launch_step_tile<c1, c2, c3, 16, 16>(a, s);
    else launch_step_tile<c1, c2, c3, 8, 16>(a, s);
  });
}

hipError_t launch_crf_decisions(const CrfDecideArgs& a, const LossTables& t, hipStream_t s) {
  const long total = (long)a.N * a.Ho * a.Wo;
  if (total <= 0) return hipSuccess;
  const dim3 g((unsigned)std::min((total + CRF_DECIDE_THREADS - 1) / CRF_DECIDE_THREADS, 8192L));
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    hipLaunchKernelGGL((crf_decisions_kernel<c1, c2, c3>), g, dim3(CRF_DECIDE_THREADS), 0, s, a, t);
  });
}
