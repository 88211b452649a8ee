// Boundary-band kernels (see boundary.h; semantics in include/seg_hip.h at seg_boundary_distance).
//
// Row pass: a block owns BR_ROWS rows x BR_CORE 64-column words of one image (blockIdx.z) plus one
// word of halo on either side (wmax <= 64 columns). A wave forms the boundary flags of one word as
// a ballot; then every thread takes four consecutive pixels and reads the distance to the nearest
// flag on either side off the pixel's own word and its two neighbours with a count of leading /
// trailing zeros. Bits outside the image are never set, so the image edge needs no case.
//
// Column pass: a block owns a BC_TY x BC_TX tile of one image and stages g for the tile and wmax
// rows above and below it in LDS; rows outside the image are filled with the cap wmax + 1, whose
// square is already beyond every band. A lane owns a column, a wave every fourth row. The distance
// kernel stores min(d2, wmax^2 + 1); the band kernel looks up the smallest band that holds the
// pixel, reads the label and the decision of band pixels only, and adds one count -- in a histogram
// private to the block where K * nc * nc ints fit beside the tile (Cityscapes), in memory otherwise
// (Vistas with four or more widths), as launch_confusion does.
#include "boundary.h"

namespace {

constexpr int BR_THREADS = 256;
constexpr int BR_ROWS = 2;
constexpr int BR_CORE = 16;             // words (of 64 columns) a block writes g for, per row
constexpr int BR_WORDS = BR_CORE + 2;   // ... and forms flags for

constexpr int BC_THREADS = 256;
constexpr int BC_TX = 64, BC_TY = 64;
constexpr size_t BC_LDS_LIMIT = 64 * 1024;

typedef unsigned long long u64;

__device__ __forceinline__ bool counted(int l, int nc, int ignore) {
  return (unsigned)l < (unsigned)nc && l != ignore;
}

// distance from bit b of m[0] to the nearest set bit of m[-1], m[0], m[1] (bit i of m[j] is
// column 64 j + i), at most cap
__device__ __forceinline__ int row_distance(const u64* m, int b, int cap) {
  const u64 right = m[0] >> b;
  const int dr = right ? __builtin_ctzll(right) : (m[1] ? 64 - b + __builtin_ctzll(m[1]) : cap);
  const u64 left = m[0] << (63 - b);
  const int dl = left ? __builtin_clzll(left) : (m[-1] ? b + 1 + __builtin_clzll(m[-1]) : cap);
  return min(min(dl, dr), cap);
}

template <bool VEC4>
__global__ __launch_bounds__(BR_THREADS) void boundary_rows_kernel(BoundaryRowArgs a) {
  __shared__ u64 masks[BR_ROWS][BR_WORDS];
  const int img = blockIdx.z;
  const int y0 = blockIdx.y * BR_ROWS;
  const int w0 = blockIdx.x * BR_CORE;   // first core word
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* lab = a.labels + (size_t)img * a.H * a.W;
  for (int i = wave; i < BR_ROWS * BR_WORDS; i += BR_THREADS / 64) {
    const int r = i / BR_WORDS, j = i - r * BR_WORDS;
    const int y = y0 + r, word = w0 - 1 + j;
    const int x = word * 64 + lane;
    bool flag = false;
    if (y < a.H && word >= 0 && x < a.W) {
      const int* row = lab + (size_t)y * a.W;
      const int l = row[x];
      if (counted(l, a.nc, a.ignore)) {
        int o;
        if (x > 0) { o = row[x - 1]; flag |= o != l && counted(o, a.nc, a.ignore); }
        if (x + 1 < a.W) { o = row[x + 1]; flag |= o != l && counted(o, a.nc, a.ignore); }
        if (y > 0) { o = row[x - a.W]; flag |= o != l && counted(o, a.nc, a.ignore); }
        if (y + 1 < a.H) { o = row[x + a.W]; flag |= o != l && counted(o, a.nc, a.ignore); }
      }
    }
    const u64 m = __ballot(flag);   // every lane of the wave is here: i depends on the wave only
    if (lane == 0) masks[r][j] = m;
  }
  __syncthreads();
  const int cap = a.wmax + 1;
  constexpr int GROUPS = BR_CORE * 64 / 4;   // groups of four pixels per row
  for (int q = threadIdx.x; q < BR_ROWS * GROUPS; q += BR_THREADS) {
    const int r = q / GROUPS, c = (q - r * GROUPS) * 4;   // column within the core
    const int y = y0 + r, x = w0 * 64 + c;
    if (y >= a.H || x >= a.W) continue;
    const u64* m = &masks[r][1 + (c >> 6)];
    uint8_t* out = a.g + ((size_t)img * a.H + y) * a.W + x;
    const int b = c & 63;   // b + 3 <= 63: the four pixels share a word
    if constexpr (VEC4) {   // W % 4 == 0 and g 4-byte aligned: the four pixels exist and line up
      const uchar4 v = make_uchar4((unsigned char)row_distance(m, b, cap), (unsigned char)row_distance(m, b + 1, cap),
                                   (unsigned char)row_distance(m, b + 2, cap), (unsigned char)row_distance(m, b + 3, cap));
      *reinterpret_cast<uchar4*>(out) = v;
    } else {
      for (int u = 0; u < 4 && x + u < a.W; ++u) out[u] = (uint8_t)row_distance(m, b + u, cap);
    }
  }
}

// MODE 0: distance; 1: band confusion into a private histogram; 2: band confusion into memory
template <int MODE, bool VEC4>
__global__ __launch_bounds__(BC_THREADS) void boundary_cols_kernel(BoundaryColArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int ncell = MODE == 1 ? a.K * a.nc * a.nc : 0;
  int* hist = reinterpret_cast<int*>(smem);
  uint8_t* tile = smem + (size_t)ncell * sizeof(int);   // [BC_TY + 2 wmax][BC_TX]
  const int img = blockIdx.z;
  const int y0 = blockIdx.y * BC_TY, x0 = blockIdx.x * BC_TX;
  const int wmax = a.wmax, rows = BC_TY + 2 * wmax, cap = wmax + 1;
  const uint8_t* g = a.g + (size_t)img * a.H * a.W;
  if constexpr (MODE == 1)
    for (int i = threadIdx.x; i < ncell; i += BC_THREADS) hist[i] = 0;
  if constexpr (VEC4) {   // W % 4 == 0 and g 4-byte aligned
    const int c = (threadIdx.x & 15) * 4;
    for (int rr = threadIdx.x >> 4; rr < rows; rr += BC_THREADS / 16) {
      const int y = y0 - wmax + rr, x = x0 + c;
      unsigned v = 0x01010101u * (unsigned)cap;
      if (y >= 0 && y < a.H && x < a.W) v = *reinterpret_cast<const unsigned*>(g + (size_t)y * a.W + x);
      *reinterpret_cast<unsigned*>(tile + rr * BC_TX + c) = v;
    }
  } else {
    const int c = threadIdx.x & 63;
    for (int rr = threadIdx.x >> 6; rr < rows; rr += BC_THREADS / 64) {
      const int y = y0 - wmax + rr, x = x0 + c;
      tile[rr * BC_TX + c] = (y >= 0 && y < a.H && x < a.W) ? g[(size_t)y * a.W + x] : (uint8_t)cap;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int x = x0 + lane;
  const int d2cap = wmax * wmax + 1;
  if (x < a.W) {
    for (int r = threadIdx.x >> 6; r < BC_TY && y0 + r < a.H; r += BC_THREADS / 64) {
      const uint8_t* col = tile + r * BC_TX + lane;   // row y - wmax of the tile
      int best = d2cap;
#pragma unroll 4
      for (int i = 0; i <= 2 * wmax; ++i) {
        const int dy = i - wmax, gg = col[i * BC_TX];
        best = min(best, dy * dy + gg * gg);
      }
      const size_t p = ((size_t)img * a.H + (y0 + r)) * a.W + x;
      if constexpr (MODE == 0) {
        a.d2[p] = (uint16_t)best;
      } else {
        // w2 is increasing and INT_MAX from K on: the bands that miss the pixel come first
        int k = 0;
#pragma unroll
        for (int j = 0; j < BOUNDARY_MAX_WIDTHS; ++j) k += best > a.w2[j];
        if (k >= a.K) continue;   // outside the widest band: neither label nor decision is read
        const int l = a.labels[p], d = a.decisions[p];
        if ((unsigned)l < (unsigned)a.nc && (unsigned)d < (unsigned)a.nc)
          atomicAdd(&(MODE == 1 ? hist : a.cm)[((size_t)k * a.nc + l) * a.nc + d], 1);
      }
    }
  }
  if constexpr (MODE == 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncell; i += BC_THREADS)
      if (hist[i]) atomicAdd(&a.cm[i], hist[i]);
  }
}

__global__ __launch_bounds__(256) void band_finalize_kernel(int* cm, int K, int cells) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  int run = 0;
  for (int k = 0; k < K; ++k) {
    run += cm[(size_t)k * cells + i];
    cm[(size_t)k * cells + i] = run;
  }
}

bool good_size(int N, int H, int W, int wmax) {
  return N >= 1 && N <= BOUNDARY_MAX_IMAGES && H >= 1 && W >= 1 && W <= (1 << 30) && wmax >= 1 && wmax <= BOUNDARY_MAX_WIDTH &&
         (H + BC_TY - 1) / BC_TY <= 65535 && (H + BR_ROWS - 1) / BR_ROWS <= 65535;
}

bool vec4_ok(const void* g, int W) { return W % 4 == 0 && ((uintptr_t)g & 3) == 0; }

dim3 cols_grid(const BoundaryColArgs& a) {
  return dim3((unsigned)((a.W + BC_TX - 1) / BC_TX), (unsigned)((a.H + BC_TY - 1) / BC_TY), (unsigned)a.N);
}

}  // namespace

size_t boundary_tile_bytes(int wmax) { return (size_t)(BC_TY + 2 * wmax) * BC_TX; }

bool boundary_hist_in_lds(int wmax, int K, int nc) {
  return (size_t)K * nc * nc * sizeof(int) + boundary_tile_bytes(wmax) <= BC_LDS_LIMIT;
}

hipError_t launch_boundary_rows(const BoundaryRowArgs& a, hipStream_t s) {
  if (!good_size(a.N, a.H, a.W, a.wmax) || !a.labels || !a.g) return hipErrorInvalidValue;
  const int words = (a.W + 63) / 64;
  const dim3 grid((unsigned)((words + BR_CORE - 1) / BR_CORE), (unsigned)((a.H + BR_ROWS - 1) / BR_ROWS),
                  (unsigned)a.N);
  if (vec4_ok(a.g, a.W))
    hipLaunchKernelGGL((boundary_rows_kernel<true>), grid, dim3(BR_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((boundary_rows_kernel<false>), grid, dim3(BR_THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_boundary_distance(const BoundaryColArgs& a, hipStream_t s) {
  if (!good_size(a.N, a.H, a.W, a.wmax) || !a.g || !a.d2) return hipErrorInvalidValue;
  const size_t lds = boundary_tile_bytes(a.wmax);
  if (vec4_ok(a.g, a.W))
    hipLaunchKernelGGL((boundary_cols_kernel<0, true>), cols_grid(a), dim3(BC_THREADS), lds, s, a);
  else
    hipLaunchKernelGGL((boundary_cols_kernel<0, false>), cols_grid(a), dim3(BC_THREADS), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_band_confusion(const BoundaryColArgs& a, hipStream_t s) {
  if (!good_size(a.N, a.H, a.W, a.wmax) || !a.g || !a.labels || !a.decisions || !a.cm) return hipErrorInvalidValue;
  if (a.K < 1 || a.K > BOUNDARY_MAX_WIDTHS || a.nc < 1 || a.nc > 256 || a.w2[a.K - 1] != a.wmax * a.wmax)
    return hipErrorInvalidValue;
  for (int k = 1; k < BOUNDARY_MAX_WIDTHS; ++k)   // increasing, INT_MAX from K on (the kernel's lookup)
    if (k < a.K ? a.w2[k] <= a.w2[k - 1] : a.w2[k] != INT_MAX) return hipErrorInvalidValue;
  const bool v = vec4_ok(a.g, a.W);
  if (boundary_hist_in_lds(a.wmax, a.K, a.nc)) {
    const size_t lds = boundary_tile_bytes(a.wmax) + (size_t)a.K * a.nc * a.nc * sizeof(int);
    if (v) hipLaunchKernelGGL((boundary_cols_kernel<1, true>), cols_grid(a), dim3(BC_THREADS), lds, s, a);
    else hipLaunchKernelGGL((boundary_cols_kernel<1, false>), cols_grid(a), dim3(BC_THREADS), lds, s, a);
  } else {
    const size_t lds = boundary_tile_bytes(a.wmax);
    if (v) hipLaunchKernelGGL((boundary_cols_kernel<2, true>), cols_grid(a), dim3(BC_THREADS), lds, s, a);
    else hipLaunchKernelGGL((boundary_cols_kernel<2, false>), cols_grid(a), dim3(BC_THREADS), lds, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_band_finalize(int* cm, int K, int nc, hipStream_t s) {
  if (!cm || K < 1 || K > BOUNDARY_MAX_WIDTHS || nc < 1 || nc > 256) return hipErrorInvalidValue;
  const int cells = nc * nc;
  hipLaunchKernelGGL(band_finalize_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, cm, K, cells);
  return hipGetLastError();
}
