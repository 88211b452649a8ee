// Sliding-window inference kernels (see window.h).
//
// The decision head has tta.hip's shape with one more level of geometry: one thread per output
// pixel, which selects a canvas pixel (Y, X); the windows that cover it are rows iy0..iy1 of ys
// times columns ix0..ix1 of xs (the origins increase strictly, so both ranges are contiguous),
// found once per pixel; the pixel takes part in the entries of those ranges only. Inside a window
// the local position (Y - y0, X - x0) goes through the calls of decision_head.h that
// tta_decisions_kernel makes (lerp_of, the lerp, the softmax, the sum, the decision), so a canvas
// of the network's size gives seg_tta_decisions' bits. The row lerp depends on iy alone and is
// formed once per row.
// The origin and pointer tables are kernel arguments, and the row and column counters are kept
// uniform over the wave (0..ny, 0..nx with the pixel's range as the predicate) so that the tables
// come by scalar loads: a wave's pixels share Y and cross a window border in X in few waves, so
// nearly every wave skips the rows and columns outside its range with one branch each. Counters
// starting at the pixel's own iy0 / ix0 made the table reads per-lane vector loads in front of
// every entry's cell loads and measured 2 to 7 % slower. The four low-resolution cells of an
// entry are read through L2 as in tta.hip.
#include "window.h"
#include "decision_head.h"

namespace {

using namespace decision_head;

constexpr int WIN_THREADS = 256;

// [first, last] of the origins o[0..n) whose window [o[i], o[i] + len) holds p. The origins
// increase strictly, start at 0, leave no gap and end at canvas - len (checked by the caller), so
// the range is never empty. One pass with a uniform index: the table reads are scalar loads.
__device__ __forceinline__ void covering(const int* o, int n, int len, int p, int& first, int& last) {
  first = 0;
  last = 0;
  for (int i = 0; i < n; ++i) {
    const int oi = o[i];
    if (oi + len <= p && i + 1 < n) first = i + 1;
    if (oi <= p) last = i;
  }
}

template <int C1, int C2, int C3>
__global__ __launch_bounds__(WIN_THREADS) void window_decisions_kernel(WinArgs a, LossTables t) {
  constexpr int CT = C1 + C2 + C3;
  const long total = (long)a.N * a.Ho * a.Wo;
  const int per = 1 + a.flip;
  const size_t image = (size_t)a.hl * a.wl * a.ld;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(id % a.Wo);
    const int yo = (int)((id / a.Wo) % a.Ho);
    const int n = (int)(id / ((long)a.Wo * a.Ho));
    const int Y = nn_src(yo, a.Hc, a.Ho), X = nn_src(xo, a.Wc, a.Wo);
    int iy0, iy1, ix0, ix1;
    covering(a.ys, a.ny, a.H, Y, iy0, iy1);
    covering(a.xs, a.nx, a.W, X, ix0, ix1);
    float acc[CT];   // the sum of the covering entries' p in entry order, starting from the first
    int k = 0;       // covering entries so far
    // The loop counters are uniform over the wave (origins and pointers come by scalar loads);
    // a pixel takes part in the rows and columns of its own ranges only, and a row or column no
    // pixel of the wave is in costs the wave one branch.
    for (int iy = 0; iy < a.ny; ++iy) {
      if (iy < iy0 || iy > iy1) continue;
      int ylo, yhi;
      float yl;
      lerp_of(Y - a.ys[iy], a.hl, a.H, ylo, yhi, yl);
      for (int ix = 0; ix < a.nx; ++ix) {
        if (ix < ix0 || ix > ix1) continue;
        const int x = X - a.xs[ix];
        for (int f = 0; f < per; ++f) {
          int xlo, xhi;
          float xl;
          lerp_of(f ? a.W - 1 - x : x, a.wl, a.W, xlo, xhi, xl);
          const float* base = a.logits[(iy * a.nx + ix) * per + f] + (size_t)n * image;
          float p[CT];
          bilerp<CT>(p, cells_of(base, ylo, yhi, xlo, xhi, a.wl, a.ld), xl, yl);
          softmax_heads<C1, C2, C3>(p);
          accumulate<CT>(acc, p, k == 0);
          ++k;
        }
      }
    }
    // Ho x Wo = Hc x Wc (checked by the caller): id is the canvas pixel
    if (a.probs) store_ct<CT>(a.probs + (size_t)id * CT, acc, a.rk[k]);
    a.out[id] = decide<C1, C2, C3>(acc, t, a.map, a.replace_voids);
  }
}

// out[b][y][x][c] = in[b][y0 + y][x0 + (flip ? W - 1 - x : x)][c]: a copy
__global__ __launch_bounds__(WIN_THREADS) void window_images_kernel(
    const float* __restrict__ in, int n, int Hc, int Wc, int y0, int x0, int H, int W, int flip,
    float* __restrict__ out) {
  const long total = (long)n * H * W;
  for (long id = (long)blockIdx.x * WIN_THREADS + threadIdx.x; id < total;
       id += (long)gridDim.x * WIN_THREADS) {
    const int x = (int)(id % W);
    const int y = (int)((id / W) % H);
    const int b = (int)(id / ((long)W * H));
    const float* src = in + (((size_t)b * Hc + (y0 + y)) * Wc + (x0 + (flip ? W - 1 - x : x))) * 3;
    float* o = out + id * 3;
    o[0] = src[0];
    o[1] = src[1];
    o[2] = src[2];
  }
}

}  // namespace

hipError_t launch_window_images(const float* in, int n, int Hc, int Wc, int y0, int x0, int H,
                                int W, int flip, float* out, hipStream_t s) {
  const long total = (long)n * H * W;
  if (total <= 0) return hipSuccess;
  long g = (total + WIN_THREADS - 1) / WIN_THREADS;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(window_images_kernel, dim3((unsigned)g), dim3(WIN_THREADS), 0, s, in, n, Hc,
                     Wc, y0, x0, H, W, flip, out);
  return hipGetLastError();
}

hipError_t launch_window_decisions(const WinArgs& a, const LossTables& t, hipStream_t s) {
  const long total = (long)a.N * a.Ho * a.Wo;
  if (total <= 0) return hipSuccess;
  const dim3 g((unsigned)std::min((total + WIN_THREADS - 1) / WIN_THREADS, 8192L));
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    hipLaunchKernelGGL((window_decisions_kernel<c1, c2, c3>), g, dim3(WIN_THREADS), 0, s, a, t);
  });
}
