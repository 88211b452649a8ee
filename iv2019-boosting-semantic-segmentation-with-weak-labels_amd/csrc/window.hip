// Sliding-window inference kernels (see window.h).
//
// The decision head is tta.hip's with one more level of geometry: one thread per output pixel,
// which selects a canvas pixel (Y, X); the windows that cover it are rows iy0..iy1 of ys times
// columns ix0..ix1 of xs (the origins increase strictly, so both ranges are contiguous), found
// once per pixel; the pixel takes part in the entries of those ranges only. Inside a window the
// local position (Y - y0, X - x0) goes through lerp_of, the top / bot lerp and the softmax exactly
// as tta_decisions_kernel writes them (the same explicit fused multiply-adds, see the head of
// tta.hip), so a canvas of the network's size gives seg_tta_decisions' bits. The row lerp depends
// on iy alone and is formed once per row.
// The origin and pointer tables are kernel arguments, and the row and column counters are kept
// uniform over the wave (0..ny, 0..nx with the pixel's range as the predicate) so that the tables
// come by scalar loads: a wave's pixels share Y and cross a window border in X in few waves, so
// nearly every wave skips the rows and columns outside its range with one branch each. Counters
// starting at the pixel's own iy0 / ix0 made the table reads per-lane vector loads in front of
// every entry's cell loads and measured 2 to 7 % slower. The four low-resolution cells of an
// entry are read through L2 as in tta.hip.
#include "window.h"

namespace {

constexpr int WIN_THREADS = 256;

__device__ __forceinline__ void lerp_of(int o, int n_in, int n_out, int& lo, int& hi, float& l) {
  // TF ResizeBilinear legacy scaler, align_corners=True (tta.hip's, bit for bit)
  const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
  const float fin = (float)o * scale;
  lo = (int)fin;
  hi = lo + 1 < n_in - 1 ? lo + 1 : n_in - 1;
  l = __fmaf_rn((float)o, scale, -(float)lo);   // fin - (float)lo, contracted as in loss.hip
}

// TF 1.12 ResizeNearestNeighbor(align_corners=True) source index (legacy scaler, roundf)
__device__ __forceinline__ int nn_src(int o, int n_in, int n_out) {
  const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : (float)n_in / (float)n_out;
  const int i = (int)roundf((float)o * scale);
  return i < n_in - 1 ? i : n_in - 1;
}

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
          const float* tl = base + ((size_t)ylo * a.wl + xlo) * a.ld;
          const float* tr = base + ((size_t)ylo * a.wl + xhi) * a.ld;
          const float* bl = base + ((size_t)yhi * a.wl + xlo) * a.ld;
          const float* br = base + ((size_t)yhi * a.wl + xhi) * a.ld;
          float p[CT];
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            // top = tl + (tr - tl) * xl; bot likewise; top + (bot - top) * yl, one fma each
            const float top = __fmaf_rn(tr[c] - tl[c], xl, tl[c]);
            const float bot = __fmaf_rn(br[c] - bl[c], xl, bl[c]);
            p[c] = __fmaf_rn(bot - top, yl, top);
          }
          // softmax per head (the same arithmetic as the loss head and the eval kernel)
          auto softmax = [&](int c0, int nc) {
            float m = p[c0];
#pragma unroll
            for (int c = 1; c < nc; ++c) m = fmaxf(m, p[c0 + c]);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < nc; ++c) { p[c0 + c] = __expf(p[c0 + c] - m); s += p[c0 + c]; }
            const float rs = 1.f / s;
#pragma unroll
            for (int c = 0; c < nc; ++c) p[c0 + c] = p[c0 + c] * rs;
          };
          softmax(0, C1);
          softmax(C1, C2);
          softmax(C1 + C2, C3);
          if (k == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = p[c];
          } else {
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = __fadd_rn(acc[c], p[c]);   // the rounded p, not an FMA
          }
          ++k;
        }
      }
    }
    if (a.probs) {   // Ho x Wo = Hc x Wc (checked by the caller): id is the canvas pixel
      const float r = a.rk[k];
      float* o = a.probs + (size_t)id * CT;
      if constexpr (CT % 4 == 0) {
#pragma unroll
        for (int c = 0; c < CT; c += 4)
          *reinterpret_cast<float4*>(o + c) = make_float4(acc[c] * r, acc[c + 1] * r,
                                                          acc[c + 2] * r, acc[c + 3] * r);
      } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) o[c] = acc[c] * r;
      }
    }
    // the eval kernel's decision logic on the sums (a positive common factor changes no order)
    int d1 = 0;
    float b1 = acc[0];
#pragma unroll
    for (int c = 1; c < C1; ++c) if (acc[c] > b1) { b1 = acc[c]; d1 = c; }
    int d;
    if (d1 == t.cid_l1_vehicle) {
      int b = 0;
      float bv = acc[C1];
#pragma unroll
      for (int c = 1; c < C2; ++c) if (acc[C1 + c] > bv) { bv = acc[C1 + c]; b = c; }
      d = t.veh_to_common[b];
    } else if (d1 == t.cid_l1_human) {
      int b = 0;
      float bv = acc[C1 + C2];
#pragma unroll
      for (int c = 1; c < C3; ++c) if (acc[C1 + C2 + c] > bv) { bv = acc[C1 + C2 + c]; b = c; }
      d = t.hum_to_common[b];
    } else {
      d = t.l1_to_common[d1];
    }
    d = a.map[d];   // tf.gather(ocids2ncids, decs)
    if (a.replace_voids) {
      // top_k(l1 sums, 2) (stable: equal values keep the lower index first)
      int d2 = -1;
      float b2 = 0.f;
#pragma unroll
      for (int c = 0; c < C1; ++c)
        if (c != d1 && (d2 < 0 || acc[c] > b2)) { b2 = acc[c]; d2 = c; }
      d = d == C1 - 1 ? d2 : d1;
    }
    a.out[id] = d;
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
  long g = (total + WIN_THREADS - 1) / WIN_THREADS;
  if (g > 8192) g = 8192;
  if (t.c1 == 14 && t.c2 == 7 && t.c3 == 3)
    hipLaunchKernelGGL((window_decisions_kernel<14, 7, 3>), dim3((int)g), dim3(WIN_THREADS), 0, s, a, t);
  else if (t.c1 == 53 && t.c2 == 12 && t.c3 == 5)
    hipLaunchKernelGGL((window_decisions_kernel<53, 12, 5>), dim3((int)g), dim3(WIN_THREADS), 0, s, a, t);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
