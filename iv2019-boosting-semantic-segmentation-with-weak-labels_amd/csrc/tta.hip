// Test-time augmentation kernels (see tta.h).
//
// The decision head has the eval kernel's shape (loss.hip): one thread per output pixel, the four
// low-resolution cells of each entry read through L2, and a register accumulator of the CT
// probability sums next to the CT live values of the entry being added. lerp_of, nn_src, the
// top / bot lerp and the softmax are loss.hip's, so that one unflipped entry gives the bits
// seg_predict and seg_full_predictions give. The one difference in the text: the fused
// multiply-adds loss.hip gets from the compiler's default contraction (in_f - lo as
// fma(o, scale, -lo), each lerp as one fma; read off full_predictions_kernel's ISA) are written
// out here. Left to the compiler, the entry loop puts o * scale and the subtraction of the row
// weight into different basic blocks, the two are not fused, and the last bits differ.
#include "tta.h"

namespace {

constexpr int TTA_THREADS = 256;

// ---- multi-entry decision head ---------------------------------------------------------

__device__ __forceinline__ void lerp_of(int o, int n_in, int n_out, int& lo, int& hi, float& l) {
  // TF ResizeBilinear legacy scaler, align_corners=True
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

template <int C1, int C2, int C3>
__global__ __launch_bounds__(TTA_THREADS) void tta_decisions_kernel(TtaArgs a, LossTables t) {
  constexpr int CT = C1 + C2 + C3;
  const long total = (long)a.N * a.Ho * a.Wo;
  const float inv_e = a.inv_e;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(id % a.Wo);
    const int yo = (int)((id / a.Wo) % a.Ho);
    const int n = (int)(id / ((long)a.Wo * a.Ho));
    const int h = nn_src(yo, a.H, a.Ho), w = nn_src(xo, a.W, a.Wo);
    float acc[CT];   // p_1 + ... + p_E in entry order, starting from p_1
    for (int e = 0; e < a.n_entries; ++e) {
      const TtaEntry& en = a.e[e];
      int ylo, yhi, xlo, xhi;
      float yl, xl;
      lerp_of(h, en.hl, a.H, ylo, yhi, yl);
      lerp_of(en.flip ? a.W - 1 - w : w, en.wl, a.W, xlo, xhi, xl);
      const float* base = en.logits + (size_t)n * en.hl * en.wl * en.ld;
      const float* tl = base + ((size_t)ylo * en.wl + xlo) * en.ld;
      const float* tr = base + ((size_t)ylo * en.wl + xhi) * en.ld;
      const float* bl = base + ((size_t)yhi * en.wl + xlo) * en.ld;
      const float* br = base + ((size_t)yhi * en.wl + xhi) * en.ld;
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
      if (e == 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = p[c];
      } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = __fadd_rn(acc[c], p[c]);   // the rounded p, not an FMA
      }
    }
    if (a.probs) {   // Ho x Wo = H x W (checked by the caller): id is the network pixel
      float* o = a.probs + (size_t)id * CT;
      if constexpr (CT % 4 == 0) {
#pragma unroll
        for (int c = 0; c < CT; c += 4)
          *reinterpret_cast<float4*>(o + c) = make_float4(acc[c] * inv_e, acc[c + 1] * inv_e,
                                                          acc[c + 2] * inv_e, acc[c + 3] * inv_e);
      } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) o[c] = acc[c] * inv_e;
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

// ---- image pyramid ---------------------------------------------------------------------
// From here to the end of the file every operation rounds on its own, as TF's CPU kernel and
// input.hip do: no FMA contraction, neither in the lerps nor in the index arithmetic (in_f - lo
// must see the rounded in_f). Equal sizes then give lerp weights of exactly 0 and the output is
// the (mirrored) input. The decision head above keeps the default contraction of loss.hip, whose
// bits it reproduces.
#pragma clang fp contract(off)

// TF 1.12 legacy scaler, align_corners = False (input.hip's lerp_legacy)
__device__ __forceinline__ void lerp_legacy(int o, int n_in, float scale, int& lo, int& hi,
                                            float& l) {
  const float fin = (float)o * scale;
  lo = (int)fin;                  // fin >= 0: floor
  hi = lo + 1 < n_in - 1 ? lo + 1 : n_in - 1;
  l = fin - (float)lo;
}

__global__ __launch_bounds__(TTA_THREADS) void resize_images_kernel(
    const float* __restrict__ in, int n, int H, int W, int Ho, int Wo, float sy, float sx, int flip,
    float* __restrict__ out) {
  const long total = (long)n * Ho * Wo;
  for (long id = (long)blockIdx.x * TTA_THREADS + threadIdx.x; id < total;
       id += (long)gridDim.x * TTA_THREADS) {
    const int x = (int)(id % Wo);
    const int y = (int)((id / Wo) % Ho);
    const int b = (int)(id / ((long)Wo * Ho));
    int ylo, yhi, xlo, xhi;
    float yl, xl;
    lerp_legacy(y, H, sy, ylo, yhi, yl);
    lerp_legacy(x, W, sx, xlo, xhi, xl);
    if (flip) { xlo = W - 1 - xlo; xhi = W - 1 - xhi; }   // the mirror, then the resize
    const float* img = in + (size_t)b * H * W * 3;
    const float* tl = img + ((size_t)ylo * W + xlo) * 3;
    const float* tr = img + ((size_t)ylo * W + xhi) * 3;
    const float* bl = img + ((size_t)yhi * W + xlo) * 3;
    const float* br = img + ((size_t)yhi * W + xhi) * 3;
    float* o = out + id * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = tl[c] + (tr[c] - tl[c]) * xl;
      const float bot = bl[c] + (br[c] - bl[c]) * xl;
      o[c] = top + (bot - top) * yl;
    }
  }
}

}  // namespace

hipError_t launch_resize_images(const float* in, int n, int H, int W, int Ho, int Wo, int flip,
                                float* out, hipStream_t s) {
  const long total = (long)n * Ho * Wo;
  if (total <= 0) return hipSuccess;
  long g = (total + TTA_THREADS - 1) / TTA_THREADS;
  if (g > 16384) g = 16384;
  const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;   // host IEEE division
  hipLaunchKernelGGL(resize_images_kernel, dim3((unsigned)g), dim3(TTA_THREADS), 0, s, in, n, H, W,
                     Ho, Wo, sy, sx, flip, out);
  return hipGetLastError();
}

hipError_t launch_tta_decisions(const TtaArgs& a, const LossTables& t, hipStream_t s) {
  const long total = (long)a.N * a.Ho * a.Wo;
  if (total <= 0) return hipSuccess;
  long g = (total + TTA_THREADS - 1) / TTA_THREADS;
  if (g > 8192) g = 8192;
  if (t.c1 == 14 && t.c2 == 7 && t.c3 == 3)
    hipLaunchKernelGGL((tta_decisions_kernel<14, 7, 3>), dim3((int)g), dim3(TTA_THREADS), 0, s, a, t);
  else if (t.c1 == 53 && t.c2 == 12 && t.c3 == 5)
    hipLaunchKernelGGL((tta_decisions_kernel<53, 12, 5>), dim3((int)g), dim3(TTA_THREADS), 0, s, a, t);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
