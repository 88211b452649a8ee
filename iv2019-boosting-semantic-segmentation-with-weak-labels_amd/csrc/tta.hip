// Test-time augmentation kernels (see tta.h).
//
// The decision head has the eval kernel's shape (decide.hip): one thread per output pixel, the
// four low-resolution cells of each entry read through L2, and a register accumulator of the CT
// probability sums next to the CT live values of the entry being added. The arithmetic is
// decision_head.h's, the same calls the eval kernels make, so that one unflipped entry gives
// seg_full_predictions' bits and seg_predict's decisions; its fused multiply-adds are explicit because,
// left to the compiler, the entry loop puts o * scale and the subtraction of the row weight into
// different basic blocks and the two are not fused.
#include "tta.h"
#include "decision_head.h"

namespace {

constexpr int TTA_THREADS = 256;

// ---- multi-entry decision head ---------------------------------------------------------

using namespace decision_head;

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
      float p[CT];
      bilerp<CT>(p, cells_of(base, ylo, yhi, xlo, xhi, en.wl, en.ld), xl, yl);
      softmax_heads<C1, C2, C3>(p);
      accumulate<CT>(acc, p, e == 0);
    }
    // Ho x Wo = H x W (checked by the caller): id is the network pixel
    if (a.probs) store_ct<CT>(a.probs + (size_t)id * CT, acc, inv_e);
    a.out[id] = decide<C1, C2, C3>(acc, t, a.map, a.replace_voids);
  }
}

// ---- image pyramid ---------------------------------------------------------------------
// From here to the end of the file every operation rounds on its own, as TF's CPU kernel and
// input.hip do: no FMA contraction, neither in the lerps nor in the index arithmetic (in_f - lo
// must see the rounded in_f). Equal sizes then give lerp weights of exactly 0 and the output is
// the (mirrored) input. The decision head above, and decision_head.h with it, stay outside this
// pragma: their fused multiply-adds are the explicit ones.
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
  const dim3 g((unsigned)std::min((total + TTA_THREADS - 1) / TTA_THREADS, 8192L));
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    hipLaunchKernelGGL((tta_decisions_kernel<c1, c2, c3>), g, dim3(TTA_THREADS), 0, s, a, t);
  });
}
