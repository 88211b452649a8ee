// The per-pixel decision head of the four inference kernels (eval_decisions_kernel and
// full_predictions_kernel in decide.hip, tta_decisions_kernel, window_decisions_kernel): the
// align-corners upsampling of the low-resolution logits, the per-head softmax, the first-maximum
// argmax, the hierarchical fusion and the void replacement, each expression once. The kernels keep
// their own loops and geometry and call these.
//
// The rounding is stated here and not left to the compiler's contraction: every fused
// multiply-add is an explicit __fmaf_rn (in_f - lo as fma(o, scale, -lo), each lerp one fma) and
// sums of rounded products go through __fadd_rn, so that one unflipped entry / one window gives
// seg_full_predictions' bits whatever loop surrounds the call (and seg_predict's decisions:
// decide.hip says where that kernel's weights keep an older rounding, an ulp apart). The training
// kernels of loss.hip keep their own lerp_of under the default contraction and do not include this.
// Include it only where the default contraction holds (in tta.hip: above the image pyramid's
// #pragma clang fp contract(off)).
#pragma once
#include <algorithm>
#include <type_traits>

#include "loss.h"

namespace decision_head {

// TF ResizeBilinear legacy scaler, align_corners=True
__device__ __forceinline__ void lerp_of(int o, int n_in, int n_out, int& lo, int& hi, float& l) {
  const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
  const float fin = (float)o * scale;
  lo = (int)fin;
  hi = lo + 1 < n_in - 1 ? lo + 1 : n_in - 1;
  l = __fmaf_rn((float)o, scale, -(float)lo);   // fin - (float)lo as one fma
}

// TF 1.12 ResizeNearestNeighbor(align_corners=True) source index (legacy scaler, roundf)
__device__ __forceinline__ int nn_src(int o, int n_in, int n_out) {
  const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : (float)n_in / (float)n_out;
  const int i = (int)roundf((float)o * scale);
  return i < n_in - 1 ? i : n_in - 1;
}

// the four cells of a bilinear footprint in one image [rows][wl][ld]
struct Cells {
  const float *tl, *tr, *bl, *br;
};

__device__ __forceinline__ Cells cells_of(const float* image, int ylo, int yhi, int xlo, int xhi,
                                          int wl, int ld) {
  return Cells{image + ((size_t)ylo * wl + xlo) * ld, image + ((size_t)ylo * wl + xhi) * ld,
               image + ((size_t)yhi * wl + xlo) * ld, image + ((size_t)yhi * wl + xhi) * ld};
}

// top = tl + (tr - tl) * xl; bot likewise; top + (bot - top) * yl, one fma each
__device__ __forceinline__ float bilerp1(float tl, float tr, float bl, float br, float xl, float yl) {
  const float top = __fmaf_rn(tr - tl, xl, tl);
  const float bot = __fmaf_rn(br - bl, xl, bl);
  return __fmaf_rn(bot - top, yl, top);
}

template <int N>
__device__ __forceinline__ void bilerp(float* p, const Cells& k, float xl, float yl) {
#pragma unroll
  for (int c = 0; c < N; ++c) p[c] = bilerp1(k.tl[c], k.tr[c], k.bl[c], k.br[c], xl, yl);
}

// softmax of N values in place (the loss head's arithmetic: max, __expf, sum, one reciprocal)
template <int N>
__device__ __forceinline__ void softmax(float* p) {
  float m = p[0];
#pragma unroll
  for (int c = 1; c < N; ++c) m = fmaxf(m, p[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < N; ++c) { p[c] = __expf(p[c] - m); s += p[c]; }
  const float rs = 1.f / s;
#pragma unroll
  for (int c = 0; c < N; ++c) p[c] = p[c] * rs;
}

template <int C1, int C2, int C3>
__device__ __forceinline__ void softmax_heads(float* p) {
  softmax<C1>(p);
  softmax<C2>(p + C1);
  softmax<C3>(p + C1 + C2);
}

// acc = p for the first entry, then acc + p: the rounded p is added, not an FMA of its last multiply
template <int N>
__device__ __forceinline__ void accumulate(float* acc, const float* p, bool first) {
  if (first) {
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] = p[c];
  } else {
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] = __fadd_rn(acc[c], p[c]);
  }
}

// tf.argmax: first maximum
template <int N>
__device__ __forceinline__ int argmax_first(const float* v) {
  int b = 0;
  float bv = v[0];
#pragma unroll
  for (int c = 1; c < N; ++c) if (v[c] > bv) { bv = v[c]; b = c; }
  return b;
}

// hierarchical fusion in common cids: the vehicle / human head decides where l1 says so
template <int C1, int C2, int C3>
__device__ __forceinline__ int fuse_decision(const float* v, const LossTables& t, int d1) {
  if (d1 == t.cid_l1_vehicle) return t.veh_to_common[argmax_first<C2>(v + C1)];
  if (d1 == t.cid_l1_human) return t.hum_to_common[argmax_first<C3>(v + C1 + C2)];
  return t.l1_to_common[d1];
}

// second of top_k(l1, 2) given the first, d1 (stable: equal values keep the lower index first);
// l1 keeps C1 channels (the segment-sum remap does not apply to it)
template <int C1>
__device__ __forceinline__ int second_best(const float* v, int d1) {
  int d2 = -1;
  float b2 = 0.f;
#pragma unroll
  for (int c = 0; c < C1; ++c)
    if (c != d1 && (d2 < 0 || v[c] > b2)) { b2 = v[c]; d2 = c; }
  return d2;
}

// fused decision -> tf.gather(ocids2ncids, decs) -> with eval_voids the EVAL-order void
// replacement (_replace_voids before the resize: void = C1 - 1 takes the second-best l1 class).
// v are probabilities or sums of them (a positive common factor changes no order).
template <int C1, int C2, int C3>
__device__ __forceinline__ int decide(const float* v, const LossTables& t, const int* map,
                                      bool eval_voids) {
  const int d1 = argmax_first<C1>(v);
  const int d = map[fuse_decision<C1, C2, C3>(v, t, d1)];
  if (!eval_voids) return d;
  return d == C1 - 1 ? second_best<C1>(v, d1) : d1;
}

// dst[0..CT) = v * scale (float4 stores where CT % 4 == 0; dst 16-byte aligned then)
template <int CT>
__device__ __forceinline__ void store_ct(float* dst, const float* v, float scale) {
  if constexpr (CT % 4 == 0) {
#pragma unroll
    for (int c = 0; c < CT; c += 4)
      *reinterpret_cast<float4*>(dst + c) =
          make_float4(v[c] * scale, v[c + 1] * scale, v[c + 2] * scale, v[c + 3] * scale);
  } else {
#pragma unroll
    for (int c = 0; c < CT; ++c) dst[c] = v[c] * scale;
  }
}

// f(std::integral_constant c1, c2, c3) for the head widths of t; any other widths are an error
template <class F>
inline hipError_t dispatch_heads(const LossTables& t, F f) {
  if (t.c1 == 14 && t.c2 == 7 && t.c3 == 3)
    f(std::integral_constant<int, 14>{}, std::integral_constant<int, 7>{}, std::integral_constant<int, 3>{});
  else if (t.c1 == 53 && t.c2 == 12 && t.c3 == 5)
    f(std::integral_constant<int, 53>{}, std::integral_constant<int, 12>{}, std::integral_constant<int, 5>{});
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace decision_head
