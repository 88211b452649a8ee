// Single-forward inference heads (see decide.h): one thread per pixel, the 4 low-resolution
// cells of the bilinear footprint read from HBM / L2 directly (eval is one forward per batch:
// these kernels are ~0.1 % of it). The arithmetic is decision_head.h's, but for the weights
// lerp_of_rounded forms in the eval kernel.
#include "decide.h"
#include "decision_head.h"

namespace {

using namespace decision_head;

// lerp_of with the weight formed from the rounded product: in_f = o * scale rounds, then
// in_f - lo, two operations, where decision_head.h's lerp_of has one fma. eval_decisions_kernel
// alone uses it, for every weight into the low-resolution grid: the pixel's own two and the
// eight of the PREDICT-order branch's four network pixels (that branch's two weights from the
// output into the network grid are lerp_of's). It is not the better rounding. It is what
// seg_predict computed while this kernel's text left the contraction to the compiler, which
// packed each of these subtractions with a channel difference into one v_pk_add_f32 and so never
// fused them (read off the gfx950 ISA of both instantiations); it is kept so that seg_predict
// gives the decisions it gave. A weight moves by an ulp at most, so against the fused form a
// decision differs only where the two best probabilities are within rounding of each other. The
// pragma is local to this body: neither operation can be contracted, whatever the caller looks
// like.
__device__ __forceinline__ void lerp_of_rounded(int o, int n_in, int n_out, int& lo, int& hi,
                                                float& l) {
#pragma clang fp contract(off)
  const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
  const float fin = (float)o * scale;
  lo = (int)fin;
  hi = lo + 1 < n_in - 1 ? lo + 1 : n_in - 1;
  l = fin - (float)lo;
}

template <int C1, int C2, int C3>
__global__ __launch_bounds__(256) void eval_decisions_kernel(EvalArgs a, LossTables t) {
  constexpr int CT = C1 + C2 + C3;
  const long total = (long)a.N * a.Ho * a.Wo;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(id % a.Wo);
    const int yo = (int)((id / a.Wo) % a.Ho);
    const int n = (int)(id / ((long)a.Wo * a.Ho));
    const int h = nn_src(yo, a.H, a.Ho), w = nn_src(xo, a.W, a.Wo);
    int ylo, yhi, xlo, xhi;
    float yl, xl;
    lerp_of_rounded(h, a.Hl, a.H, ylo, yhi, yl);
    lerp_of_rounded(w, a.Wl, a.W, xlo, xhi, xl);
    const float* base = a.logits + (size_t)n * a.Hl * a.Wl * a.ldl;
    float p[CT];
    bilerp<CT>(p, cells_of(base, ylo, yhi, xlo, xhi, a.Wl, a.ldl), xl, yl);
    softmax_heads<C1, C2, C3>(p);
    int d = decide<C1, C2, C3>(p, t, a.map, a.replace_voids == 1);
    if (a.replace_voids == 2) {
      // PREDICT order (define_estimator_hierarchical.py:227-231): _resize_predictions first --
      // decisions NEAREST (above), l1_probabilities ResizeBilinear(align_corners) from the
      // network to the output size -- then _replace_voids on the RESIZED probabilities
      // (top_k(k=2), stable; void = decision C1 - 1). The 4 network-resolution pixels of the
      // output pixel's footprint get their l1 softmax from the low-res logits as above.
      int y0, y1, x0, x1;
      float ylp, xlp;
      lerp_of(yo, a.H, a.Ho, y0, y1, ylp);
      lerp_of(xo, a.W, a.Wo, x0, x1, xlp);
      float q[4][C1];
      const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int ya, yb, xa, xb;
        float ly, lx;
        lerp_of_rounded(ys[k >> 1], a.Hl, a.H, ya, yb, ly);
        lerp_of_rounded(xs[k & 1], a.Wl, a.W, xa, xb, lx);
        bilerp<C1>(q[k], cells_of(base, ya, yb, xa, xb, a.Wl, a.ldl), lx, ly);
        softmax<C1>(q[k]);
      }
      int i1 = -1, i2 = -1;
      float v1 = 0.f, v2 = 0.f;
#pragma unroll
      for (int c = 0; c < C1; ++c) {
        const float v = bilerp1(q[0][c], q[1][c], q[2][c], q[3][c], xlp, ylp);
        if (i1 < 0 || v > v1) { i2 = i1; v2 = v1; i1 = c; v1 = v; }
        else if (i2 < 0 || v > v2) { i2 = c; v2 = v; }
      }
      d = d == C1 - 1 ? i2 : i1;
    }
    a.out[id] = d;
  }
}

// The model's full-resolution `predictions` (hierarchical.py:84-130), materialised on demand:
// per network-resolution pixel the align-corners bilinear logits of the three heads, their
// softmax, per-head argmax and the fused common-cid decision; every output is optional. Stores
// are per pixel runs of CT floats.
template <int C1, int C2, int C3>
__global__ __launch_bounds__(256) void full_predictions_kernel(FullPredArgs a, LossTables t) {
  constexpr int CT = C1 + C2 + C3;
  const long total = (long)a.N * a.H * a.W;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (long)gridDim.x * blockDim.x) {
    const int w = (int)(id % a.W);
    const int h = (int)((id / a.W) % a.H);
    const int n = (int)(id / ((long)a.W * a.H));
    int ylo, yhi, xlo, xhi;
    float yl, xl;
    lerp_of(h, a.Hl, a.H, ylo, yhi, yl);
    lerp_of(w, a.Wl, a.W, xlo, xhi, xl);
    const float* base = a.logits + (size_t)n * a.Hl * a.Wl * a.ldl;
    float p[CT];
    bilerp<CT>(p, cells_of(base, ylo, yhi, xlo, xhi, a.Wl, a.ldl), xl, yl);
    if (a.logits_out) store_ct<CT>(a.logits_out + (size_t)id * CT, p, 1.f);
    softmax_heads<C1, C2, C3>(p);
    if (a.probs_out) store_ct<CT>(a.probs_out + (size_t)id * CT, p, 1.f);
    const int d1 = argmax_first<C1>(p);
    if (a.head_decs_out) {
      int* o = a.head_decs_out + (size_t)id * 3;
      o[0] = d1; o[1] = argmax_first<C2>(p + C1); o[2] = argmax_first<C3>(p + C1 + C2);
    }
    if (a.decs_out) a.decs_out[id] = fuse_decision<C1, C2, C3>(p, t, d1);
  }
}

}  // namespace

hipError_t launch_eval_decisions(const EvalArgs& a, const LossTables& t, hipStream_t s) {
  const long total = (long)a.N * a.Ho * a.Wo;
  if (total <= 0) return hipSuccess;
  const dim3 g((unsigned)std::min((total + 255) / 256, 8192L));
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    hipLaunchKernelGGL((eval_decisions_kernel<c1, c2, c3>), g, dim3(256), 0, s, a, t);
  });
}

hipError_t launch_full_predictions(const FullPredArgs& a, const LossTables& t, hipStream_t s) {
  const long total = (long)a.N * a.H * a.W;
  if (total <= 0) return hipSuccess;
  const dim3 g((unsigned)std::min((total + 255) / 256, 16384L));
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    hipLaunchKernelGGL((full_predictions_kernel<c1, c2, c3>), g, dim3(256), 0, s, a, t);
  });
}
