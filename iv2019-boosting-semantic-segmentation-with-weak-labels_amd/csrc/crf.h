// Mean-field CRF refinement of the per-head probabilities (no reference counterpart; semantics in
// include/seg_hip.h at seg_crf_decisions):
//   one mean-field step: Q^{t+1} from Q^t, the unary P and the prepared image, a Potts model with
//     a bilateral and a spatial kernel over the (2r + 1)^2 - 1 offsets (dy * d, dx * d);
//   decisions from a full-resolution probability tensor: nearest source pixel, then
//     decision_head.h's argmax / hierarchical fusion / cid map / void replacement.
#pragma once
#include "loss.h"

#define CRF_MAX_RADIUS 5
#define CRF_MAX_DILATION 4
#define CRF_MAX_ITERATIONS 32
// the (2r + 1)^2 cells of the neighbourhood in row-major (dy, dx) order, the centre included
#define CRF_MAX_CELLS ((2 * CRF_MAX_RADIUS + 1) * (2 * CRF_MAX_RADIUS + 1))   // 121

struct CrfStepArgs {
  const float* q;          // Q^t   [N][H][W][CT]
  const float* p;          // the unary P, same layout
  const float* img;        // prepared images [N][H][W][3]
  float* out;              // Q^{t+1}; neither q nor p
  int N, H, W;
  int r, d;                // offsets (dy * d, dx * d), dy, dx in -r..r without (0, 0), row-major
  float inv2b;             // 1 / (2 (theta_beta * 2 / 255)^2)
  // per cell of the neighbourhood; the centre (0, 0) is no offset and holds 0 in both tables
  float ga[CRF_MAX_CELLS];     // w_a * exp(-|o|^2 / (2 theta_alpha^2))
  float gs[CRF_MAX_CELLS];     // w_s * exp(-|o|^2 / (2 theta_gamma^2))
};

struct CrfDecideArgs {
  const float* q;          // [N][H][W][CT]
  int N, H, W;
  int Ho, Wo;              // output resolution
  int replace_voids;       // 0 no, 1 the EVAL order on the l1 values
  int n_map;
  int map[SEG_MAX_PP];     // training cid -> new cid (voids already replaced)
  int* out;                // [N][Ho][Wo]
};

// bytes of dynamic LDS the step launch of these head widths and this radius takes (its tile
// choice included); 0 for head widths without an instantiation
size_t crf_step_lds_bytes(const LossTables& t, int r);
hipError_t launch_crf_step(const CrfStepArgs& a, const LossTables& t, hipStream_t s);
hipError_t launch_crf_decisions(const CrfDecideArgs& a, const LossTables& t, hipStream_t s);
