// Single-forward inference heads over the context's low-resolution logits: the EVAL / PREDICT
// decisions at the output size and the model's full-resolution predictions. The arithmetic is
// decision_head.h's, shared with the multi-entry heads of tta.h and window.h.
#pragma once
#include "loss.h"

// EVAL / PREDICT decisions (define_estimator_hierarchical.py:161-194,215-232): per output
// pixel, the NEAREST_NEIGHBOR align_corners source pixel of the network-resolution decision
// map (_resize_predictions :524-575), recomputed from the low-res logits exactly as the loss
// head does (bilinear, softmax, argmax, hierarchical fusion), mapped through the training ->
// evaluation/inference cid table (_map_predictions_to_new_cids :490-522) and, optionally,
// void decisions replaced by the l1 top-k rule (_replace_voids :577-630).
struct EvalArgs {
  const float* logits;     // [N][Hl][Wl][ldl]
  int N, Hl, Wl, ldl;
  int H, W;                // network resolution (where decisions are formed)
  int Ho, Wo;              // output (label) resolution
  int replace_voids;       // 0 no, 1 EVAL order (replace, then resize), 2 PREDICT order
  int n_map;               // entries of map (= training classes)
  int map[SEG_MAX_PP];     // training cid -> new cid (voids already replaced)
  int* out;                // [N][Ho][Wo]
};

// Full-resolution predictions of the model (hierarchical.py:84-130) at network resolution;
// each output is optional (nullptr skips it)
struct FullPredArgs {
  const float* logits;     // [N][Hl][Wl][ldl]
  int N, Hl, Wl, ldl;
  int H, W;                // network resolution
  float* logits_out;       // [N][H][W][c1+c2+c3] upsampled logits (l1 | l2v | l2h)
  float* probs_out;        // [N][H][W][c1+c2+c3] per-head softmax
  int* head_decs_out;      // [N][H][W][3] per-head argmax (l1, l2v, l2h)
  int* decs_out;           // [N][H][W] fused decisions in common cids
};

hipError_t launch_eval_decisions(const EvalArgs& a, const LossTables& t, hipStream_t s);
hipError_t launch_full_predictions(const FullPredArgs& a, const LossTables& t, hipStream_t s);
