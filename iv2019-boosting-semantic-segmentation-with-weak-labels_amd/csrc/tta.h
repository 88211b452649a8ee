// Test-time augmentation (multi-scale and flip inference; no reference counterpart, semantics in
// include/seg_hip.h at seg_tta_decisions):
//   an image pyramid on the device: fp32 [n][H][W][3] -> legacy bilinear (align_corners = False,
//     the arithmetic of input.h's image resize) of the optionally mirrored image;
//   a decision head over several sets of low-resolution logits: per selected network pixel the
//     align-corners bilinear logits and per-head softmax of every entry (decision_head.h, the
//     calls the eval kernel of decide.hip makes), summed in entry order, then the eval kernel's
//     argmax / hierarchical fusion / cid map / void replacement / nearest resize on the sums. No
//     full-resolution intermediate is written unless the mean probabilities are asked for.
#pragma once
#include "loss.h"

#define TTA_MAX_ENTRIES 16

struct TtaEntry {
  const float* logits;     // [N][hl][wl][ld]: l1 | l2v | l2h channels
  int hl, wl, ld;
  int flip;                // 1: the entry saw the mirrored image; read at column W - 1 - x
};

struct TtaArgs {
  TtaEntry e[TTA_MAX_ENTRIES];
  int n_entries;
  float inv_e;             // 1.0f / n_entries, divided on the host
  int N, H, W;             // network resolution (where probabilities are averaged)
  int Ho, Wo;              // output resolution
  int replace_voids;       // 0 no, 1 the EVAL order on the l1 sums
  int n_map;
  int map[SEG_MAX_PP];     // training cid -> new cid (voids already replaced)
  float* probs;            // optional [N][H][W][c1+c2+c3] mean probabilities (Ho x Wo = H x W)
  int* out;                // [N][Ho][Wo]
};

hipError_t launch_resize_images(const float* in, int n, int H, int W, int Ho, int Wo, int flip,
                                float* out, hipStream_t s);
hipError_t launch_tta_decisions(const TtaArgs& a, const LossTables& t, hipStream_t s);
