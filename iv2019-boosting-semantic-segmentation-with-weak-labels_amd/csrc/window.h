// Sliding-window inference (no reference counterpart beyond the [tile] / [stich] of its system
// sketch, utils/utils.py; semantics in include/seg_hip.h at seg_window_decisions):
//   a window extraction: fp32 [n][Hc][Wc][3] canvas -> the H x W window at (y0, x0), optionally
//     mirrored in x, copied bit for bit;
//   a decision head over the low-resolution logits of a separable grid of windows: per selected
//     canvas pixel the align-corners bilinear logits and per-head softmax of every window that
//     covers it (decision_head.h, the calls tta.hip makes), summed in entry order, times the
//     rounded 1 / k of the k covering entries, then the same argmax / hierarchical fusion / cid
//     map / void replacement / nearest resize from the canvas. No full-resolution intermediate is written unless the mean
//     probabilities are asked for.
#pragma once
#include "loss.h"

#define WIN_MAX_ENTRIES 64

struct WinArgs {
  const float* logits[WIN_MAX_ENTRIES];   // entry (iy * nx + ix) * (1 + flip) + mirrored
  int ys[WIN_MAX_ENTRIES], xs[WIN_MAX_ENTRIES];   // window origins, strictly increasing, no gap
  float rk[WIN_MAX_ENTRIES + 1];          // rk[k] = 1.0f / k, divided on the host (rk[0] unused)
  int ny, nx, flip;
  int hl, wl, ld;          // every entry is [N][hl][wl][ld]: l1 | l2v | l2h channels
  int N, H, W;             // network = window resolution
  int Hc, Wc;              // canvas resolution (where probabilities are averaged)
  int Ho, Wo;              // output resolution
  int replace_voids;       // 0 no, 1 the EVAL order on the l1 sums
  int n_map;
  int map[SEG_MAX_PP];     // training cid -> new cid (voids already replaced)
  float* probs;            // optional [N][Hc][Wc][c1+c2+c3] mean probabilities (Ho x Wo = Hc x Wc)
  int* out;                // [N][Ho][Wo]
};

hipError_t launch_window_images(const float* in, int n, int Hc, int Wc, int y0, int x0, int H,
                                int W, int flip, float* out, hipStream_t s);
hipError_t launch_window_decisions(const WinArgs& a, const LossTables& t, hipStream_t s);
