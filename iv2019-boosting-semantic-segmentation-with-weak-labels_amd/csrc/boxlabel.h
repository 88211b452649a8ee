// Box-constrained pseudo-labels from per-head probabilities and a box list (no reference
// counterpart; semantics in include/seg_hip.h at seg_box_constrain):
//   constrain: the l2 heads of a pixel keep only the channels its covering boxes allow;
//   decide:    training-cid labels at the size of the probabilities, the fine class taken among
//              the allowed channels, IGNORE for an unboxed vehicle / human pixel or a confidence
//              below tau, and per box (covered pixels, pixels labelled with the box's class);
//   finalize:  nearest resize of the labels, IGNORE under every rejected box.
// The cover (box rectangles, output pixel -> source pixel) is that of labels.h without flip.
#pragma once
#include "labels.h"
#include "loss.h"

#define BOXLABEL_MAX_BOXES 1024

// boxes [total][4] = (xmin, xmax, ymin, ymax) normalised, cids [total], box_off [n + 1] prefix
// offsets per image, geom [n]: the arguments of launch_bbox_labels
struct BoxListArgs {
  const float* boxes;
  const int* cids;
  const int* box_off;
  const BboxGeom* geom;
};

struct BoxConstrainArgs {
  const float* p;          // [N][H][W][CT]
  BoxListArgs b;
  int N, H, W;
  float* out;              // [N][H][W][CT]; not p
  unsigned short* mask;    // optional [N][H][W]: bit k = some box of class k covers the pixel
};

struct BoxDecideArgs {
  const float* q;          // [N][H][W][CT]
  BoxListArgs b;
  int N, H, W;
  int max_boxes;           // bound of the per-image count: sizes the launch that zeroes counts
  float tau;
  int* labels;             // [N][H][W] training cids
  float* conf;             // optional [N][H][W]: the l1 maximum
  int* counts;             // [total][2] = (area, hit); zeroed by the launch
};

struct BoxFinalizeArgs {
  const int* labels;       // [N][H][W]
  BoxListArgs b;
  const int* reject;       // [total]
  int N, H, W;
  int Ho, Wo;
  int* out;                // [N][Ho][Wo]
};

hipError_t launch_box_constrain(const BoxConstrainArgs& a, const LossTables& t, hipStream_t s);
hipError_t launch_box_decisions(const BoxDecideArgs& a, const LossTables& t, hipStream_t s);
hipError_t launch_box_finalize(const BoxFinalizeArgs& a, const LossTables& t, hipStream_t s);
