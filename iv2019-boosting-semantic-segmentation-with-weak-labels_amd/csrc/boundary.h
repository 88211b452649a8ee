// Boundary-band (trimap) confusion of the EVAL branch (no reference counterpart; semantics in
// include/seg_hip.h at seg_boundary_distance). All of it is integer arithmetic:
//   counted:  a label l with 0 <= l < nc and l != ignore;
//   boundary: a pixel that carries a counted label and has a 4-neighbour in its image with another
//             counted label (both pixels of the pair);
//   d2:       the least dy^2 + dx^2 to a boundary pixel of the same image, capped at wmax^2 + 1;
//   band w:   d2 <= w^2; cm[k][l][d] counts the pixels of band w_k with label l and decision d,
//             both in [0, nc) (seg_confusion's rule: ignored labels are counted here too).
// Two passes over one byte per pixel:
//   rows:    the boundary flags of 64 columns as one ballot word, then per pixel the horizontal
//            distance g to the nearest flag of its row from three words, capped at wmax + 1;
//   columns: d2 = min over |dy| <= wmax of dy^2 + g(y + dy, x)^2 from an LDS tile of g with a
//            wmax-row halo (rows outside the image hold the cap), then either d2 itself or one
//            count in the histogram of the smallest band that holds the pixel; finalize sums the
//            histograms over k (the bands are nested).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#define BOUNDARY_MAX_WIDTH 64
#define BOUNDARY_MAX_WIDTHS 8
#define BOUNDARY_MAX_IMAGES 65535   // the grid's z dimension is the image

struct BoundaryRowArgs {
  const int* labels;   // [N][H][W]
  int N, H, W;
  int nc, ignore;      // ignore: a class id or -1
  int wmax;            // 1..BOUNDARY_MAX_WIDTH
  uint8_t* g;          // [N][H][W]: min(horizontal distance to a boundary pixel, wmax + 1)
};

struct BoundaryColArgs {
  const uint8_t* g;    // [N][H][W] of launch_boundary_rows with the same wmax
  int N, H, W;
  int wmax;
  // distance: d2 [N][H][W] = min(d2, wmax^2 + 1)
  uint16_t* d2;
  // band confusion: w2[k] = w_k^2, strictly increasing, w2[K - 1] = wmax^2, INT_MAX from K on; cm
  // [K][nc][nc] zeroed by the caller: every pixel is counted at the smallest k that holds it
  // (launch_band_finalize turns that into the nested counts)
  const int* labels;
  const int* decisions;
  int nc, K;
  int w2[BOUNDARY_MAX_WIDTHS];
  int* cm;
};

// bytes of dynamic LDS a block of the band kernel takes at wmax: the g tile alone, and with the
// block's private histogram beside it; the histogram is private where the sum fits 64 KiB
size_t boundary_tile_bytes(int wmax);
bool boundary_hist_in_lds(int wmax, int K, int nc);

hipError_t launch_boundary_rows(const BoundaryRowArgs& a, hipStream_t s);
hipError_t launch_boundary_distance(const BoundaryColArgs& a, hipStream_t s);
hipError_t launch_band_confusion(const BoundaryColArgs& a, hipStream_t s);
hipError_t launch_band_finalize(int* cm, int K, int nc, hipStream_t s);
