// Per-image augmentation record (the layout of seg_aug_params in include/seg_hip.h) and its
// host-side validation. Plain C++ with no HIP dependency, so the validation also compiles into
// a stand-alone CPU program. A table that fails here never reaches a kernel.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

struct AugParams {        // 64 bytes, one per image
  int32_t color_order;    // -1 none, 0..3 (distort_color's four op orders)
  float brightness_delta;
  float saturation_factor;
  float hue_delta;
  float contrast_factor;
  int32_t quantize;       // the flip stage's uint8 round trip (on whenever the stage is enabled)
  int32_t flip;
  int32_t scale_mode;     // 0 none, 1 up (crop + resize back), 2 down (resize + pad)
  int32_t sh, sw;         // up: crop size; down: resized size
  int32_t oy, ox;         // up: crop offset
  int32_t void_cid;       // label fill of the down-scale pad
  // seg_aug_params' blur sub-record (mode, ksize, sigma), flat
  int32_t blur_mode;      // 0 none, 1 median, 2 bilateral
  int32_t blur_ksize;     // odd, 3..9: the k x k window (median), the disc's diameter (bilateral)
  float blur_sigma;       // bilateral: sigmaColor = sigmaSpace, on values in [0, 1]
};
static_assert(sizeof(AugParams) == 64, "seg_aug_params is 64 bytes");

// 0 when every record is usable at H x W, else the index + 1 of the first bad record with the
// reason in msg
static inline int aug_validate(const AugParams* p, int n, int H, int W, char* msg, size_t len) {
  for (int i = 0; i < n; ++i) {
    const AugParams& a = p[i];
    if (a.color_order < -1 || a.color_order > 3) {
      snprintf(msg, len, "image %d: color_order = %d (-1..3)", i, a.color_order);
      return i + 1;
    }
    if (a.scale_mode < 0 || a.scale_mode > 2) {
      snprintf(msg, len, "image %d: scale_mode = %d (0..2)", i, a.scale_mode);
      return i + 1;
    }
    if (a.scale_mode != 0) {
      if (a.sh < 1 || a.sh > H || a.sw < 1 || a.sw > W) {
        snprintf(msg, len, "image %d: scaled size %dx%d outside 1..%d x 1..%d", i, a.sh, a.sw, H, W);
        return i + 1;
      }
      if (a.void_cid < 0) {
        snprintf(msg, len, "image %d: void_cid = %d", i, a.void_cid);
        return i + 1;
      }
    }
    // 64-bit sums: an offset near INT32_MAX must not wrap into the image
    if (a.scale_mode == 1 && (a.oy < 0 || a.ox < 0 || (int64_t)a.oy + a.sh > H ||
                              (int64_t)a.ox + a.sw > W)) {
      snprintf(msg, len, "image %d: crop %dx%d at (%d, %d) outside the %dx%d image", i, a.sh, a.sw,
               a.oy, a.ox, H, W);
      return i + 1;
    }
    if (a.blur_mode < 0 || a.blur_mode > 2) {
      snprintf(msg, len, "image %d: blur.mode = %d (0..2)", i, a.blur_mode);
      return i + 1;
    }
    if (a.blur_mode != 0 && (a.blur_ksize < 3 || a.blur_ksize > 9 || a.blur_ksize % 2 == 0)) {
      snprintf(msg, len, "image %d: blur.ksize = %d (odd, 3..9)", i, a.blur_ksize);
      return i + 1;
    }
    if (a.blur_mode == 2) {
      // a NaN fails the first comparison, an infinity the second
      if (!(a.blur_sigma > 0.f) || !(a.blur_sigma <= 3.4028234e38f)) {
        snprintf(msg, len, "image %d: blur.sigma = %g (finite, > 0)", i, (double)a.blur_sigma);
        return i + 1;
      }
      // reflect-101 reaches blur_ksize / 2 pixels past an edge
      if ((H < W ? H : W) < a.blur_ksize / 2 + 1) {
        snprintf(msg, len, "image %d: bilateral blur.ksize = %d needs min(H, W) >= %d, got %dx%d", i,
                 a.blur_ksize, a.blur_ksize / 2 + 1, H, W);
        return i + 1;
      }
    }
  }
  return 0;
}
