// Training augmentation on the GPU: the reference's preprocessing/augmentation_library.py
// (random_color :359-406, random_blur :408-466, random_flipping :298-321, random_scaling :21-296)
// restated as pure functions of (raw input, per-image parameter record). The random draws happen
// on the host (input_pipelines/augment.py). Per image, in the reference's order:
//   resize (as seg_prepare_images[_crop]) -> colour -> blur -> flip stage -> scaling
//   -> (x - 0.5) / 0.5
//   colour : brightness x + d | saturation / hue through HSV | contrast (x - m_c) * f + m_c with
//            m_c the per-channel mean of the image entering the op; four op orders; clip to [0, 1]
//   blur   : median (cv2.medianBlur on 8-bit data): q = trunc(x * 255), per-channel median of the
//            k x k window with replicated borders, q_med / 255; or bilateral (cv2.bilateralFilter,
//            float path, sigmaColor = sigmaSpace = sigma on values in [0, 1]): taps (i, j) with
//            i^2 + j^2 <= (k / 2)^2, reflect-101 borders, weight exp(-(i^2 + j^2) / (2 sigma^2)) *
//            exp(-(|dR| + |dG| + |dB|)^2 / (2 sigma^2)), weighted mean per channel. cv2 reads its
//            colour term from a table of 4096 bins per channel with linear interpolation; that
//            table is not reproduced, the closed form is the specification (like the rest of
//            this file, parity with cv2 / TF themselves is unpinned). k is odd, 3..9
//   flip   : every image of an enabled stage goes through uint8 (trunc(x * 255.5)) and back
//            (q * (1 / 255)); flipped ones are mirrored in x
//   up     : crop (sh, sw) at (oy, ox), uint8 round trip, legacy bilinear resize back to H x W
//            (labels: nearest)
//   down   : legacy bilinear resize to (sh, sw) (labels: nearest), centred in H x W; the rest is
//            the scalar mean of the resized image (labels: void_cid)
//
// Passes over a batch (each skipped when no image of the batch needs it; inside a launch an
// image that does not need the pass costs one early-exit per block):
//   1 contrast mean   raw -> resize + the ops ahead of the contrast -> AUG_PARTS partial sums
//   2 colour          raw -> resize + colour + clip + quantise -> out (no geometry) or stage
//   2b blur           LDS-tiled median / bilateral from the buffer pass 2 wrote for the image to
//                     the other one (never in place): stage -> out, or out -> stage when
//                     geometry follows; a blurred image is quantised / centred here, not in 2
//   3 down-scale mean stage -> bilinear (sh, sw) -> AUG_PARTS partial sums
//   4 geometry        stage -> flip / up / down gather -> out
// Both means are sums of fixed per-thread strides, a fixed block tree and a fixed-order sum of
// the AUG_PARTS partials that every consuming block repeats: no atomics, bitwise repeatable.
#pragma once
#include "aug_params.h"
#include "input.h"

#define AUG_PARTS 256       // partial sums per image and mean
#define AUG_MAX_CHUNK 32    // images per launch (their host-divided scales travel as arguments)

// resize / crop geometry of seg_prepare_images_crop
struct AugResize { int Hr, Wr, Hs, Ws, cy, cx; };

size_t aug_workspace_bytes(int n, int H, int W);
// host: the validated host copy of the device table dev
hipError_t launch_augment_images(const uint8_t* raw, int n, const AugResize& r, int H, int W,
                                 const AugParams* host, const AugParams* dev, float* out,
                                 void* workspace, hipStream_t s);
hipError_t launch_augment_labels(const uint8_t* raw, int n, int Hr, int Wr, int H, int W,
                                 const LidMap& m, const AugParams* host, const AugParams* dev,
                                 int32_t* out, hipStream_t s);
// diagnostics (tools/aug_table.py): with profiling on, every seg_augment_images call records
// events around its passes (first AUG_MAX_CHUNK images); read waits for the last call and
// gives the milliseconds of passes 1, 2, 3, 4 (0 for a skipped pass), read_blur those of pass 2b.
// Not for use inside a captured graph.
hipError_t aug_profile_enable(bool on);
hipError_t aug_profile_read(float ms[4]);
hipError_t aug_profile_read_blur(float* ms);
