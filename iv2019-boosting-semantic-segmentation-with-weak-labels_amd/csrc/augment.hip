// Training augmentation kernels (see augment.h for the semantics and the pass structure).
#include "augment.h"

// the lerps round like the restatement the tests compare with (IEEE float, no FMA), as in
// input.hip; the scales are divided on the host
#pragma clang fp contract(off)

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_PX = 4;   // consecutive pixels per thread of the storing kernels: 3 x 16 bytes

static_assert(AUG_PARTS == AG_THREADS, "a consuming block sums one partial per thread");

struct AugArgs { int Hr, Wr, H, W, cy, cx; float ry, rx; };   // ry, rx: raw / resized
// per-image scaling scales of one launch: up (sh / H, sw / W), down (H / sh, W / sw)
struct AugScales { float y[AUG_MAX_CHUNK], x[AUG_MAX_CHUNK]; };

__device__ __forceinline__ void lerp_legacy(int o, int n_in, float scale, int& lo, int& hi,
                                            float& l) {
  const float fin = (float)o * scale;
  lo = (int)fin;                  // fin >= 0: floor
  hi = lo + 1 < n_in - 1 ? lo + 1 : n_in - 1;
  l = fin - (float)lo;
}

__device__ __forceinline__ float bilerp(float tl, float tr, float bl, float br, float xl, float yl) {
  const float top = tl + (tr - tl) * xl;
  const float bot = bl + (br - bl) * xl;
  return top + (bot - top) * yl;
}

// the [0, 1] image of seg_prepare_images_crop before its centring
__device__ __forceinline__ void resized_px(const uint8_t* img, const AugArgs& g, int y, int x,
                                           float v[3]) {
  const float inv255 = (float)(1.0 / 255.0);
  int ylo, yhi, xlo, xhi;
  float yl, xl;
  lerp_legacy(y + g.cy, g.Hr, g.ry, ylo, yhi, yl);
  lerp_legacy(x + g.cx, g.Wr, g.rx, xlo, xhi, xl);
  const uint8_t* tl = img + ((size_t)ylo * g.Wr + xlo) * 3;
  const uint8_t* tr = img + ((size_t)ylo * g.Wr + xhi) * 3;
  const uint8_t* bl = img + ((size_t)yhi * g.Wr + xlo) * 3;
  const uint8_t* br = img + ((size_t)yhi * g.Wr + xhi) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v[c] = bilerp((float)tl[c] * inv255, (float)tr[c] * inv255, (float)bl[c] * inv255,
                  (float)br[c] * inv255, xl, yl);
}

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float centre(float x) { return (x - 0.5f) / 0.5f; }
// convert_image_dtype float -> uint8 -> float: trunc(x * 255.5), q * (1 / 255); x in [0, 1]
__device__ __forceinline__ float quant(float x) {
  return (float)(int)(x * 255.5f) * (float)(1.0 / 255.0);
}

__device__ __forceinline__ void rgb_to_hsv(const float c[3], float& h, float& s, float& v) {
  const float r = c[0], g = c[1], b = c[2];
  v = fmaxf(r, fmaxf(g, b));
  const float range = v - fminf(r, fminf(g, b));
  s = v > 0.f ? range / v : 0.f;
  const float n = 1.f / (6.f * range);
  h = r == v ? n * (g - b) : (g == v ? n * (b - r) + 2.f / 6.f : n * (r - g) + 4.f / 6.f);
  h = range == 0.f ? 0.f : h;
  h = h < 0.f ? h + 1.f : h;
}

__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float c[3]) {
  const float dh = 6.f * h;
  const float d[3] = {clip01(fabsf(dh - 3.f) - 1.f), clip01(2.f - fabsf(dh - 2.f)),
                      clip01(2.f - fabsf(dh - 4.f))};
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = ((d[k] - 1.f) * s + 1.f) * v;
}

// distort_color's op orders, 2 bits per op (0 brightness, 1 saturation, 2 hue, 3 contrast),
// one byte per order: 0 = B S H C, 1 = S B C H, 2 = C H B S, 3 = H S C B
__device__ __forceinline__ unsigned colour_seq(int order) { return (0x364BB1E4u >> (8 * order)) & 0xffu; }
__device__ __forceinline__ int contrast_pos(unsigned seq) {
  int k = 0;
  while (((seq >> (2 * k)) & 3u) != 3u) ++k;
  return k;
}

// ops [k0, k1) of the sequence on one pixel; mean is read by the contrast op only
__device__ __forceinline__ void colour_ops(float c[3], const AugParams& a, unsigned seq, int k0,
                                           int k1, const float mean[3]) {
  for (int k = k0; k < k1; ++k) {
    const unsigned op = (seq >> (2 * k)) & 3u;
    if (op == 0u) {
#pragma unroll
      for (int i = 0; i < 3; ++i) c[i] = c[i] + a.brightness_delta;
    } else if (op == 3u) {
#pragma unroll
      for (int i = 0; i < 3; ++i) c[i] = (c[i] - mean[i]) * a.contrast_factor + mean[i];
    } else {
      float h, s, v;
      rgb_to_hsv(c, h, s, v);
      if (op == 1u) {
        s = clip01(s * a.saturation_factor);
      } else {
        h = h + a.hue_delta;
        h = h - floorf(h);
      }
      hsv_to_rgb(h, s, v, c);
    }
  }
}

// every thread returns the block's sums; the order of the additions is fixed
template <int N>
__device__ __forceinline__ void block_sum(float v[N], float* red /* [4 * N] */) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = wave_sum(v[c]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) red[wave * N + c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = ((red[c] + red[N + c]) + red[2 * N + c]) + red[3 * N + c];
  __syncthreads();
}

// AG_PX pixels of 3 floats at pixel p0 of an image of npix pixels; base is 16-byte aligned
// when vec
__device__ __forceinline__ void store_px(float* base, long p0, long npix, bool vec,
                                         const float v[3 * AG_PX]) {
  if (p0 >= npix) return;
  float* o = base + p0 * 3;
  if (vec) {   // npix % AG_PX == 0: the whole group is inside
#pragma unroll
    for (int i = 0; i < 3; ++i)
      ((float4*)o)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else {
    const int nv = (int)(npix - p0 < AG_PX ? npix - p0 : AG_PX) * 3;
    for (int i = 0; i < nv; ++i) o[i] = v[i];
  }
}

// pass 1: per-channel sums of the image entering the contrast op
__global__ __launch_bounds__(AG_THREADS) void aug_contrast_mean_kernel(
    const uint8_t* __restrict__ raw, AugArgs g, const AugParams* __restrict__ prm,
    float* __restrict__ part) {
  __shared__ float red[4 * 3];
  const int img = blockIdx.y;
  const AugParams a = prm[img];
  if (a.color_order < 0) return;
  const unsigned seq = colour_seq(a.color_order);
  const int kc = contrast_pos(seq);
  const long npix = (long)g.H * g.W;
  const uint8_t* im = raw + (size_t)img * g.Hr * g.Wr * 3;
  float acc[3] = {0.f, 0.f, 0.f};
  for (long p = (long)blockIdx.x * AG_THREADS + threadIdx.x; p < npix;
       p += (long)AUG_PARTS * AG_THREADS) {
    float c[3];
    resized_px(im, g, (int)(p / g.W), (int)(p % g.W), c);
    colour_ops(c, a, seq, 0, kc, nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] += c[i];
  }
  block_sum<3>(acc, red);
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)img * AUG_PARTS + blockIdx.x) * 4;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
  }
}

// pass 2: resize + colour + clip + the flip stage's quantisation; an image with no geometry
// is centred and finished here, the others go to the stage un-centred. An image with blur
// leaves quantisation and centring to the blur pass and goes to the buffer that pass reads:
// out when geometry follows (the blur then fills the stage), else the stage
__global__ __launch_bounds__(AG_THREADS) void aug_colour_kernel(
    const uint8_t* __restrict__ raw, AugArgs g, const AugParams* __restrict__ prm,
    const float* __restrict__ part, float* __restrict__ stage, float* __restrict__ out) {
  __shared__ float red[4 * 3];
  const int img = blockIdx.y;
  const AugParams a = prm[img];
  const long npix = (long)g.H * g.W;
  const bool geom = a.flip != 0 || a.scale_mode != 0;
  const bool blur = a.blur_mode != 0;
  const bool colour = a.color_order >= 0;
  const unsigned seq = colour ? colour_seq(a.color_order) : 0u;
  float mean[3] = {0.f, 0.f, 0.f};
  if (colour) {   // uniform per block
    const float* pp = part + ((size_t)img * AUG_PARTS + threadIdx.x) * 4;
    mean[0] = pp[0]; mean[1] = pp[1]; mean[2] = pp[2];
    block_sum<3>(mean, red);
#pragma unroll
    for (int i = 0; i < 3; ++i) mean[i] = mean[i] / (float)npix;
  }
  const uint8_t* im = raw + (size_t)img * g.Hr * g.Wr * 3;
  const long p0 = ((long)blockIdx.x * AG_THREADS + threadIdx.x) * AG_PX;
  float v[3 * AG_PX];
#pragma unroll
  for (int k = 0; k < AG_PX; ++k) {
    const long p = p0 + k;
    float c[3] = {0.f, 0.f, 0.f};
    if (p < npix) {
      resized_px(im, g, (int)(p / g.W), (int)(p % g.W), c);
      if (colour) {
        colour_ops(c, a, seq, 0, 4, mean);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = clip01(c[i]);
      }
      if (a.quantize && !blur) {
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = quant(c[i]);
      }
      if (!geom && !blur) {
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = centre(c[i]);
      }
    }
    v[3 * k] = c[0]; v[3 * k + 1] = c[1]; v[3 * k + 2] = c[2];
  }
  store_px((geom != blur ? stage : out) + (size_t)img * npix * 3, p0, npix, (npix % AG_PX) == 0, v);
}

// ---- pass 2b: random_blur (augment.h) -------------------------------------------------------
// One block per BL_TH x BL_TW output tile: the tile and its K / 2 halo are staged in LDS with the
// border rule applied (every staged coordinate is clamped into the image, so a ragged tile reads
// nothing outside it), then each thread finishes BL_PX pixels from LDS alone.
constexpr int BL_TW = 64, BL_TH = 32;
constexpr int BL_PX = BL_TW * BL_TH / AG_THREADS;
constexpr int BL_KMAX = 9;
constexpr int BL_LDS_FLOATS = (BL_TH + BL_KMAX - 1) * (BL_TW + BL_KMAX - 1) * 3;

// where the tile's results go: the flip stage's round trip, and the centring of an image that no
// geometry pass follows
__device__ __forceinline__ void blur_store(float* dst, int W, int y, int x, float c[3], bool q,
                                           bool ctr) {
  float* o = dst + ((size_t)y * W + x) * 3;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float v = c[i];
    if (q) v = quant(v);
    if (ctr) v = centre(v);
    o[i] = v;
  }
}

// cv2.medianBlur on 8-bit data: q = trunc(x * 255), per-channel median of the K x K window with
// replicated borders, q_med / 255. A staged pixel is one word of three 10-bit fields, each the
// channel's byte with bit 9 set. The median is built most significant bit first: candidate
// t = m | bit is kept when at least N / 2 + 1 window values are >= t, and (field - t) keeps its
// bit 9 exactly when value >= t (512 + v - t >= 257, so no borrow crosses a field), so one
// subtract, shift, mask and add per window word counts all three channels. Exact.
template <int K>
__device__ __forceinline__ void blur_median_tile(const float* src, float* dst, int H, int W, int y0,
                                                 int x0, bool q, bool ctr, uint32_t* lds) {
  constexpr int R = K / 2, SW = BL_TW + 2 * R, SH = BL_TH + 2 * R, N = K * K;
  constexpr uint32_t LOW = 1u | (1u << 10) | (1u << 20), GUARD = LOW << 9;
  for (int e = threadIdx.x; e < SH * SW; e += AG_THREADS) {
    const int sy = e / SW, sx = e - sy * SW;
    const int gy = min(max(y0 - R + sy, 0), H - 1), gx = min(max(x0 - R + sx, 0), W - 1);
    const float* p = src + ((size_t)gy * W + gx) * 3;
    const uint32_t r = min((uint32_t)(p[0] * 255.f), 255u), g = min((uint32_t)(p[1] * 255.f), 255u),
                   b = min((uint32_t)(p[2] * 255.f), 255u);
    lds[e] = r | (g << 10) | (b << 20) | GUARD;
  }
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < BL_PX; ++i) {
    const int e = threadIdx.x + i * AG_THREADS;
    const int ly = e / BL_TW, lx = e % BL_TW;
    if (y0 + ly >= H || x0 + lx >= W) continue;
    uint32_t w[N];
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
      for (int dx = 0; dx < K; ++dx) w[dy * K + dx] = lds[(ly + dy) * SW + lx + dx];
    uint32_t m = 0;
#pragma unroll
    for (int bit = 7; bit >= 0; --bit) {
      const uint32_t t = m | (LOW << bit);
      uint32_t ge = 0;
#pragma unroll
      for (int k = 0; k < N; ++k) ge += ((w[k] - t) >> 9) & LOW;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (((ge >> (10 * c)) & 0x3ffu) >= (uint32_t)(N / 2 + 1)) m |= (1u << bit) << (10 * c);
    }
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (float)((m >> (10 * k)) & 0xffu) / 255.f;
    blur_store(dst, W, y0 + ly, x0 + lx, c, q, ctr);
  }
}

__device__ __forceinline__ int reflect101(int g, int n) {   // n >= K / 2 + 1 (aug_validate)
  g = g < 0 ? -g : g;
  g = g >= n ? 2 * n - 2 - g : g;
  return min(max(g, 0), n - 1);   // only positions of a ragged tile that no kept output reads
}

// cv2.bilateralFilter's float path in closed form: taps on the disc i^2 + j^2 <= R^2, borders
// reflect-101, weight exp(coef * (i^2 + j^2)) * exp(coef * (|dR| + |dG| + |dB|)^2) with
// coef = -0.5 / sigma^2, weighted mean per channel. Taps are summed row by row.
template <int K>
__device__ __forceinline__ void blur_bilateral_tile(const float* src, float* dst, int H, int W,
                                                    int y0, int x0, float sigma, bool q, bool ctr,
                                                    float* lds) {
  constexpr int R = K / 2, SW = BL_TW + 2 * R, SH = BL_TH + 2 * R;
  for (int e = threadIdx.x; e < SH * SW * 3; e += AG_THREADS) {
    const int sy = e / (SW * 3), rem = e - sy * (SW * 3);
    const int sx = rem / 3, c = rem - sx * 3;
    const int gy = reflect101(y0 - R + sy, H), gx = reflect101(x0 - R + sx, W);
    lds[e] = src[((size_t)gy * W + gx) * 3 + c];
  }
  __syncthreads();
  // a sigma whose square underflows would give 0 * -inf at the centre tap
  const float coef = fmaxf(-0.5f / (sigma * sigma), -3.4028234e38f);
  float sp[R * R + 1];
#pragma unroll
  for (int d = 0; d <= R * R; ++d) sp[d] = expf((float)d * coef);
#pragma unroll 1
  for (int i = 0; i < BL_PX; ++i) {
    const int e = threadIdx.x + i * AG_THREADS;
    const int ly = e / BL_TW, lx = e % BL_TW;
    if (y0 + ly >= H || x0 + lx >= W) continue;
    const float* ctrp = lds + ((ly + R) * SW + lx + R) * 3;
    const float c0 = ctrp[0], c1 = ctrp[1], c2 = ctrp[2];
    float acc[3] = {0.f, 0.f, 0.f}, sum = 0.f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        if (dy * dy + dx * dx > R * R) continue;
        const float* p = ctrp + (dy * SW + dx) * 3;
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        const float d = (fabsf(p0 - c0) + fabsf(p1 - c1)) + fabsf(p2 - c2);
        const float wgt = sp[dy * dy + dx * dx] * expf((d * d) * coef);
        acc[0] += p0 * wgt; acc[1] += p1 * wgt; acc[2] += p2 * wgt;
        sum += wgt;
      }
    float c[3] = {acc[0] / sum, acc[1] / sum, acc[2] / sum};
    blur_store(dst, W, y0 + ly, x0 + lx, c, q, ctr);
  }
}

// Reads the buffer the colour pass wrote for the image and writes the other one: stage -> out
// (finished: quantised, centred) without geometry, out -> stage (quantised) with it.
__global__ __launch_bounds__(AG_THREADS) void aug_blur_kernel(float* stage, float* out, int H, int W,
                                                              int tiles_x,
                                                              const AugParams* __restrict__ prm) {
  __shared__ float lds[BL_LDS_FLOATS];
  const int img = blockIdx.y;
  const AugParams a = prm[img];
  if (a.blur_mode == 0) return;
  const bool geom = a.flip != 0 || a.scale_mode != 0;
  const size_t off = (size_t)img * H * W * 3;
  const float* src = (geom ? out : stage) + off;
  float* dst = (geom ? stage : out) + off;
  const int y0 = (int)(blockIdx.x / tiles_x) * BL_TH, x0 = (int)(blockIdx.x % tiles_x) * BL_TW;
  const bool q = a.quantize != 0, ctr = !geom;
  if (a.blur_mode == 1) {
    uint32_t* l = (uint32_t*)lds;
    switch (a.blur_ksize) {   // uniform per block
      case 3: blur_median_tile<3>(src, dst, H, W, y0, x0, q, ctr, l); break;
      case 5: blur_median_tile<5>(src, dst, H, W, y0, x0, q, ctr, l); break;
      case 7: blur_median_tile<7>(src, dst, H, W, y0, x0, q, ctr, l); break;
      default: blur_median_tile<9>(src, dst, H, W, y0, x0, q, ctr, l); break;
    }
  } else {
    switch (a.blur_ksize) {
      case 3: blur_bilateral_tile<3>(src, dst, H, W, y0, x0, a.blur_sigma, q, ctr, lds); break;
      case 5: blur_bilateral_tile<5>(src, dst, H, W, y0, x0, a.blur_sigma, q, ctr, lds); break;
      case 7: blur_bilateral_tile<7>(src, dst, H, W, y0, x0, a.blur_sigma, q, ctr, lds); break;
      default: blur_bilateral_tile<9>(src, dst, H, W, y0, x0, a.blur_sigma, q, ctr, lds); break;
    }
  }
}

// the staged image after the flip: pixel (y, x) of the flip stage's output
__device__ __forceinline__ const float* staged(const float* st, int W, int flip, int y, int x) {
  return st + ((size_t)y * W + (flip ? W - 1 - x : x)) * 3;
}

// pixel (i, j) of the down-scaled (sh, sw) image
__device__ __forceinline__ void down_px(const float* st, const AugParams& a, int H, int W,
                                        float scy, float scx, int i, int j, float v[3]) {
  int ylo, yhi, xlo, xhi;
  float yl, xl;
  lerp_legacy(i, H, scy, ylo, yhi, yl);
  lerp_legacy(j, W, scx, xlo, xhi, xl);
  const float* tl = staged(st, W, a.flip, ylo, xlo);
  const float* tr = staged(st, W, a.flip, ylo, xhi);
  const float* bl = staged(st, W, a.flip, yhi, xlo);
  const float* br = staged(st, W, a.flip, yhi, xhi);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = bilerp(tl[c], tr[c], bl[c], br[c], xl, yl);
}

// pixel (y, x) of the crop (sh, sw) at (oy, ox), quantised, resized back to H x W
__device__ __forceinline__ void up_px(const float* st, const AugParams& a, int W, float scy,
                                      float scx, int y, int x, float v[3]) {
  int ylo, yhi, xlo, xhi;
  float yl, xl;
  lerp_legacy(y, a.sh, scy, ylo, yhi, yl);
  lerp_legacy(x, a.sw, scx, xlo, xhi, xl);
  const float* tl = staged(st, W, a.flip, a.oy + ylo, a.ox + xlo);
  const float* tr = staged(st, W, a.flip, a.oy + ylo, a.ox + xhi);
  const float* bl = staged(st, W, a.flip, a.oy + yhi, a.ox + xlo);
  const float* br = staged(st, W, a.flip, a.oy + yhi, a.ox + xhi);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v[c] = bilerp(quant(tl[c]), quant(tr[c]), quant(bl[c]), quant(br[c]), xl, yl);
}

// pass 3: the sum over all pixels and channels of the down-scaled image
__global__ __launch_bounds__(AG_THREADS) void aug_down_mean_kernel(
    const float* __restrict__ stage, int H, int W, const AugParams* __restrict__ prm,
    AugScales sc, float* __restrict__ part) {
  __shared__ float red[4];
  const int img = blockIdx.y;
  const AugParams a = prm[img];
  if (a.scale_mode != 2) return;
  const float* st = stage + (size_t)img * H * W * 3;
  const long cnt = (long)a.sh * a.sw;
  float acc[1] = {0.f};
  for (long e = (long)blockIdx.x * AG_THREADS + threadIdx.x; e < cnt;
       e += (long)AUG_PARTS * AG_THREADS) {
    float v[3];
    down_px(st, a, H, W, sc.y[img], sc.x[img], (int)(e / a.sw), (int)(e % a.sw), v);
    acc[0] += (v[0] + v[1]) + v[2];
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) part[(size_t)img * AUG_PARTS + blockIdx.x] = acc[0];
}

// pass 4: flip / up / down gather from the stage, centred
__global__ __launch_bounds__(AG_THREADS) void aug_geometry_kernel(
    const float* __restrict__ stage, int H, int W, const AugParams* __restrict__ prm,
    AugScales sc, const float* __restrict__ part, float* __restrict__ out) {
  __shared__ float red[4];
  const int img = blockIdx.y;
  const AugParams a = prm[img];
  if (a.flip == 0 && a.scale_mode == 0) return;   // finished by the colour pass
  const long npix = (long)H * W;
  const float* st = stage + (size_t)img * npix * 3;
  const float scy = sc.y[img], scx = sc.x[img];
  float fill[1] = {0.f};
  if (a.scale_mode == 2) {   // uniform per block
    fill[0] = part[(size_t)img * AUG_PARTS + threadIdx.x];
    block_sum<1>(fill, red);
    fill[0] = fill[0] / (float)((long)a.sh * a.sw * 3);
  }
  const int top = (H - a.sh) / 2, left = (W - a.sw) / 2;
  const long p0 = ((long)blockIdx.x * AG_THREADS + threadIdx.x) * AG_PX;
  float v[3 * AG_PX];
#pragma unroll
  for (int k = 0; k < AG_PX; ++k) {
    const long p = p0 + k;
    float c[3] = {0.f, 0.f, 0.f};
    if (p < npix) {
      const int y = (int)(p / W), x = (int)(p % W);
      if (a.scale_mode == 1) {
        up_px(st, a, W, scy, scx, y, x, c);
      } else if (a.scale_mode == 2) {
        const int i = y - top, j = x - left;
        if (i >= 0 && i < a.sh && j >= 0 && j < a.sw) down_px(st, a, H, W, scy, scx, i, j, c);
        else c[0] = c[1] = c[2] = fill[0];
      } else {
        const float* s = staged(st, W, 1, y, x);
        c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) c[i] = centre(c[i]);
    }
    v[3 * k] = c[0]; v[3 * k + 1] = c[1]; v[3 * k + 2] = c[2];
  }
  store_px(out + (size_t)img * npix * 3, p0, npix, (npix % AG_PX) == 0, v);
}

__device__ __forceinline__ int nearest(int o, float scale, int n_in) {
  const int s = (int)floorf((float)o * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

// labels: one gather composing the scaling's nearest resize / pad, the flip and the prepare
// step's nearest resize + lids2cids
__global__ __launch_bounds__(AG_THREADS) void aug_labels_kernel(
    const uint8_t* __restrict__ raw, int Hr, int Wr, int H, int W, float ry, float rx, LidMap m,
    const AugParams* __restrict__ prm, AugScales sc, int32_t* __restrict__ out) {
  const int img = blockIdx.y;
  const AugParams a = prm[img];
  const long npix = (long)H * W;
  const float scy = sc.y[img], scx = sc.x[img];
  const int top = (H - a.sh) / 2, left = (W - a.sw) / 2;
  const uint8_t* im = raw + (size_t)img * Hr * Wr;
  const long p0 = ((long)blockIdx.x * AG_THREADS + threadIdx.x) * AG_PX;
  if (p0 >= npix) return;
  int v[AG_PX];
#pragma unroll
  for (int k = 0; k < AG_PX; ++k) {
    const long p = p0 + k;
    v[k] = 0;
    if (p < npix) {
      const int y = (int)(p / W), x = (int)(p % W);
      int fy = y, fx = x;   // position in the flip stage's H x W label
      bool pad = false;
      if (a.scale_mode == 1) {
        fy = a.oy + nearest(y, scy, a.sh);
        fx = a.ox + nearest(x, scx, a.sw);
      } else if (a.scale_mode == 2) {
        const int i = y - top, j = x - left;
        pad = i < 0 || i >= a.sh || j < 0 || j >= a.sw;
        fy = pad ? 0 : nearest(i, scy, H);
        fx = pad ? 0 : nearest(j, scx, W);
      }
      if (a.flip) fx = W - 1 - fx;
      const int lid = im[(size_t)nearest(fy, ry, Hr) * Wr + nearest(fx, rx, Wr)];
      const int cid = lid < m.n ? m.cid[lid] : -1;   // as seg_prepare_labels
      v[k] = pad ? a.void_cid : cid;
    }
  }
  int32_t* o = out + (size_t)img * npix + p0;
  if ((npix % AG_PX) == 0 && ((uintptr_t)o & 15) == 0) {
    *(int4*)o = make_int4(v[0], v[1], v[2], v[3]);
  } else {
    const int nv = (int)(npix - p0 < AG_PX ? npix - p0 : AG_PX);
    for (int i = 0; i < nv; ++i) o[i] = v[i];
  }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// host-divided scales of images [b0, b0 + nc)
AugScales chunk_scales(const AugParams* host, int nc, int H, int W) {
  AugScales sc{};
  for (int i = 0; i < nc; ++i) {
    const AugParams& a = host[i];
    if (a.scale_mode == 1) { sc.y[i] = (float)a.sh / (float)H; sc.x[i] = (float)a.sw / (float)W; }
    if (a.scale_mode == 2) { sc.y[i] = (float)H / (float)a.sh; sc.x[i] = (float)W / (float)a.sw; }
  }
  return sc;
}

// pass timing (seg_augment_profile[_blur]): events around the passes of a call's first chunk, in
// launch order: contrast mean, colour, blur, down-scale mean, geometry
bool g_prof = false;
constexpr int AG_EVENTS = 6;
hipEvent_t g_ev[AG_EVENTS] = {};

}  // namespace

hipError_t aug_profile_enable(bool on) {
  for (int i = 0; i < AG_EVENTS && on && !g_ev[i]; ++i) {
    const hipError_t e = hipEventCreate(&g_ev[i]);
    if (e != hipSuccess) return e;
  }
  g_prof = on;
  return hipSuccess;
}

hipError_t aug_profile_read(float ms[4]) {
  if (!g_ev[0]) return hipErrorNotReady;
  hipError_t e = hipEventSynchronize(g_ev[AG_EVENTS - 1]);
  const int first[4] = {0, 1, 3, 4};   // the blur pass sits between events 2 and 3
  for (int i = 0; i < 4 && e == hipSuccess; ++i)
    e = hipEventElapsedTime(&ms[i], g_ev[first[i]], g_ev[first[i] + 1]);
  return e;
}

hipError_t aug_profile_read_blur(float* ms) {
  if (!g_ev[0]) return hipErrorNotReady;
  const hipError_t e = hipEventSynchronize(g_ev[AG_EVENTS - 1]);
  return e == hipSuccess ? hipEventElapsedTime(ms, g_ev[2], g_ev[3]) : e;
}

// [stage n * H * W * 3 floats][contrast partials n * AUG_PARTS * 4][down partials n * AUG_PARTS]
size_t aug_workspace_bytes(int n, int H, int W) {
  const size_t npix = (size_t)H * W;
  return align256((size_t)n * npix * 3 * sizeof(float)) +
         align256((size_t)n * AUG_PARTS * 4 * sizeof(float)) +
         align256((size_t)n * AUG_PARTS * sizeof(float));
}

hipError_t launch_augment_images(const uint8_t* raw, int n, const AugResize& r, int H, int W,
                                 const AugParams* host, const AugParams* dev, float* out,
                                 void* workspace, hipStream_t s) {
  const size_t npix = (size_t)H * W;
  if (n <= 0 || npix == 0) return hipSuccess;
  float* stage = (float*)workspace;
  float* part1 = (float*)((char*)workspace + align256((size_t)n * npix * 3 * sizeof(float)));
  float* part2 = (float*)((char*)part1 + align256((size_t)n * AUG_PARTS * 4 * sizeof(float)));
  const AugArgs g{r.Hr, r.Wr, H, W, r.cy, r.cx, (float)r.Hr / (float)r.Hs,
                  (float)r.Wr / (float)r.Ws};   // host IEEE division
  const unsigned gx = (unsigned)ceil_div((long)npix, (long)AG_THREADS * AG_PX);
  for (int b0 = 0; b0 < n; b0 += AUG_MAX_CHUNK) {
    const int nc = std::min(n - b0, AUG_MAX_CHUNK);
    bool colour = false, geom = false, down = false, blur = false;
    for (int i = 0; i < nc; ++i) {
      const AugParams& a = host[b0 + i];
      colour |= a.color_order >= 0;
      geom |= a.flip != 0 || a.scale_mode != 0;
      down |= a.scale_mode == 2;
      blur |= a.blur_mode != 0;
    }
    const AugScales sc = chunk_scales(host + b0, nc, H, W);
    const uint8_t* raw_c = raw + (size_t)b0 * r.Hr * r.Wr * 3;
    const AugParams* prm = dev + b0;
    float* stage_c = stage + (size_t)b0 * npix * 3;
    float* out_c = out + (size_t)b0 * npix * 3;
    float* p1 = part1 + (size_t)b0 * AUG_PARTS * 4;
    float* p2 = part2 + (size_t)b0 * AUG_PARTS;
    const bool prof = g_prof && b0 == 0;
    if (prof) (void)hipEventRecord(g_ev[0], s);
    if (colour)
      hipLaunchKernelGGL(aug_contrast_mean_kernel, dim3(AUG_PARTS, nc), dim3(AG_THREADS), 0, s,
                         raw_c, g, prm, p1);
    if (prof) (void)hipEventRecord(g_ev[1], s);
    hipLaunchKernelGGL(aug_colour_kernel, dim3(gx, nc), dim3(AG_THREADS), 0, s, raw_c, g, prm, p1,
                       stage_c, out_c);
    if (prof) (void)hipEventRecord(g_ev[2], s);
    if (blur) {
      const int tx = ceil_div(W, BL_TW), ty = ceil_div(H, BL_TH);
      hipLaunchKernelGGL(aug_blur_kernel, dim3((unsigned)(tx * ty), nc), dim3(AG_THREADS), 0, s,
                         stage_c, out_c, H, W, tx, prm);
    }
    if (prof) (void)hipEventRecord(g_ev[3], s);
    if (down)
      hipLaunchKernelGGL(aug_down_mean_kernel, dim3(AUG_PARTS, nc), dim3(AG_THREADS), 0, s,
                         stage_c, H, W, prm, sc, p2);
    if (prof) (void)hipEventRecord(g_ev[4], s);
    if (geom)
      hipLaunchKernelGGL(aug_geometry_kernel, dim3(gx, nc), dim3(AG_THREADS), 0, s, stage_c, H, W,
                         prm, sc, p2, out_c);
    if (prof) (void)hipEventRecord(g_ev[5], s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_augment_labels(const uint8_t* raw, int n, int Hr, int Wr, int H, int W,
                                 const LidMap& m, const AugParams* host, const AugParams* dev,
                                 int32_t* out, hipStream_t s) {
  const size_t npix = (size_t)H * W;
  if (n <= 0 || npix == 0) return hipSuccess;
  const float ry = (float)Hr / (float)H, rx = (float)Wr / (float)W;
  const unsigned gx = (unsigned)ceil_div((long)npix, (long)AG_THREADS * AG_PX);
  for (int b0 = 0; b0 < n; b0 += AUG_MAX_CHUNK) {
    const int nc = std::min(n - b0, AUG_MAX_CHUNK);
    const AugScales sc = chunk_scales(host + b0, nc, H, W);
    hipLaunchKernelGGL(aug_labels_kernel, dim3(gx, nc), dim3(AG_THREADS), 0, s,
                       raw + (size_t)b0 * Hr * Wr, Hr, Wr, H, W, ry, rx, m, dev + b0, sc,
                       out + (size_t)b0 * npix);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
