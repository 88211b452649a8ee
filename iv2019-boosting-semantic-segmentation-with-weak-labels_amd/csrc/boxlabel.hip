// Box-constrained pseudo-label kernels (see boxlabel.h; semantics in include/seg_hip.h).
//
// Three streaming kernels over one geometry: a block owns BL consecutive pixels of one image
// (blockIdx.y), stages that image's boxes in LDS once (stage_boxes: integer source rectangles,
// class, reject flag, and the per-class tables of the heads) and every thread walks the staged
// boxes for its own source pixel (src_pixel). The rectangles and the pixel mapping restate
// bbox_labels_kernel of labels.hip expression by expression; tests pin the two together.
//
// A pixel's CT probabilities are contiguous. Where CT % 4 == 0 (Cityscapes, 24) a thread moves its
// row as 16-byte vectors; where it is not (Vistas, 70) the block's rows, contiguous in memory, go
// through LDS as 16-byte chunks, as bbox_labels_kernel stores its 15-float rows, with half the
// threads so that the staged rows stay within 64 KiB beside the boxes.
#include "boxlabel.h"
#include "decision_head.h"

namespace {

using namespace decision_head;

constexpr int BL_MAX = BOXLABEL_MAX_BOXES;
constexpr int BL_REJECT = 256;   // bit of BoxStage::meta above the class
constexpr int bl_threads(int ct) { return ct % 4 == 0 ? 256 : 128; }
// float4s of LDS the rows of a block take (1: none, a thread loads its own row): the rows, up to
// three floats further in so that the 16-byte chunks of LDS and of memory line up (load_rows)
constexpr int bl_row_vecs(int ct) { return ct % 4 == 0 ? 1 : (bl_threads(ct) * ct + 3 + 3) / 4; }

struct BoxStage {
  alignas(16) int rect[BL_MAX * 4];   // xmin, xmax, ymin, ymax in source pixels, both inclusive
  int meta[BL_MAX];                   // class (bits 0..3) | BL_REJECT
  // per weak class 0..15: the bit of its vehicle / human channel (0: not such a box) and the
  // training cid a pixel of such a box is expected to take (-1 for an inert class)
  unsigned vbit[16], hbit[16];
  int tgt[16];
};

// boxes of image img, clamped to what the stage holds
__device__ __forceinline__ int box_count(const BoxListArgs& bl, int img) {
  return min(max(bl.box_off[img + 1] - bl.box_off[img], 0), BL_MAX);
}

// Stages the nb boxes of image img and the class tables; ends with a barrier.
// reject: NULL or [total] flags.
template <int THREADS>
__device__ __forceinline__ void stage_boxes(BoxStage& s, const BoxListArgs& bl, const int* reject,
                                            int img, int nb, const BboxGeom& g, const LossTables& t) {
  const int b0 = bl.box_off[img];
  for (int b = threadIdx.x; b < nb; b += THREADS) {
    const float* c = bl.boxes + 4 * (size_t)(b0 + b);
    // float32 coordinate times an integer size in float64, truncated (labels.hip)
    const int xmin = (int)((double)c[0] * g.src_w), xmax = (int)((double)c[1] * g.src_w);
    const int ymin = (int)((double)c[2] * g.src_h), ymax = (int)((double)c[3] * g.src_h);
    *reinterpret_cast<int4*>(&s.rect[4 * b]) = make_int4(xmin, xmax, ymin, ymax);
    s.meta[b] = (bl.cids[b0 + b] & 15) | ((reject && reject[b0 + b]) ? BL_REJECT : 0);
  }
  if (threadIdx.x < 16) {
    const int k = threadIdx.x;
    unsigned vb = 0, hb = 0;
    int tg = -1;
    if (k < SEG_WEAK_CLASSES - 1) {   // weak classes 0..13; anything else is inert
      const int v = t.pb2veh[k], h = t.pb2hum[k];
      if (v != t.c2 - 1) { vb = 1u << v; tg = t.veh_to_common[v]; }
      if (h != t.c3 - 1) { hb = 1u << h; if (tg < 0) tg = t.hum_to_common[h]; }
    }
    s.vbit[k] = vb; s.hbit[k] = hb; s.tgt[k] = tg;
  }
  __syncthreads();
}

// the source pixel of output pixel (y, x): TF 1.12 ResizeNearestNeighbor (align_corners = false)
// of the resized map, after the crop offset (labels.hip)
__device__ __forceinline__ void src_pixel(const BboxGeom& g, int y, int x, int& sy, int& sx) {
  const float sh = (float)g.src_h / (float)g.rh, sw = (float)g.src_w / (float)g.rw;
  sy = min((int)floorf((float)(y + g.oy) * sh), g.src_h - 1);
  sx = min((int)floorf((float)(x + g.ox) * sw), g.src_w - 1);
}

__device__ __forceinline__ bool covers(const BoxStage& s, int b, int sy, int sx) {
  const int4 r = *reinterpret_cast<const int4*>(&s.rect[4 * b]);
  return (sx >= r.x) & (sx <= r.y) & (sy >= r.z) & (sy <= r.w);
}

// mask: bit k = a box of class k covers the source pixel; av / ah: the allowed vehicle / human
// channels (AV_i, AH_i)
struct Cover { unsigned mask, av, ah; };

__device__ __forceinline__ Cover cover_of(const BoxStage& s, int nb, int sy, int sx) {
  Cover c{0u, 0u, 0u};
  for (int b = 0; b < nb; ++b)
    if (covers(s, b, sy, sx)) c.mask |= 1u << (s.meta[b] & 15);
#pragma unroll
  for (int k = 0; k < SEG_WEAK_CLASSES - 1; ++k)
    if (c.mask >> k & 1u) { c.av |= s.vbit[k]; c.ah |= s.hbit[k]; }
  return c;
}

// floats from p to the next 16-byte boundary
__device__ __forceinline__ int lead_floats(const float* p) {
  return (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
}

// v[0..CT) = the row of this thread's pixel. src: the block's first row; rows: the block's valid
// pixels. CT % 4 == 0: 16-byte loads of the thread's own row (src 16-byte aligned: the entries
// check the base). Otherwise the block's rows * CT contiguous floats through stage: the floats
// before the first 16-byte boundary of src singly, then 16-byte chunks, then the tail.
template <int CT, int THREADS>
__device__ __forceinline__ void load_rows(const float* src, int rows, float* stage, float* v) {
  if constexpr (CT % 4 == 0) {
    if ((int)threadIdx.x < rows) {
      const float4* p = reinterpret_cast<const float4*>(src + (size_t)threadIdx.x * CT);
#pragma unroll
      for (int u = 0; u < CT / 4; ++u) {
        const float4 q = p[u];
        v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
      }
    }
  } else {
    const int nval = rows * CT;
    const int lead = min(lead_floats(src), nval);
    float* st = stage + ((4 - lead) & 3);   // st + lead is 16-byte aligned, as src + lead is
    const int nvec = (nval - lead) / 4;
    if ((int)threadIdx.x < lead) st[threadIdx.x] = src[threadIdx.x];
    for (int i = threadIdx.x; i < nvec; i += THREADS)
      reinterpret_cast<float4*>(st + lead)[i] = reinterpret_cast<const float4*>(src + lead)[i];
    for (int i = lead + 4 * nvec + threadIdx.x; i < nval; i += THREADS) st[i] = src[i];
    __syncthreads();
    if ((int)threadIdx.x < rows) {
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) v[ch] = st[threadIdx.x * CT + ch];
    }
  }
}

// the counterpart of load_rows; every thread of the block calls it
template <int CT, int THREADS>
__device__ __forceinline__ void store_rows(float* dst, int rows, float* stage, const float* v) {
  if constexpr (CT % 4 == 0) {
    if ((int)threadIdx.x < rows) {
      float4* p = reinterpret_cast<float4*>(dst + (size_t)threadIdx.x * CT);
#pragma unroll
      for (int u = 0; u < CT / 4; ++u) p[u] = make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
    }
  } else {
    // dst's alignment may differ from src's, and the rows then lie up to three floats apart in
    // the stage: every thread has read its row before any thread rewrites one
    const int nval = rows * CT;
    const int lead = min(lead_floats(dst), nval);
    float* st = stage + ((4 - lead) & 3);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) st[threadIdx.x * CT + ch] = v[ch];
    }
    __syncthreads();
    const int nvec = (nval - lead) / 4;
    if ((int)threadIdx.x < lead) dst[threadIdx.x] = st[threadIdx.x];
    for (int i = threadIdx.x; i < nvec; i += THREADS)
      reinterpret_cast<float4*>(dst + lead)[i] = reinterpret_cast<const float4*>(st + lead)[i];
    for (int i = lead + 4 * nvec + threadIdx.x; i < nval; i += THREADS) dst[i] = st[i];
  }
}

// one l2 head under its allowed channels: the others become +0, the kept ones P * (1 / s) with s
// their fp32 sum in channel order; no allowed channel, or a sum that is not >= 1e-30f, keeps P
template <int N>
__device__ __forceinline__ void constrain_head(float* v, unsigned allow) {
  if (!allow) return;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < N; ++c)
    if (allow >> c & 1u) s += v[c];
  if (!(s >= 1e-30f)) return;
  const float rs = 1.f / s;
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = (allow >> c & 1u) ? v[c] * rs : 0.f;
}

// first maximum over the allowed channels only, in channel order (allow != 0)
template <int N>
__device__ __forceinline__ int argmax_allowed(const float* v, unsigned allow) {
  int b = -1;
  float bv = 0.f;
#pragma unroll
  for (int c = 0; c < N; ++c)
    if ((allow >> c & 1u) && (b < 0 || v[c] > bv)) { bv = v[c]; b = c; }
  return b;
}

template <int C1, int C2, int C3>
__global__ __launch_bounds__(bl_threads(C1 + C2 + C3)) void box_constrain_kernel(BoxConstrainArgs a, LossTables t) {
  constexpr int CT = C1 + C2 + C3;
  constexpr int THREADS = bl_threads(CT);
  __shared__ BoxStage bs;
  __shared__ float4 rows4[bl_row_vecs(CT)];
  float* stage = reinterpret_cast<float*>(rows4);
  const int img = blockIdx.y;
  const BboxGeom g = a.b.geom[img];
  const int nb = box_count(a.b, img);
  stage_boxes<THREADS>(bs, a.b, nullptr, img, nb, g, t);
  const long npix = (long)a.H * a.W;
  const long p0 = (long)blockIdx.x * THREADS;
  const int rows = (int)(npix - p0 < THREADS ? npix - p0 : THREADS);
  const size_t row0 = (size_t)img * npix + p0;
  float v[CT];
  load_rows<CT, THREADS>(a.p + row0 * CT, rows, stage, v);
  if ((int)threadIdx.x < rows) {
    const long p = p0 + threadIdx.x;
    const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
    int sy, sx;
    src_pixel(g, y, x, sy, sx);
    const Cover c = cover_of(bs, nb, sy, sx);
    constrain_head<C2>(v + C1, c.av);
    constrain_head<C3>(v + C1 + C2, c.ah);
    if (a.mask) a.mask[row0 + threadIdx.x] = (unsigned short)c.mask;
  }
  store_rows<CT, THREADS>(a.out + row0 * CT, rows, stage, v);
}

template <int C1, int C2, int C3>
__global__ __launch_bounds__(bl_threads(C1 + C2 + C3)) void box_decide_kernel(BoxDecideArgs a, LossTables t) {
  constexpr int CT = C1 + C2 + C3;
  constexpr int THREADS = bl_threads(CT);
  __shared__ BoxStage bs;
  __shared__ int cnt[BL_MAX * 2];   // (area, hit) of this block's pixels per box
  __shared__ float4 rows4[bl_row_vecs(CT)];
  // static LDS ends at 64 KiB: a field more in BoxStage or a wider head has to shrink the block
  static_assert(sizeof(BoxStage) + sizeof(cnt) + sizeof(rows4) <= 64 * 1024, "decide kernel LDS");
  float* stage = reinterpret_cast<float*>(rows4);
  const int img = blockIdx.y;
  const BboxGeom g = a.b.geom[img];
  const int nb = box_count(a.b, img);
  for (int i = threadIdx.x; i < 2 * nb; i += THREADS) cnt[i] = 0;
  stage_boxes<THREADS>(bs, a.b, nullptr, img, nb, g, t);
  const long npix = (long)a.H * a.W;
  const long p0 = (long)blockIdx.x * THREADS;
  const int rows = (int)(npix - p0 < THREADS ? npix - p0 : THREADS);
  const size_t row0 = (size_t)img * npix + p0;
  float v[CT];
  load_rows<CT, THREADS>(a.q + row0 * CT, rows, stage, v);
  const bool valid = (int)threadIdx.x < rows;
  const int ignore = t.n_pp - 1;
  int sy = -1, sx = -1, label = ignore;
  if (valid) {
    const long p = p0 + threadIdx.x;
    const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
    src_pixel(g, y, x, sy, sx);
    const Cover c = cover_of(bs, nb, sy, sx);
    const int d1 = argmax_first<C1>(v);
    float conf = v[0];   // v[d1] as selects: a dynamic index would put the row in scratch
#pragma unroll
    for (int ch = 1; ch < C1; ++ch) conf = ch == d1 ? v[ch] : conf;
    if (d1 == t.cid_l1_vehicle)
      label = c.av ? t.veh_to_common[argmax_allowed<C2>(v + C1, c.av)] : ignore;
    else if (d1 == t.cid_l1_human)
      label = c.ah ? t.hum_to_common[argmax_allowed<C3>(v + C1 + C2, c.ah)] : ignore;
    else
      label = t.l1_to_common[d1];
    if (!(conf >= a.tau)) label = ignore;
    a.labels[row0 + threadIdx.x] = label;
    if (a.conf) a.conf[row0 + threadIdx.x] = conf;
  }
  // per box: the wave's covered pixels and hits as two ballots, one LDS add per wave, then one
  // global add per box and block (integers: exact in any order)
  const bool lane0 = (threadIdx.x & 63) == 0;
  for (int b = 0; b < nb; ++b) {
    const bool in = valid && covers(bs, b, sy, sx);
    const unsigned long long win = __ballot(in);
    if (win) {
      const unsigned long long whit = __ballot(in && label == bs.tgt[bs.meta[b] & 15]);
      if (lane0) {
        atomicAdd(&cnt[2 * b], __popcll(win));
        if (whit) atomicAdd(&cnt[2 * b + 1], __popcll(whit));
      }
    }
  }
  __syncthreads();
  int* out = a.counts + 2 * (size_t)a.b.box_off[img];
  for (int i = threadIdx.x; i < 2 * nb; i += THREADS)
    if (cnt[i]) atomicAdd(&out[i], cnt[i]);
}

__global__ __launch_bounds__(256) void box_zero_counts_kernel(const int* box_off, int n, int* counts) {
  const long total = 2L * box_off[n];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) counts[i] = 0;
}

constexpr int BL_FIN_THREADS = 256;

__global__ __launch_bounds__(BL_FIN_THREADS) void box_finalize_kernel(BoxFinalizeArgs a, LossTables t) {
  __shared__ BoxStage bs;
  const int img = blockIdx.y;
  const BboxGeom g = a.b.geom[img];
  const int nb = box_count(a.b, img);
  stage_boxes<BL_FIN_THREADS>(bs, a.b, a.reject, img, nb, g, t);
  const long nout = (long)a.Ho * a.Wo;
  const long p = (long)blockIdx.x * BL_FIN_THREADS + threadIdx.x;
  if (p >= nout) return;   // no barrier below
  const int yo = (int)(p / a.Wo), xo = (int)(p - (long)yo * a.Wo);
  const int h = nn_src(yo, a.H, a.Ho), w = nn_src(xo, a.W, a.Wo);
  int label = a.labels[((size_t)img * a.H + h) * a.W + w];
  int sy, sx;
  src_pixel(g, h, w, sy, sx);
  for (int b = 0; b < nb; ++b)
    if ((bs.meta[b] & BL_REJECT) && covers(bs, b, sy, sx)) { label = t.n_pp - 1; break; }
  a.out[(size_t)img * nout + p] = label;
}

// the grid's y dimension is the image
constexpr int BL_MAX_IMAGES = 65535;

}  // namespace

hipError_t launch_box_constrain(const BoxConstrainArgs& a, const LossTables& t, hipStream_t s) {
  if (a.N < 1 || a.N > BL_MAX_IMAGES || a.H < 1 || a.W < 1) return hipErrorInvalidValue;
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    constexpr int TH = bl_threads(c1 + c2 + c3);
    const dim3 grid((unsigned)ceil_div((long)a.H * a.W, TH), (unsigned)a.N);
    hipLaunchKernelGGL((box_constrain_kernel<c1, c2, c3>), grid, dim3(TH), 0, s, a, t);
  });
}

hipError_t launch_box_decisions(const BoxDecideArgs& a, const LossTables& t, hipStream_t s) {
  if (a.N < 1 || a.N > BL_MAX_IMAGES || a.H < 1 || a.W < 1) return hipErrorInvalidValue;
  return dispatch_heads(t, [&](auto c1, auto c2, auto c3) {
    constexpr int TH = bl_threads(c1 + c2 + c3);
    const long cells = 2L * a.N * std::max(a.max_boxes, 1);
    hipLaunchKernelGGL(box_zero_counts_kernel, dim3((unsigned)std::min<long>(ceil_div(cells, 256), 1024)),
                       dim3(256), 0, s, a.b.box_off, a.N, a.counts);
    const dim3 grid((unsigned)ceil_div((long)a.H * a.W, TH), (unsigned)a.N);
    hipLaunchKernelGGL((box_decide_kernel<c1, c2, c3>), grid, dim3(TH), 0, s, a, t);
  });
}

hipError_t launch_box_finalize(const BoxFinalizeArgs& a, const LossTables& t, hipStream_t s) {
  if (a.N < 1 || a.N > BL_MAX_IMAGES || a.H < 1 || a.W < 1 || a.Ho < 1 || a.Wo < 1)
    return hipErrorInvalidValue;
  // the head widths select no code here, but widths without tables are an error everywhere
  return dispatch_heads(t, [&](auto, auto, auto) {
    const dim3 grid((unsigned)ceil_div((long)a.Ho * a.Wo, BL_FIN_THREADS), (unsigned)a.N);
    hipLaunchKernelGGL(box_finalize_kernel, grid, dim3(BL_FIN_THREADS), 0, s, a, t);
  });
}
