// Internal to the native runtime of the training step (net_build.cpp, net_layers.cpp,
// net_step.cpp, api.cpp, api_ops.cpp): the dilated-ResNet + pyramid + hierarchical heads graph
// (slim resnet_v1 unit schedule, reference models/*), its context and what those files share.
// The C ABI is declared in include/seg_hip.h; seg_ctx is opaque to it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/seg_hip.h"
#include "bn.h"
#include "bootstrap.h"
#include "boundary.h"
#include "boxlabel.h"
#include "lbf.h"
#include "input.h"
#include "augment.h"
#include "conv.h"
#include "crf.h"
#include "decide.h"
#include "deconv.h"
#include "gn.h"
#include "loss.h"
#include "labels.h"
#include "optim.h"
#include "pool.h"
#include "tta.h"
#include "window.h"

namespace segnet {

struct Act {
  void* p = nullptr;
  int N = 0, H = 0, W = 0, C = 0, ld = 0;
  uint8_t* mask = nullptr;   // ReLU bits [M][C/8] of a BN+ReLU output (read by the backward)
  long M() const { return (long)N * H * W; }
};

struct ConvL {
  std::string name;
  int ci, co, k, stride, rate;
  bool explicit_pad, relu;
  long w_off = 0, g_off = 0, b_off = 0, mv_off = 0;  // flat offsets
  int N = 0, H = 0, W = 0, Ho = 0, Wo = 0, pad_h = 0, pad_w = 0;
  int co_pad = 0;                 // wgrad row padding (co % 8 != 0)
  void* w_lp = nullptr;           // compute-dtype weights [co][k][k][ci]
  void* wt_lp = nullptr;          // flipped transpose [ci][k][k][co] (dgrad)
  bool need_dgrad = true;
  Act x;                          // input of the last forward (not owned)
  Act y, dy;                      // conv output and its gradient
  BnState st{};
  float* stats_part = nullptr;    // [mtiles][co][2]
  float* bwd_part = nullptr;      // [rb][co][2] (group norm: [N][rb][co][2], rb per image)
  int rb = 1;
  // linear BN-backward fold (lbf.h; an identity unit's expansion conv3): per-channel (A, B, D)
  // [3][co] of the last backward, the gated gradient it read (seg_debug_tensor materialises dy
  // from it on request: the step itself never writes dy of such a layer)
  float* lbf_coef = nullptr;
  float* lbf_cs = nullptr;        // [rb of the unit's conv2 BN][ci] column-sum partials of y2
  bool lbf_done = false;          // folded in the last backward
  bool lbf_dy_ready = false;      // ... and dy materialised since (seg_debug_tensor)
  Act lbf_dyhat;
  // group norm: groups, per-image states (host copies of the device array st_dev) and the
  // forward chunk partials
  int groups = 0;
  std::vector<BnState> st_img;
  BnState* st_dev = nullptr;
  float* gn_part = nullptr;
};

enum ShortcutKind { SC_IDENTITY = 0, SC_SUBSAMPLE = 1, SC_CONV = 2 };

struct Unit {
  int sc = -1, c1 = -1, c2 = -1, c3 = -1;
  ShortcutKind kind = SC_IDENTITY;
  int stride = 1;
  Act in, out;        // in is not owned (previous output)
  Act z1, z2;         // post BN+ReLU of conv1/conv2
  Act dz1, dz2, dpre; // gradients; dpre = relu-masked gradient of out (identity/subsample)
  Act dout;           // gradient wrt out (owned)
  // this step's dout was written already ReLU-masked by the next unit's conv1 data gradient
  // (unit_backward): the c3 BN backward reads it without the bits and dout serves as dpre
  bool dout_masked = false;
};

struct Prof {
  bool on = false;
  std::vector<hipEvent_t> ev;
  // gflop: algorithmic work (conv classes) or algorithmic GB (BN classes); gbytes: the
  // launch's compulsory HBM bytes (every operand read / written once) in GB
  struct Rec { int cls; int layer; double gflop; int e0, e1; double gbytes; };
  std::vector<Rec> recs;
  int next = 0;
};

}  // namespace segnet

struct seg_ctx {
  seg_cfg cfg{};
  int device = 0;
  int dt = SEG_BF16;
  size_t esz = 2;
  std::string err;
  std::vector<void*> allocs;
  bool bound = false;
  segnet::Prof prof;

  // parameters
  std::vector<segnet::ConvL> convs;
  long n_train = 0, n_decay = 0, n_moving = 0, n_stats = 0;
  struct PInfo { std::string name; long off, numel; int kind; int dims[4]; };
  std::vector<PInfo> pinfo;
  float* params = nullptr;
  float* grads = nullptr;
  float* mom = nullptr;
  float* ema = nullptr;
  float* moving = nullptr;
  void* w_lp_flat = nullptr;      // bf16 copy of the conv-weight region (bf16 mode)
  FlipJob* flip_jobs = nullptr;   // device table: every dgrad weight flip in one launch
  int n_flip = 0;
  long flip_total = 0;

  // graph
  segnet::Act img;                // compute-dtype images
  int stem = -1;
  // 16-bit stem as a 4 x 4 conv over the space-to-depth image (conv.h): img [N][Ho+3][Wo+3][16],
  // weights [64][256] (stem_wpad); img_dbg = the [N][H][W][8] image view for seg_debug_tensor
  bool stem_s2d = false;
  void* img_dbg = nullptr;
  bf16_t* stem_wpad = nullptr;
  segnet::Act z0, dz0, p0, dp0;
  bool z0_stale = false;   // the fused stem BN + ReLU + max-pool did not store z0 (see forward)
  uint8_t* pool_arg = nullptr;    // max-pool first-max window index per output element
  int pool_ph = 0, pool_pw = 0;
  std::vector<segnet::Unit> units;
  int dfd = -1;
  segnet::Act z_dfd, dz_dfd;      // extension output (pyramid input); may be a slice of concat
  int fov = -1;                   // optional extension/increase_fov conv after decrease_fdims
  segnet::Act z_pre, dz_pre;      // decrease_fdims BN/ReLU output when fov >= 0
  // pyramid
  std::vector<int> pyr_conv;      // per branch conv index
  std::vector<segnet::Act> pooled, dpooled, zb, dzb;
  int pyr_final = -1;
  segnet::Act concat, dconcat;
  segnet::Act feat, dfeat;
  GridSpec pool_grids{};          // avg-pool grids over z_dfd
  std::vector<GridSpec> up_grids; // resize-transpose per branch
  float* grid_part = nullptr;     // [N][Hf][cells][C]
  // heads
  segnet::Unit heads[3];
  int logit_conv[3] = {-1, -1, -1};
  segnet::Act logits;             // fp32 [N][Hl][Wl][ldl]
  float* grad_un = nullptr;       // fp32 same shape (gradient w.r.t. head_in)
  const float* head_in = nullptr; // what the bilinear upsampler reads: logits or up_in
  int ldl = 0, nc[3] = {0, 0, 0};
  bool gn = false;                // norm_layer = group (gn.h)
  float* gn_gscaled = nullptr;    // group norm: the logits gradient times the loss factors
  // 'hybrid' upsampling: per-head 3x3 conv2d_transpose + bias on the logits (deconv.h)
  bool hybrid = false;
  long dc_w_off[3] = {0, 0, 0}, dc_b_off[3] = {0, 0, 0}, dc_b_lo = 0;
  float* up_in = nullptr;         // deconv output [N][Hl][Wl][ldl]
  float* dc_dx = nullptr;         // gradient w.r.t. the logits [N][Hl][Wl][ldl]
  float* dc_part = nullptr;       // weight-gradient tile partials
  // loss
  LossTables tables{};
  float* loss_part = nullptr;
  int loss_blocks = 0;
  float* loss_out = nullptr;      // [10]
  float* dzscale = nullptr;       // [ldl]
  float loss_scale = 1.f;         // gradient seed multiplier (fp16 dynamic loss scaling)
  int64_t loss_yf_launches = 0;   // loss heads run by the y-first kernel (seg_counter)
  // bootstrapped l1 loss (seg_set_bootstrap): percentage (<= 0 off), K of this context's
  // npp * H * W map entries, the per-pixel loss map, the select's slab and device state
  int bs_pct = 0;
  int64_t bs_k = 0;
  float* bs_map = nullptr;         // [npp][H][W]
  unsigned* bs_slab = nullptr;
  BootstrapState* bs_state = nullptr;
  int64_t bootstrap_launches = 0;  // seg_loss calls that ran map + select + gated head (seg_counter)
  // seg_boundary_distance: the row distances g [n][H][W] bytes of the last call, grown on demand
  uint8_t* bd_rows = nullptr;
  size_t bd_rows_bytes = 0;
  // update
  int nesterov = 0;               // MomentumOptimizer use_nesterov (seg_set_nesterov)
  int* skip_flag = nullptr;       // device: non-finite scaled gradients this step (update skipped)
  float* reg_part = nullptr;
  float* reg_out = nullptr;

  // gradient all-reduce buckets in ready order: conv-weight ranges [lo, hi) cut at layer
  // boundaries walking the layers in reverse (the backward's order), then the BN-parameter +
  // batch-statistics tail. An event is recorded on the backward stream as soon as every
  // weight gradient of a bucket has been written, so a collective on another stream can
  // start while the rest of the backward runs.
  std::vector<long> bk_lo, bk_hi;
  std::vector<std::vector<int>> bk_convs;
  std::vector<hipEvent_t> bk_ev;
  std::vector<char> wg_done;
  int bk_next = 0;
  // backward on two streams: every weight gradient runs on `side` (waiting for its layer's
  // dy on the compute stream), so the dgrad -> BN-backward chain and the wgrads overlap
  bool side_on = false;
  bool side_active = false;        // this backward: side_on and not profiling (kernel-alone timing)
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> ev_dy;   // per conv: dy written on the compute stream
  hipEvent_t ev_join = nullptr;
  // seg_set_defer_stem: the backward's compute stream joins the weight-gradient stream before the
  // stem's weight gradient (ev_prestem) instead of after it; seg_apply_update updates every other
  // parameter beside that last kernel and joins (ev_join) before the stem's weights
  hipEvent_t ev_prestem = nullptr;
  bool defer_stem = false;
  bool prestem_rec = false;
  bool stem_pending = false;
  // cross-replica BN (seg_set_bn_sync): per-layer moment exchange through the caller's hook
  seg_allreduce_fn sync_fn = nullptr;
  void* sync_user = nullptr;
  int sync_world = 1;
  float* sync_pack = nullptr;     // [2 * max C]
  int bn_infer = 0;   // seg_set_bn_inference: forward normalises with the moving statistics
  BnInferJob* infer_jobs = nullptr;   // device table: every layer's moving stats -> BnState
  bool premask = true;             // seg_set_premask: pre-masked identity-unit gradients (unit_backward)
  int64_t premask_launches = 0;    // conv1 data gradients stored pre-masked (seg_counter)
  // workspace
  float* slab = nullptr;
  size_t slab_floats = 0;
  // linear BN-backward fold (lbf.h), on unless seg_set_lbf(ctx, 0): 16-bit bottleneck units
  // whose conv3 expands (co >= 2 ci, ci % 64 == 0: every unit of R50). Compute-stream scratch (used in
  // order by one layer at a time): the scaled data-gradient weights, the D-scaled weights, H
  // and its split-K slab, the data gradient's constant; weight-gradient-stream scratch: the
  // two GEMM results and the column-sum partials of the conv input
  bool lbf_on = true;
  void* lbf_wts = nullptr;
  void* lbf_xd = nullptr;
  void* lbf_h = nullptr;
  float* lbf_hslab = nullptr;
  float* lbf_bias = nullptr;
  float* lbf_bpart = nullptr;
  float* lbf_p1 = nullptr;
  int64_t lbf_launches = 0;        // layers folded (seg_counter)
};

namespace segnet {

// ---- errors and allocation ----
inline thread_local std::string g_err;   // the last error of a call without a context

inline int set_err(std::string* dst, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (dst) *dst = buf;
  g_err = buf;
  return code;
}

inline int hip_fail(seg_ctx* c, hipError_t e, const char* where) {
  return set_err(c ? &c->err : nullptr, -EIO, "%s: %s", where, hipGetErrorString(e));
}
#define HIPCALL(c, expr)                                    \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return hip_fail((c), _e, #expr);  \
  } while (0)

inline int dt_of(int abi_dtype) {
  return abi_dtype == SEG_DTYPE_BF16 ? SEG_BF16 : (abi_dtype == SEG_DTYPE_F16 ? SEG_F16 : SEG_F32);
}

template <typename T>
int dalloc(seg_ctx* c, T** p, size_t count) {
  void* q = nullptr;
  size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return hip_fail(c, e, "hipMalloc");
  (void)hipMemset(q, 0, bytes);
  c->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

inline int alloc_act(seg_ctx* c, Act& a, int N, int H, int W, int C, int ld = 0, size_t esz = 0) {
  a.N = N; a.H = H; a.W = W; a.C = C; a.ld = ld ? ld : C;
  size_t e = esz ? esz : c->esz;
  char* p = nullptr;
  int r = dalloc(c, &p, (size_t)a.M() * a.ld * e);
  a.p = p;
  return r;
}

inline Act slice(const seg_ctx* c, const Act& a, int c_off, int C) {
  Act v = a;
  v.p = (char*)a.p + (size_t)c_off * c->esz;
  v.C = C;
  return v;
}

// one image's rows of an activation (img < 0: all of it)
inline Act image_rows(const Act& a, int img, size_t esz) {
  if (img < 0) return a;
  Act v = a;
  const size_t hw = (size_t)a.H * a.W;
  v.p = (char*)a.p + (size_t)img * hw * a.ld * esz;
  if (a.mask) v.mask = a.mask + (size_t)img * hw * (a.C / 8);
  v.N = 1;
  return v;
}

// ---- kernel sequencing ----
struct Step {
  seg_ctx* c;
  hipStream_t s;
  int dt;
};

// One profiled launch: while seg_profile is on (and events remain) the begin event and the
// record {class, layer, work, bytes}, then the launch, then the end event. bytes < 0: the work
// column is the bytes (BN classes). `what` names the launch in an error message; a callable
// that launches more than once under one record moves it on as it goes.
template <typename F>
int profiled(seg_ctx* c, hipStream_t s, int cls, int layer, double gflop, double gbytes,
             const char* const& what, F&& launch) {
  int e1 = -1;
  if (c->prof.on && c->prof.next + 2 <= (int)c->prof.ev.size()) {
    const int e0 = c->prof.next++;
    e1 = c->prof.next++;
    HIPCALL(c, hipEventRecord(c->prof.ev[e0], s));
    c->prof.recs.push_back({cls, layer, gflop, e0, e1, gbytes < 0 ? gflop : gbytes});
  }
  const hipError_t e = launch();
  if (e != hipSuccess) return hip_fail(c, e, what);
  if (e1 >= 0) HIPCALL(c, hipEventRecord(c->prof.ev[e1], s));
  return 0;
}
#define PROFILED(c, s, cls, layer, gflop, gbytes, expr) \
  segnet::profiled((c), (s), (cls), (layer), (gflop), (gbytes), #expr, [&] { return (expr); })

// ---- net_build.cpp ----
int build(seg_ctx* c);
void conv_geom(ConvL& L, int N, int H, int W);
bool lbf_shape_ok(const seg_ctx* c, const Unit& u);
inline int lbf_hsplits(const ConvL& L3) { return std::max(1, L3.co / 128); }   // H: 128 channels per split

// ---- net_layers.cpp: argument builders (shared with the seg_op_conv_* entries) ----
ConvArgs fwd_conv_args(const void* x, int N, int H, int W, int C, int ldx, const void* w, int Co,
                       int k, int stride, int rate, int pad_h, int pad_w, int Ho, int Wo, void* y,
                       int ldy, float* stats);
ConvArgs dgrad_conv_args(const void* dy, int N, int Ho, int Wo, int Co, int lddy, const void* wt,
                         int Ci, int k, int stride, int rate, int pad_h, int pad_w, int H, int W,
                         void* dx, int lddx);
void dgrad_dual_args(ConvArgs& a, const void* dy2, int lddy2, int Co2, const void* wt2);
WgradArgs wgrad_conv_args(const void* dy, int lddy, const void* x, int N, int H, int W, int C, int ldx,
                          int Ho, int Wo, int Co, int k, int stride, int rate, int pad_h, int pad_w,
                          bool s2d = false);
WgradArgs wgrad_problem(const ConvL& L, bool s2d);
int wgrad_splits(const WgradArgs& a, int dt, bool concurrent = false);
// a split-K launch never exceeds the slab it reduces from: per = floats of one split
inline int clamp_splits(long splits, long slab_floats, long per) {
  return (int)std::max<long>(1, std::min<long>(splits, slab_floats / per));
}
BnBwdArgs bn_bwd_args(const ConvL& L, const BnState& st, const Act& y, const Act& dy, const Act& dz);
ConvArgs dgrad_args(seg_ctx* c, int li, const Act& dx, const Act* r1, const Act* r2);
bool dgrad_takes_mask(int dt, ConvArgs& a, const uint8_t* bits);
void mark_premasked(seg_ctx* c, Unit* pred);
bool bn_dual_ok(const seg_ctx* c, const Unit& u);

// ---- net_layers.cpp: per-layer launches ----
int conv_forward(Step& S, int li, const Act& x);
// out = act(bn(y) [+ residual])
int bn_apply(Step& S, int li, const Act& out, int out_f32, const Act* res = nullptr, int rs = 1,
             int li2 = -1, int relu = -1);
int bn_backward(Step& S, int li, const Act& dz, int dz_f32, const Act* z, const Act* dyhat_out,
                const float* dzscale = nullptr, const float* dshift = nullptr,
                bool reduce_only = false, float* cs_out = nullptr);
int bn_backward_dual(Step& S, int li, int li2, const Act& dz, const Act& z, bool second_only = false);
int conv_dgrad(Step& S, int li, const Act& dx, const Act* r1 = nullptr, const Act* r2 = nullptr,
               const uint8_t* omask = nullptr);
int conv_dgrad_dual(Step& S, int li, int li2, const Act& dx, const uint8_t** omask = nullptr);
int conv_wgrad(Step& S, int li, const Act& x);
int bucket_progress(seg_ctx* c, hipStream_t ws, bool final);
bool lbf_ok(seg_ctx* c, const Unit& u, bool in_masked);
int lbf_backward(Step& S, Unit& u, const Act& dyhat);
int lbf_combine(Step& S, Unit& u);

// ---- net_step.cpp ----
int forward(Step& S, const float* images);
int backward(Step& S);
int join_stem(seg_ctx* c, hipStream_t s, bool consume = false);
int refresh_stem_pad(seg_ctx* c, hipStream_t s);
int refresh_compute_weights(seg_ctx* c, hipStream_t s);

}  // namespace segnet
