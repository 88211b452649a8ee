// The C ABI declared in include/seg_hip.h: every entry that takes a context (the context-free
// entries are in api_ops.cpp).
#include "net.h"

using namespace segnet;

extern "C" {

const char* seg_last_error(seg_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int seg_create(int device, const seg_cfg* cfg, seg_ctx** out) {
  if (!cfg || !out) return set_err(nullptr, -EINVAL, "null argument");
  *out = nullptr;
  // host-side validation first: a bad configuration fails the same way with or without a GPU
  if (cfg->dtype < SEG_DTYPE_F32 || cfg->dtype > SEG_DTYPE_F16)
    return set_err(nullptr, -EINVAL, "dtype %d (SEG_DTYPE_F32 / _BF16 / _F16)", cfg->dtype);
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return set_err(nullptr, -ENODEV, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
  seg_ctx* c = new seg_ctx();
  c->cfg = *cfg;
  c->device = device;
  c->dt = dt_of(cfg->dtype);
  c->esz = seg_half(c->dt) ? 2 : 4;
  int r = build(c);
  if (!r && c->dt == SEG_F16) r = seg_set_loss_scale(c, 1.f);   // overflow flag of fp16 steps
  if (r) {
    std::string msg = c->err;
    seg_destroy(c);
    return set_err(nullptr, r, "%s", msg.c_str());
  }
  *out = c;
  return 0;
}

int seg_destroy(seg_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->side) (void)hipStreamSynchronize(c->side);   // a deferred stem weight gradient
  (void)hipDeviceSynchronize();
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->infer_jobs) (void)hipFree(c->infer_jobs);
  if (c->bd_rows) (void)hipFree(c->bd_rows);
  for (auto ev : c->prof.ev) (void)hipEventDestroy(ev);
  for (auto ev : c->bk_ev) (void)hipEventDestroy(ev);
  for (auto ev : c->ev_dy) (void)hipEventDestroy(ev);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_prestem) (void)hipEventDestroy(c->ev_prestem);
  if (c->side) (void)hipStreamDestroy(c->side);
  delete c;
  return 0;
}

int seg_sizes(seg_ctx* c, int64_t* n_train, int64_t* n_decay, int64_t* n_moving, int64_t* n_stats) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (n_train) *n_train = c->n_train;
  if (n_decay) *n_decay = c->n_decay;
  if (n_moving) *n_moving = c->n_moving;
  if (n_stats) *n_stats = c->n_stats;
  return 0;
}

int seg_bind_buffers(seg_ctx* c, float* params, float* grads, float* momentum, float* ema,
                     float* moving) {
  if (!c || !params || !grads || !momentum || !moving)
    return set_err(c ? &c->err : nullptr, -EINVAL, "params/grads/momentum/moving required");
  c->params = params; c->grads = grads; c->mom = momentum; c->ema = ema; c->moving = moving;
  const long half = c->n_moving / 2;
  for (auto& L : c->convs) {
    if (c->dt == SEG_F32) L.w_lp = params + L.w_off;
    // batch statistics land directly in the gradient tail (one all-reduce covers them)
    L.st.mean = grads + c->n_train + L.mv_off;
    L.st.var_unb = grads + c->n_train + half + L.mv_off;
  }
  // the batched flip table needs the compute-weight pointers (fp32: the bound params)
  std::vector<FlipJob> jobs;
  long tot = 0;
  for (auto& L : c->convs)
    if (L.wt_lp) {
      jobs.push_back({L.w_lp, L.wt_lp, L.co, L.k, L.ci, tot});
      tot += flip_tiles(L.co, L.k, L.ci);
    }
  c->n_flip = (int)jobs.size();
  c->flip_total = tot;
  if (c->n_flip) {
    if (!c->flip_jobs)
      if (int r = dalloc(c, &c->flip_jobs, jobs.size())) return r;
    HIPCALL(c, hipMemcpy(c->flip_jobs, jobs.data(), jobs.size() * sizeof(FlipJob), hipMemcpyHostToDevice));
  }
  c->bound = true;
  return 0;
}

int64_t seg_param_count(seg_ctx* c) { return c ? (int64_t)c->pinfo.size() : -1; }

int seg_param_info(seg_ctx* c, int64_t i, const char** name, int64_t* offset, int64_t* numel,
                   int* kind) {
  if (!c || i < 0 || i >= (int64_t)c->pinfo.size()) return set_err(c ? &c->err : nullptr, -EINVAL, "bad index");
  const auto& p = c->pinfo[i];
  if (name) *name = p.name.c_str();
  if (offset) *offset = p.off;
  if (numel) *numel = p.numel;
  if (kind) *kind = p.kind;
  return 0;
}

int seg_param_shape(seg_ctx* c, int64_t i, int64_t* dims) {
  if (!c || !dims || i < 0 || i >= (int64_t)c->pinfo.size())
    return set_err(c ? &c->err : nullptr, -EINVAL, "bad index");
  for (int k = 0; k < 4; ++k) dims[k] = c->pinfo[i].dims[k];
  return 0;
}

#define NEED_BOUND(c) \
  if (!(c) || !(c)->bound) return set_err((c) ? &(c)->err : nullptr, -EINVAL, "context not bound")

int seg_params_updated(seg_ctx* c, void* stream) {
  NEED_BOUND(c);
  if (int r = join_stem(c, (hipStream_t)stream)) return r;
  return refresh_compute_weights(c, (hipStream_t)stream);
}

int seg_forward(seg_ctx* c, const float* images, void* stream) {
  NEED_BOUND(c);
  if (!images) return set_err(&c->err, -EINVAL, "images required");
  Step S{c, (hipStream_t)stream, c->dt};
  if (int r = join_stem(c, S.s)) return r;
  return forward(S, images);
}

int seg_loss(seg_ctx* c, const int32_t* px, const float* bbox, const float* tag, int32_t* decisions,
             void* stream) {
  NEED_BOUND(c);
  if (int r = join_stem(c, (hipStream_t)stream)) return r;
  const seg_cfg& g = c->cfg;
  if ((g.nb_pp && !px) || (g.nb_pb && !bbox) || (g.nb_pi && !tag))
    return set_err(&c->err, -EINVAL, "missing labels for a non-empty sub-batch");
  LossArgs a{};
  a.logits = c->head_in; a.N = c->logits.N; a.Hl = c->logits.H; a.Wl = c->logits.W;
  a.ldl = c->ldl; a.H = g.height; a.W = g.width;
  a.npp = g.nb_pp; a.npb = g.nb_pb; a.npi = g.nb_pi;
  a.px_labels = px; a.bbox_soft = bbox; a.tag_soft = tag;
  a.grad_un = c->grad_un; a.part = c->loss_part; a.decisions = decisions;
  hipStream_t s = (hipStream_t)stream;
  if (c->bs_pct > 0 && g.nb_pp > 0) {   // bootstrapped l1: map -> K-th largest -> gated head
    HIPCALL(c, launch_l1_loss_map(a, c->tables, c->bs_map, s));
    HIPCALL(c, launch_bootstrap_select(c->bs_map, (long long)g.nb_pp * g.height * g.width, c->bs_k,
                                       c->bs_slab, c->bs_state, s));
    a.l1_map = c->bs_map;
    a.tau = &c->bs_state->tau;
    ++c->bootstrap_launches;
  }
  HIPCALL(c, launch_loss_head(a, c->tables, s));
  if (c->tables.c1 == 14 && loss_head_yf(a.W, a.Wl)) ++c->loss_yf_launches;
  HIPCALL(c, launch_loss_finalize(c->loss_part, c->loss_blocks, c->tables, c->ldl, c->loss_scale,
                                  c->loss_out, c->dzscale, s));
  return 0;
}

int seg_set_bn_inference(seg_ctx* c, int on) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (c->gn) return 0;   // group norm normalises every image by its own statistics in all modes
  if (on) {   // (re)build the per-layer job table from the bound buffers (outside any step)
    NEED_BOUND(c);
    std::vector<BnInferJob> jobs;
    const long half = c->n_moving / 2;
    for (const ConvL& L : c->convs)
      jobs.push_back({c->moving + L.mv_off, c->moving + half + L.mv_off, c->params + L.g_off,
                      L.st, L.co});
    if (!c->infer_jobs) {
      HIPCALL(c, hipMalloc(&c->infer_jobs, jobs.size() * sizeof(BnInferJob)));
    }
    HIPCALL(c, hipMemcpy(c->infer_jobs, jobs.data(), jobs.size() * sizeof(BnInferJob),
                         hipMemcpyHostToDevice));
  }
  c->bn_infer = on ? 1 : 0;
  return 0;
}

// "who: " in front of the messages of the entries that name themselves in their errors
static std::string prefix(const char* who) { return who ? std::string(who) + ": " : std::string(); }

static int check_aligned16(seg_ctx* c, const char* who, const void* p, const char* name) {
  if (reinterpret_cast<uintptr_t>(p) & 15)
    return set_err(&c->err, -EINVAL, "%s%s must be 16-byte aligned", prefix(who).c_str(), name);
  return 0;
}

// What the four decision entries (seg_predict, seg_tta_decisions, seg_window_decisions,
// seg_crf_decisions) ask of the two pointers, replace_voids, the cid map and the output size.
// max_rv: the highest replace_voids mode of the entry (2 for seg_predict, else 1); kind: what its
// probabilities are ("averaged", "refined") in the refusal of mode 2. Writes the map of
// utils._replacevoids (-1 -> max + 1; anything below -1 is refused) to map.
static int check_decision_args(seg_ctx* c, const char* who, int max_rv, const char* kind,
                               int replace_voids, const int32_t* cid_map, int n_map, int out_h,
                               int out_w, const int32_t* decisions_out, int* map) {
  const std::string pre = prefix(who);
  std::string* err = &c->err;
  if (!cid_map) return set_err(err, -EINVAL, "%snull cid_map", pre.c_str());
  if (!decisions_out) return set_err(err, -EINVAL, "%snull decisions_out", pre.c_str());
  if (replace_voids == 2 && max_rv < 2)
    return set_err(err, -EINVAL, "%sreplace_voids = 2 (the PREDICT order on resized "
                   "probabilities) is not defined for %s probabilities; use 1", pre.c_str(), kind);
  if (replace_voids < 0 || replace_voids > max_rv)
    return set_err(err, -EINVAL, "%sreplace_voids = %d (%s)", pre.c_str(), replace_voids,
                   max_rv == 2 ? "0, 1 or 2" : "0 or 1");
  if (n_map != c->tables.n_pp)
    return set_err(err, -EINVAL, "%scid_map has %d entries, the model has %d training classes",
                   pre.c_str(), n_map, c->tables.n_pp);
  if (out_h < 1 || out_w < 1)
    return set_err(err, -EINVAL, "%sbad output size out_h x out_w = %dx%d", pre.c_str(), out_h, out_w);
  int mx = -1;
  for (int i = 0; i < n_map; ++i) mx = std::max(mx, (int)cid_map[i]);
  for (int i = 0; i < n_map; ++i) {
    if (cid_map[i] < -1)
      return set_err(err, -EINVAL, "%scid_map[%d] = %d", pre.c_str(), i, cid_map[i]);
    map[i] = cid_map[i] == -1 ? mx + 1 : cid_map[i];
  }
  return 0;
}

// mean_probs_out of the multi-entry heads needs the output to have the size the probabilities are
// averaged at: avg_h x avg_w, "the <avg_name> size" in the message.
static int check_mean_probs_out(seg_ctx* c, const char* who, const float* mean_probs_out, int out_h,
                                int out_w, const char* avg_name, int avg_h, int avg_w) {
  if (mean_probs_out && (out_h != avg_h || out_w != avg_w))
    return set_err(&c->err, -EINVAL, "%s: mean_probs_out needs the output size %dx%d to be the "
                   "%s size %dx%d", who, out_h, out_w, avg_name, avg_h, avg_w);
  return check_aligned16(c, who, mean_probs_out, "mean_probs_out");
}

int seg_predict(seg_ctx* c, const int32_t* cid_map, int n_map, int replace_voids, int out_h,
                int out_w, int32_t* decisions_out, void* stream) {
  NEED_BOUND(c);
  if (int r = join_stem(c, (hipStream_t)stream)) return r;
  const seg_cfg& g = c->cfg;
  EvalArgs a{};
  if (int r = check_decision_args(c, nullptr, 2, "", replace_voids, cid_map, n_map, out_h, out_w,
                                  decisions_out, a.map))
    return r;
  a.logits = c->head_in; a.N = c->logits.N; a.Hl = c->logits.H; a.Wl = c->logits.W;
  a.ldl = c->ldl; a.H = g.height; a.W = g.width; a.Ho = out_h; a.Wo = out_w;
  a.replace_voids = replace_voids; a.n_map = n_map; a.out = decisions_out;
  HIPCALL(c, launch_eval_decisions(a, c->tables, (hipStream_t)stream));
  return 0;
}

int seg_full_predictions(seg_ctx* c, float* logits_out, float* probs_out,
                         int32_t* head_decisions_out, int32_t* decisions_out, void* stream) {
  NEED_BOUND(c);
  if (int r = join_stem(c, (hipStream_t)stream)) return r;
  FullPredArgs a{};
  a.logits = c->head_in; a.N = c->logits.N; a.Hl = c->logits.H; a.Wl = c->logits.W;
  a.ldl = c->ldl; a.H = c->cfg.height; a.W = c->cfg.width;
  a.logits_out = logits_out; a.probs_out = probs_out;
  a.head_decs_out = head_decisions_out; a.decs_out = decisions_out;
  if (int r = check_aligned16(c, nullptr, logits_out, "logits_out")) return r;
  if (int r = check_aligned16(c, nullptr, probs_out, "probs_out")) return r;
  HIPCALL(c, launch_full_predictions(a, c->tables, (hipStream_t)stream));
  return 0;
}

int seg_tta_decisions(seg_ctx* c, const seg_tta_entry* entries, int n_entries,
                      const int32_t* cid_map, int n_map, int replace_voids, int out_h, int out_w,
                      float* mean_probs_out, int32_t* decisions_out, void* stream) {
  const char* who = "seg_tta_decisions";
  if (!c) return set_err(nullptr, -EINVAL, "%s: null ctx", who);
  if (!entries) return set_err(&c->err, -EINVAL, "%s: null entries", who);
  if (n_entries < 1 || n_entries > SEG_TTA_MAX_ENTRIES)
    return set_err(&c->err, -EINVAL, "%s: %d entries (1..%d)", who, n_entries, SEG_TTA_MAX_ENTRIES);
  static_assert(SEG_TTA_MAX_ENTRIES == TTA_MAX_ENTRIES, "entry table size");
  const seg_cfg& g = c->cfg;
  const LossTables& t = c->tables;
  const int ct = t.c1 + t.c2 + t.c3;
  TtaArgs a{};
  if (int r = check_decision_args(c, who, 1, "averaged", replace_voids, cid_map, n_map, out_h, out_w,
                                  decisions_out, a.map))
    return r;
  if (int r = check_mean_probs_out(c, who, mean_probs_out, out_h, out_w, "network", g.height, g.width))
    return r;
  for (int i = 0; i < n_entries; ++i) {
    const seg_tta_entry& e = entries[i];
    if (!e.logits) return set_err(&c->err, -EINVAL, "%s: entry %d: null logits", who, i);
    if (e.h_low < 1 || e.w_low < 1)
      return set_err(&c->err, -EINVAL, "%s: entry %d: low-resolution size %dx%d", who, i, e.h_low, e.w_low);
    if (e.ld < ct)
      return set_err(&c->err, -EINVAL, "%s: entry %d: pixel stride %d < %d channels", who, i, e.ld, ct);
    if (e.flip < 0 || e.flip > 1)
      return set_err(&c->err, -EINVAL, "%s: entry %d: flip = %d (0 or 1)", who, i, e.flip);
    a.e[i] = TtaEntry{e.logits, e.h_low, e.w_low, e.ld, e.flip};
  }
  a.n_entries = n_entries;
  a.inv_e = 1.0f / (float)n_entries;
  a.N = c->logits.N; a.H = g.height; a.W = g.width; a.Ho = out_h; a.Wo = out_w;
  a.replace_voids = replace_voids; a.n_map = n_map;
  a.probs = mean_probs_out; a.out = decisions_out;
  HIPCALL(c, launch_tta_decisions(a, t, (hipStream_t)stream));
  return 0;
}

int seg_window_decisions(seg_ctx* c, const float* const* logits, int h_low, int w_low, int ld,
                         const int* ys, int ny, const int* xs, int nx, int flip,
                         int canvas_h, int canvas_w, const int32_t* cid_map, int n_map,
                         int replace_voids, int out_h, int out_w,
                         float* mean_probs_out, int32_t* decisions_out, void* stream) {
  const char* who = "seg_window_decisions";
  if (!c) return set_err(nullptr, -EINVAL, "%s: null ctx", who);
  if (!logits || !ys || !xs) return set_err(&c->err, -EINVAL, "%s: null logits / ys / xs", who);
  if (ny < 1 || nx < 1)
    return set_err(&c->err, -EINVAL, "%s: %d x %d windows (at least 1 x 1)", who, ny, nx);
  if (flip < 0 || flip > 1) return set_err(&c->err, -EINVAL, "%s: flip = %d (0 or 1)", who, flip);
  static_assert(SEG_WIN_MAX_ENTRIES == WIN_MAX_ENTRIES, "entry table size");
  const long n_entries = (long)ny * nx * (1 + flip);
  if (n_entries > SEG_WIN_MAX_ENTRIES)
    return set_err(&c->err, -EINVAL, "%s: %d x %d windows%s are %ld entries (1..%d)", who, ny, nx,
                   flip ? " with flip" : "", n_entries, SEG_WIN_MAX_ENTRIES);
  const seg_cfg& g = c->cfg;
  const LossTables& t = c->tables;
  const int ct = t.c1 + t.c2 + t.c3;
  if (h_low < 1 || w_low < 1)
    return set_err(&c->err, -EINVAL, "%s: low-resolution size %dx%d", who, h_low, w_low);
  if (ld < ct) return set_err(&c->err, -EINVAL, "%s: pixel stride %d < %d channels", who, ld, ct);
  if (canvas_h < g.height || canvas_w < g.width)
    return set_err(&c->err, -EINVAL, "%s: the canvas %dx%d is smaller than the network size %dx%d",
                   who, canvas_h, canvas_w, g.height, g.width);
  // strictly increasing from 0, no gap, the last window flush with the edge: every canvas pixel
  // is covered, and every window lies inside the canvas
  auto origins = [&](const char* name, const int* o, int n, int len, int canvas) {
    if (o[0] != 0) return set_err(&c->err, -EINVAL, "%s: %s[0] = %d (must be 0)", who, name, o[0]);
    for (int i = 0; i + 1 < n; ++i) {
      if (o[i + 1] <= o[i])
        return set_err(&c->err, -EINVAL, "%s: %s[%d] = %d after %d: origins must increase strictly",
                       who, name, i + 1, o[i + 1], o[i]);
      if (o[i + 1] > o[i] + len)
        return set_err(&c->err, -EINVAL, "%s: %s[%d] = %d leaves a gap after the window at %d of "
                       "length %d", who, name, i + 1, o[i + 1], o[i], len);
    }
    if ((long)o[n - 1] + len != canvas)
      return set_err(&c->err, -EINVAL, "%s: the last window %s[%d] = %d of length %d does not end "
                     "at the canvas edge %d", who, name, n - 1, o[n - 1], len, canvas);
    return 0;
  };
  if (int rc = origins("ys", ys, ny, g.height, canvas_h)) return rc;
  if (int rc = origins("xs", xs, nx, g.width, canvas_w)) return rc;
  WinArgs a{};
  if (int r = check_decision_args(c, who, 1, "averaged", replace_voids, cid_map, n_map, out_h, out_w,
                                  decisions_out, a.map))
    return r;
  if (int r = check_mean_probs_out(c, who, mean_probs_out, out_h, out_w, "canvas", canvas_h, canvas_w))
    return r;
  for (int i = 0; i < (int)n_entries; ++i) {
    if (!logits[i]) return set_err(&c->err, -EINVAL, "%s: entry %d: null logits", who, i);
    a.logits[i] = logits[i];
  }
  for (int i = 0; i < ny; ++i) a.ys[i] = ys[i];
  for (int i = 0; i < nx; ++i) a.xs[i] = xs[i];
  for (int k = 1; k <= WIN_MAX_ENTRIES; ++k) a.rk[k] = 1.0f / (float)k;   // host IEEE division
  a.ny = ny; a.nx = nx; a.flip = flip;
  a.hl = h_low; a.wl = w_low; a.ld = ld;
  a.N = c->logits.N; a.H = g.height; a.W = g.width; a.Hc = canvas_h; a.Wc = canvas_w;
  a.Ho = out_h; a.Wo = out_w;
  a.replace_voids = replace_voids; a.n_map = n_map;
  a.probs = mean_probs_out; a.out = decisions_out;
  HIPCALL(c, launch_window_decisions(a, t, (hipStream_t)stream));
  return 0;
}

// one Q buffer of the mean-field iteration, rounded up to the 16-byte alignment the kernels ask
static int64_t crf_buffer_bytes(int n, int H, int W, int ct) {
  return ((int64_t)n * H * W * ct * (int64_t)sizeof(float) + 15) / 16 * 16;
}

int seg_crf_workspace(int n, int H, int W, int ct, int64_t* bytes) {
  if (!bytes || n < 1 || H < 1 || W < 1 || ct < 1)
    return set_err(nullptr, -EINVAL, "seg_crf_workspace: bad arguments (n %d, H %d, W %d, ct %d%s)",
                   n, H, W, ct, bytes ? "" : ", null bytes");
  *bytes = 2 * crf_buffer_bytes(n, H, W, ct);
  return 0;
}

int seg_crf_decisions(seg_ctx* c, const float* probs, const float* images, int n, int H, int W,
                      const seg_crf_params* p, void* workspace, int64_t workspace_bytes,
                      const int32_t* cid_map, int n_map, int replace_voids, int out_h, int out_w,
                      float* probs_out, int32_t* decisions_out, void* stream) {
  const char* who = "seg_crf_decisions";
  if (!c) return set_err(nullptr, -EINVAL, "%s: null ctx", who);
  std::string* err = &c->err;
  if (!probs) return set_err(err, -EINVAL, "%s: null probs", who);
  if (!images) return set_err(err, -EINVAL, "%s: null images", who);
  if (!p) return set_err(err, -EINVAL, "%s: null params (seg_crf_params)", who);
  if (n < 1 || H < 1 || W < 1)
    return set_err(err, -EINVAL, "%s: bad size n = %d, H = %d, W = %d", who, n, H, W);
  if (p->iterations < 0 || p->iterations > CRF_MAX_ITERATIONS)
    return set_err(err, -EINVAL, "%s: iterations = %d (0..%d)", who, p->iterations, CRF_MAX_ITERATIONS);
  if (p->radius < 1 || p->radius > CRF_MAX_RADIUS)
    return set_err(err, -EINVAL, "%s: radius = %d (1..%d)", who, p->radius, CRF_MAX_RADIUS);
  if (p->dilation < 1 || p->dilation > CRF_MAX_DILATION)
    return set_err(err, -EINVAL, "%s: dilation = %d (1..%d)", who, p->dilation, CRF_MAX_DILATION);
  const struct { const char* name; float v; bool weight; } fl[] = {
      {"w_appearance", p->w_appearance, true}, {"w_smoothness", p->w_smoothness, true},
      {"theta_alpha", p->theta_alpha, false},  {"theta_beta", p->theta_beta, false},
      {"theta_gamma", p->theta_gamma, false}};
  for (const auto& f : fl) {
    if (!std::isfinite(f.v)) return set_err(err, -EINVAL, "%s: %s is not finite", who, f.name);
    if (f.weight ? f.v < 0.f : f.v <= 0.f)
      return set_err(err, -EINVAL, "%s: %s = %g (must be %s 0)", who, f.name, (double)f.v,
                     f.weight ? ">=" : ">");
  }
  const LossTables& t = c->tables;
  const int ct = t.c1 + t.c2 + t.c3;
  CrfDecideArgs da{};
  if (int r = check_decision_args(c, who, 1, "refined", replace_voids, cid_map, n_map, out_h, out_w,
                                  decisions_out, da.map))
    return r;
  if (int r = check_aligned16(c, who, probs, "probs")) return r;
  if (int r = check_aligned16(c, who, probs_out, "probs_out")) return r;
  const int T = p->iterations;
  const int64_t buf = crf_buffer_bytes(n, H, W, ct);
  if (T >= 1) {
    if (!workspace) return set_err(err, -EINVAL, "%s: null workspace with iterations = %d", who, T);
    if (int r = check_aligned16(c, who, workspace, "workspace")) return r;
    if (workspace_bytes < 2 * buf)
      return set_err(err, -EINVAL, "%s: workspace of %lld bytes, %lld needed (seg_crf_workspace)",
                     who, (long long)workspace_bytes, (long long)(2 * buf));
  }

  hipStream_t s = (hipStream_t)stream;
  const float* q = probs;   // Q^0 = P
  if (T >= 1) {
    CrfStepArgs a{};
    a.p = probs; a.img = images; a.N = n; a.H = H; a.W = W;
    a.r = p->radius; a.d = p->dilation;
    const double sb = (double)p->theta_beta * 2.0 / 255.0;   // one grey level of the prepared image
    a.inv2b = (float)(1.0 / (2.0 * sb * sb));
    int o = 0;
    for (int dy = -a.r; dy <= a.r; ++dy)
      for (int dx = -a.r; dx <= a.r; ++dx, ++o) {
        if (!dy && !dx) continue;   // the centre is no offset: both tables keep 0 there
        const double d2 = ((double)dy * dy + (double)dx * dx) * a.d * a.d;
        a.ga[o] = (float)((double)p->w_appearance *
                          std::exp(-d2 / (2.0 * (double)p->theta_alpha * (double)p->theta_alpha)));
        a.gs[o] = (float)((double)p->w_smoothness *
                          std::exp(-d2 / (2.0 * (double)p->theta_gamma * (double)p->theta_gamma)));
      }
    float* ws[2] = {static_cast<float*>(workspace),
                    reinterpret_cast<float*>(static_cast<char*>(workspace) + buf)};
    for (int it = 0; it < T; ++it) {
      a.q = q;
      a.out = (it == T - 1 && probs_out) ? probs_out : ws[it & 1];
      HIPCALL(c, launch_crf_step(a, t, s));
      q = a.out;
    }
  } else if (probs_out) {
    HIPCALL(c, hipMemcpyAsync(probs_out, probs, (size_t)n * H * W * ct * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
  }
  da.q = q; da.N = n; da.H = H; da.W = W; da.Ho = out_h; da.Wo = out_w;
  da.replace_voids = replace_voids; da.n_map = n_map; da.out = decisions_out;
  HIPCALL(c, launch_crf_decisions(da, t, s));
  return 0;
}

// What the three box-label entries (seg_box_constrain, seg_box_decisions, seg_box_finalize) ask of
// the context, the size and the box lists; fills b.
static int check_box_args(seg_ctx* c, const char* who, int n, int H, int W, const float* boxes,
                          const int32_t* cids, const int32_t* box_off, const int32_t* geom,
                          int max_boxes, BoxListArgs* b) {
  if (!c) return set_err(nullptr, -EINVAL, "%s: null ctx", who);
  std::string* err = &c->err;
  if (!boxes) return set_err(err, -EINVAL, "%s: null boxes", who);
  if (!cids) return set_err(err, -EINVAL, "%s: null cids", who);
  if (!box_off) return set_err(err, -EINVAL, "%s: null box_off", who);
  if (!geom) return set_err(err, -EINVAL, "%s: null geom", who);
  if (n < 1 || n > 65535 || H < 1 || W < 1)
    return set_err(err, -EINVAL, "%s: bad size n = %d, H = %d, W = %d", who, n, H, W);
  if (max_boxes < 0 || max_boxes > BOXLABEL_MAX_BOXES)
    return set_err(err, -EINVAL, "%s: max_boxes = %d (0..%d boxes per image)", who, max_boxes,
                   BOXLABEL_MAX_BOXES);
  static_assert(sizeof(BboxGeom) == 6 * sizeof(int32_t), "geom layout");
  *b = BoxListArgs{boxes, cids, box_off, reinterpret_cast<const BboxGeom*>(geom)};
  return 0;
}

int seg_box_kinds(seg_ctx* c, int32_t* kinds) {
  const char* who = "seg_box_kinds";
  if (!c) return set_err(nullptr, -EINVAL, "%s: null ctx", who);
  if (!kinds) return set_err(&c->err, -EINVAL, "%s: null kinds", who);
  const LossTables& t = c->tables;
  for (int k = 0; k < SEG_WEAK_CLASSES - 1; ++k)
    kinds[k] = t.pb2veh[k] != t.c2 - 1 ? 1 : t.pb2hum[k] != t.c3 - 1 ? 2 : 0;
  return 0;
}

int seg_box_constrain(seg_ctx* c, const float* probs, int n, int H, int W, const float* boxes,
                      const int32_t* cids, const int32_t* box_off, const int32_t* geom,
                      int max_boxes, float* probs_out, uint16_t* mask_out, void* stream) {
  const char* who = "seg_box_constrain";
  BoxConstrainArgs a{};
  if (int r = check_box_args(c, who, n, H, W, boxes, cids, box_off, geom, max_boxes, &a.b)) return r;
  if (!probs) return set_err(&c->err, -EINVAL, "%s: null probs", who);
  if (!probs_out) return set_err(&c->err, -EINVAL, "%s: null probs_out", who);
  if (int r = check_aligned16(c, who, probs, "probs")) return r;
  if (int r = check_aligned16(c, who, probs_out, "probs_out")) return r;
  if (probs_out == probs) return set_err(&c->err, -EINVAL, "%s: probs_out must not be probs", who);
  a.p = probs; a.N = n; a.H = H; a.W = W; a.out = probs_out; a.mask = mask_out;
  HIPCALL(c, launch_box_constrain(a, c->tables, (hipStream_t)stream));
  return 0;
}

int seg_box_decisions(seg_ctx* c, const float* q, int n, int H, int W, const float* boxes,
                      const int32_t* cids, const int32_t* box_off, const int32_t* geom,
                      int max_boxes, float tau, int32_t* labels_out, float* conf_out,
                      int32_t* counts_out, void* stream) {
  const char* who = "seg_box_decisions";
  BoxDecideArgs a{};
  if (int r = check_box_args(c, who, n, H, W, boxes, cids, box_off, geom, max_boxes, &a.b)) return r;
  if (!q) return set_err(&c->err, -EINVAL, "%s: null q", who);
  if (!labels_out) return set_err(&c->err, -EINVAL, "%s: null labels_out", who);
  if (!counts_out) return set_err(&c->err, -EINVAL, "%s: null counts_out", who);
  if (int r = check_aligned16(c, who, q, "q")) return r;
  if (!std::isfinite(tau) || tau < 0.f || tau > 1.f)
    return set_err(&c->err, -EINVAL, "%s: tau = %g (a finite value in [0, 1])", who, (double)tau);
  a.q = q; a.N = n; a.H = H; a.W = W; a.max_boxes = max_boxes; a.tau = tau;
  a.labels = labels_out; a.conf = conf_out; a.counts = counts_out;
  HIPCALL(c, launch_box_decisions(a, c->tables, (hipStream_t)stream));
  return 0;
}

int seg_box_finalize(seg_ctx* c, const int32_t* labels, int n, int H, int W, const float* boxes,
                     const int32_t* cids, const int32_t* box_off, const int32_t* geom,
                     int max_boxes, const int32_t* reject, int out_h, int out_w, int32_t* out,
                     void* stream) {
  const char* who = "seg_box_finalize";
  BoxFinalizeArgs a{};
  if (int r = check_box_args(c, who, n, H, W, boxes, cids, box_off, geom, max_boxes, &a.b)) return r;
  if (!labels) return set_err(&c->err, -EINVAL, "%s: null labels", who);
  if (!reject) return set_err(&c->err, -EINVAL, "%s: null reject", who);
  if (!out) return set_err(&c->err, -EINVAL, "%s: null out", who);
  if (out_h < 1 || out_w < 1)
    return set_err(&c->err, -EINVAL, "%s: bad output size out_h x out_w = %dx%d", who, out_h, out_w);
  a.labels = labels; a.reject = reject; a.N = n; a.H = H; a.W = W; a.Ho = out_h; a.Wo = out_w;
  a.out = out;
  HIPCALL(c, launch_box_finalize(a, c->tables, (hipStream_t)stream));
  return 0;
}

int seg_backward(seg_ctx* c, void* stream) {
  NEED_BOUND(c);
  Step S{c, (hipStream_t)stream, c->dt};
  if (int r = join_stem(c, S.s, true)) return r;
  return backward(S);
}

int seg_apply_update(seg_ctx* c, float lr, float momentum, float ema_decay_eff, float grad_scale,
                     void* stream) {
  NEED_BOUND(c);
  hipStream_t s = (hipStream_t)stream;
  const ConvL& stl = c->convs[c->stem];
  const long st_lo = stl.w_off, st_hi = stl.w_off + (long)stl.co * stl.k * stl.k * stl.ci;
  // deferred stem (seg_set_defer_stem): every parameter but the stem's conv weights is updated
  // while the stem's weight gradient still runs on the weight-gradient stream; not with loss
  // scaling (one overflow check covers all gradients) or a gradient scale (the all-reduce path)
  const bool split = c->stem_pending && !c->skip_flag && grad_scale == 1.f && !stl.wt_lp &&
                     st_hi <= c->n_decay;
  if (!split)
    if (int r = join_stem(c, s, true)) return r;
  if (c->skip_flag) {   // loss-scaled (fp16) step: unscale, and skip it if anything overflowed
    HIPCALL(c, hipMemsetAsync(c->skip_flag, 0, sizeof(int), s));
    HIPCALL(c, launch_nonfinite(c->grads, c->n_train, c->skip_flag, s));
    HIPCALL(c, launch_scale2(c->grads, c->n_train, grad_scale / c->loss_scale, c->n_stats, grad_scale, s));
  } else if (grad_scale != 1.f) {
    HIPCALL(c, launch_scale_inplace(c->grads, c->n_train + c->n_stats, grad_scale, s));
  }
  SgdmArgs a{};
  a.w = c->params; a.g = c->grads; a.v = c->mom;
  a.ema = ema_decay_eff > 0.f ? c->ema : nullptr;
  a.w_lp = seg_half(c->dt) ? c->w_lp_flat : nullptr;
  a.lp_f16 = c->dt == SEG_F16;
  a.skip = c->skip_flag;
  a.n = c->n_decay; a.lr = lr; a.momentum = momentum; a.wd = c->cfg.weight_decay;
  a.ema_decay = ema_decay_eff; a.reg_part = c->reg_part; a.nesterov = c->nesterov;
  int nparts = sgdm_blocks(c->n_decay);
  SgdmArgs st_a = a;   // the stem's range (split): [st_lo, st_hi), partials after the others'
  if (split) {
    // [0, st_lo) and [st_hi, n_decay) now, partials packed in that order, then the stem's
    SgdmArgs r0 = a, r1 = a;
    r0.n = st_lo;
    r1.w = a.w + st_hi; r1.g = a.g + st_hi; r1.v = a.v + st_hi;
    r1.ema = a.ema ? a.ema + st_hi : nullptr;
    r1.w_lp = a.w_lp ? (char*)a.w_lp + st_hi * c->esz : nullptr;
    r1.n = c->n_decay - st_hi;
    r1.reg_part = a.reg_part + sgdm_blocks(r0.n);
    HIPCALL(c, launch_sgdm(r0, s));
    HIPCALL(c, launch_sgdm(r1, s));
    st_a.w = a.w + st_lo; st_a.g = a.g + st_lo; st_a.v = a.v + st_lo;
    st_a.ema = a.ema ? a.ema + st_lo : nullptr;
    st_a.w_lp = a.w_lp ? (char*)a.w_lp + st_lo * c->esz : nullptr;
    st_a.n = st_hi - st_lo;
    st_a.reg_part = r1.reg_part + sgdm_blocks(r1.n);
    nparts = sgdm_blocks(r0.n) + sgdm_blocks(r1.n) + sgdm_blocks(st_a.n);
  } else {
    HIPCALL(c, launch_sgdm(a, s));
    HIPCALL(c, launch_sum_partials(c->reg_part, nparts, c->reg_out, s));
  }
  if (c->cfg.train_bn) {
    SgdmArgs b = a;
    b.w = c->params + c->n_decay; b.g = c->grads + c->n_decay; b.v = c->mom + c->n_decay;
    b.ema = a.ema ? c->ema + c->n_decay : nullptr; b.w_lp = nullptr; b.n = c->n_train - c->n_decay;
    b.wd = 0.f; b.reg_part = nullptr;
    HIPCALL(c, launch_sgdm(b, s));
  } else if (c->hybrid) {   // frozen BN parameters: the deconv biases still train
    SgdmArgs b = a;
    b.w = c->params + c->dc_b_lo; b.g = c->grads + c->dc_b_lo; b.v = c->mom + c->dc_b_lo;
    b.ema = a.ema ? c->ema + c->dc_b_lo : nullptr; b.w_lp = nullptr; b.n = c->n_train - c->dc_b_lo;
    b.wd = 0.f; b.reg_part = nullptr;
    HIPCALL(c, launch_sgdm(b, s));
  }
  const long half = c->n_moving / 2;
  // group norm keeps no moving statistics; a moving-statistics (frozen) step updates none
  if (!c->gn && !c->bn_infer)
    HIPCALL(c, launch_moving_update(c->moving, c->moving + half, c->grads + c->n_train,
                                    c->grads + c->n_train + half, (int)half, c->cfg.bn_decay, s));
  if (c->n_flip) HIPCALL(c, launch_weight_flip_batched(c->dt, c->flip_jobs, c->n_flip, c->flip_total, s));
  if (split) {   // the stem's weight gradient is done: its update, then the regulariser sum
    if (int r = join_stem(c, s, true)) return r;
    HIPCALL(c, launch_sgdm(st_a, s));
    HIPCALL(c, launch_sum_partials(c->reg_part, nparts, c->reg_out, s));
  }
  return refresh_stem_pad(c, s);
}

int seg_flush_grads(seg_ctx* c, void* stream) {
  NEED_BOUND(c);
  // a deferred stem weight gradient may still run on the weight-gradient stream: the caller's
  // stream waits for it (without consuming the join seg_apply_update takes)
  return join_stem(c, (hipStream_t)stream, false);
}

int seg_set_defer_stem(seg_ctx* c, int on) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  c->defer_stem = on != 0;
  return 0;
}

int seg_set_premask(seg_ctx* c, int on) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  c->premask = on != 0;
  return 0;
}

int seg_set_lbf(seg_ctx* c, int on) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  c->lbf_on = on != 0;
  return 0;
}

int seg_set_bootstrap(seg_ctx* c, int percentage) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (percentage > 100)
    return set_err(&c->err, -EINVAL, "bootstrapping_percentage %d: must be at most 100 (<= 0 disables "
                   "bootstrapping)", percentage);
  if (percentage <= 0 || c->cfg.nb_pp <= 0) {   // off; without strong images there is no l1 loss
    c->bs_pct = 0;
    return 0;
  }
  const int64_t M = (int64_t)c->cfg.nb_pp * c->cfg.height * c->cfg.width;
  if (M > 2147483647ll) return set_err(&c->err, -EINVAL, "bootstrapping: %lld map entries", (long long)M);
  if (!c->bs_map) {   // first enable (outside any step); freed with the context's allocations
    if (int r = dalloc(c, &c->bs_map, (size_t)M)) return r;
    if (int r = dalloc(c, &c->bs_slab, BOOTSTRAP_SLAB_BYTES / sizeof(unsigned))) return r;
    if (int r = dalloc(c, &c->bs_state, 1)) return r;
  }
  c->bs_pct = percentage;
  c->bs_k = std::max<int64_t>(1, (int64_t)percentage * M / 100);
  return 0;
}

int seg_counter(seg_ctx* c, const char* name, int64_t* value) {
  if (!c || !name || !value) return set_err(c ? &c->err : nullptr, -EINVAL, "null argument");
  const std::string n(name);
  if (n == "premask_launches") *value = c->premask_launches;
  else if (n == "lbf_layers") *value = c->lbf_launches;
  else if (n == "loss_yf_launches") *value = c->loss_yf_launches;
  else if (n == "bootstrap_launches") *value = c->bootstrap_launches;
  else return set_err(&c->err, -ENOENT, "unknown counter '%s'", name);
  return 0;
}

int seg_outputs(seg_ctx* c, const float** losses, const float** reg, const float** logits,
                int* ld, int* hl, int* wl) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (losses) *losses = c->loss_out;
  if (reg) *reg = c->reg_out;
  if (logits) *logits = c->head_in;
  if (ld) *ld = c->ldl;
  if (hl) *hl = c->logits.H;
  if (wl) *wl = c->logits.W;
  return 0;
}

int seg_confusion(seg_ctx* c, const int32_t* labels, const int32_t* decisions, int64_t n,
                  int num_classes, int32_t* cm, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(cm, 0, (size_t)num_classes * num_classes * 4, s);
  if (e == hipSuccess) e = launch_confusion(labels, decisions, n, num_classes, cm, s);
  if (e != hipSuccess) return hip_fail(c, e, "seg_confusion");
  return 0;
}

// What seg_boundary_distance and seg_band_confusion ask of the context, the labels, the size and
// the classes.
static int check_boundary_args(seg_ctx* c, const char* who, const int32_t* labels, int n, int H,
                               int W, int num_classes, int ignore) {
  if (!c) return set_err(nullptr, -EINVAL, "%s: null ctx", who);
  std::string* err = &c->err;
  if (!labels) return set_err(err, -EINVAL, "%s: null labels", who);
  if (n < 1 || n > BOUNDARY_MAX_IMAGES || H < 1 || W < 1)
    return set_err(err, -EINVAL, "%s: bad size n = %d, H = %d, W = %d", who, n, H, W);
  if (num_classes < 1 || num_classes > 256)
    return set_err(err, -EINVAL, "%s: num_classes = %d (1..256)", who, num_classes);
  if (ignore < -1 || ignore >= num_classes)
    return set_err(err, -EINVAL, "%s: ignore = %d (-1 for none, or a class id below num_classes = %d)",
                   who, ignore, num_classes);
  return 0;
}

// the row distances, one byte per pixel, rounded up to 16 bytes
static int64_t boundary_rows_bytes(int n, int H, int W) {
  return ((int64_t)n * H * W + 15) / 16 * 16;
}

int seg_boundary_distance(seg_ctx* c, const int32_t* labels, int n, int H, int W, int num_classes,
                          int ignore, int max_width, uint16_t* d2_out, void* stream) {
  const char* who = "seg_boundary_distance";
  if (int r = check_boundary_args(c, who, labels, n, H, W, num_classes, ignore)) return r;
  if (max_width < 1 || max_width > BOUNDARY_MAX_WIDTH)
    return set_err(&c->err, -EINVAL, "%s: max_width = %d (1..%d)", who, max_width, BOUNDARY_MAX_WIDTH);
  if (!d2_out) return set_err(&c->err, -EINVAL, "%s: null d2_out", who);
  const size_t need = (size_t)boundary_rows_bytes(n, H, W);
  if (c->bd_rows_bytes < need) {   // hipFree waits for the launches that still read the old buffer
    if (c->bd_rows) HIPCALL(c, hipFree(c->bd_rows));
    c->bd_rows = nullptr; c->bd_rows_bytes = 0;
    HIPCALL(c, hipMalloc((void**)&c->bd_rows, need));
    c->bd_rows_bytes = need;
  }
  hipStream_t s = (hipStream_t)stream;
  const BoundaryRowArgs ra{labels, n, H, W, num_classes, ignore, max_width, c->bd_rows};
  HIPCALL(c, launch_boundary_rows(ra, s));
  BoundaryColArgs ca{};
  ca.g = c->bd_rows; ca.N = n; ca.H = H; ca.W = W; ca.wmax = max_width; ca.d2 = d2_out;
  HIPCALL(c, launch_boundary_distance(ca, s));
  return 0;
}

int seg_band_confusion_workspace(int n, int H, int W, int n_widths, int num_classes, int64_t* bytes) {
  if (!bytes || n < 1 || H < 1 || W < 1 || n_widths < 1 || n_widths > BOUNDARY_MAX_WIDTHS ||
      num_classes < 1 || num_classes > 256)
    return set_err(nullptr, -EINVAL, "seg_band_confusion_workspace: bad arguments (n %d, H %d, W %d, "
                   "n_widths %d, num_classes %d%s)", n, H, W, n_widths, num_classes,
                   bytes ? "" : ", null bytes");
  *bytes = boundary_rows_bytes(n, H, W);
  return 0;
}

int seg_band_confusion(seg_ctx* c, const int32_t* labels, const int32_t* decisions, int n, int H,
                       int W, int num_classes, int ignore, const int32_t* widths, int n_widths,
                       void* workspace, int64_t workspace_bytes, int32_t* cm_out, void* stream) {
  const char* who = "seg_band_confusion";
  if (int r = check_boundary_args(c, who, labels, n, H, W, num_classes, ignore)) return r;
  std::string* err = &c->err;
  if (!decisions) return set_err(err, -EINVAL, "%s: null decisions", who);
  if (!widths) return set_err(err, -EINVAL, "%s: null widths", who);
  if (!workspace) return set_err(err, -EINVAL, "%s: null workspace", who);
  if (!cm_out) return set_err(err, -EINVAL, "%s: null cm_out", who);
  if (n_widths < 1 || n_widths > BOUNDARY_MAX_WIDTHS)
    return set_err(err, -EINVAL, "%s: n_widths = %d (1..%d)", who, n_widths, BOUNDARY_MAX_WIDTHS);
  BoundaryColArgs ca{};
  for (int k = 0; k < BOUNDARY_MAX_WIDTHS; ++k) ca.w2[k] = INT_MAX;
  for (int k = 0; k < n_widths; ++k) {
    if (widths[k] < 1 || widths[k] > BOUNDARY_MAX_WIDTH)
      return set_err(err, -EINVAL, "%s: widths[%d] = %d (1..%d)", who, k, widths[k], BOUNDARY_MAX_WIDTH);
    if (k && widths[k] <= widths[k - 1])
      return set_err(err, -EINVAL, "%s: widths must be strictly increasing (widths[%d] = %d after %d)",
                     who, k, widths[k], widths[k - 1]);
    ca.w2[k] = widths[k] * widths[k];
  }
  const int64_t need = boundary_rows_bytes(n, H, W);
  if (workspace_bytes < need)
    return set_err(err, -EINVAL, "%s: workspace of %lld bytes, %lld needed (seg_band_confusion_workspace)",
                   who, (long long)workspace_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const int wmax = widths[n_widths - 1];
  const BoundaryRowArgs ra{labels, n, H, W, num_classes, ignore, wmax, static_cast<uint8_t*>(workspace)};
  ca.g = ra.g; ca.N = n; ca.H = H; ca.W = W; ca.wmax = wmax;
  ca.labels = labels; ca.decisions = decisions; ca.nc = num_classes; ca.K = n_widths; ca.cm = cm_out;
  HIPCALL(c, hipMemsetAsync(cm_out, 0, (size_t)n_widths * num_classes * num_classes * sizeof(int32_t), s));
  HIPCALL(c, launch_boundary_rows(ra, s));
  HIPCALL(c, launch_band_confusion(ca, s));
  HIPCALL(c, launch_band_finalize(cm_out, n_widths, num_classes, s));
  return 0;
}

int seg_set_nesterov(seg_ctx* c, int on) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  c->nesterov = on ? 1 : 0;
  return 0;
}

int seg_set_loss_scale(seg_ctx* c, float scale) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (!(scale > 0.f)) return set_err(&c->err, -EINVAL, "loss scale must be > 0");
  c->loss_scale = scale;
  if (!c->skip_flag && (scale != 1.f || c->dt == SEG_F16))
    if (int r = dalloc(c, &c->skip_flag, 1)) return r;
  return 0;
}

int seg_set_bn_sync(seg_ctx* c, seg_allreduce_fn fn, void* user, int world) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (c->gn && fn && world > 1)   // module_arg_scope :329-331
    return set_err(&c->err, -EINVAL, "cross_replica_norm is supported only for batch normalization");
  if (world < 1) return set_err(&c->err, -EINVAL, "world must be >= 1");
  if (!fn) {   // world == 1 with a hook still exchanges (a one-replica collective)
    c->sync_fn = nullptr;
    c->sync_user = nullptr;
    c->sync_world = 1;
    return 0;
  }
  if (!c->sync_pack) {
    int cmax = 1;
    for (const ConvL& L : c->convs) cmax = std::max(cmax, L.co);
    if (int r = dalloc(c, &c->sync_pack, 2 * (size_t)cmax)) return r;
  }
  c->sync_fn = fn;
  c->sync_user = user;
  c->sync_world = world;
  return 0;
}

int seg_found_inf(seg_ctx* c, const int32_t** flag) {
  if (!c || !flag) return set_err(c ? &c->err : nullptr, -EINVAL, "null argument");
  *flag = c->skip_flag;
  return 0;
}

int seg_grad_buckets(seg_ctx* c, int max_buckets, int64_t* lo, int64_t* hi) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  const int n = (int)c->bk_lo.size();
  for (int i = 0; i < n && i < max_buckets; ++i) {
    if (lo) lo[i] = c->bk_lo[i];
    if (hi) hi[i] = c->bk_hi[i];
  }
  return n;
}

int seg_stream_wait_bucket(seg_ctx* c, int bucket, void* stream) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (bucket < 0 || bucket >= (int)c->bk_ev.size()) return set_err(&c->err, -EINVAL, "bad bucket %d", bucket);
  HIPCALL(c, hipStreamWaitEvent((hipStream_t)stream, c->bk_ev[bucket], 0));
  return 0;
}

int seg_debug_tensor(seg_ctx* c, const char* name, void** ptr, int* dims, int* ld, int* dtype) {
  if (!c || !name) return set_err(c ? &c->err : nullptr, -EINVAL, "null argument");
  if (c->stem_pending)   // the caller reads on its own stream: a deferred stem gradient first
    HIPCALL(c, hipEventSynchronize(c->ev_join));
  std::string n(name);
  Act a;
  int dt = c->dt == SEG_BF16 ? SEG_DTYPE_BF16 : (c->dt == SEG_F16 ? SEG_DTYPE_F16 : SEG_DTYPE_F32);
  if (n == "logits") { a = c->logits; dt = SEG_DTYPE_F32; }
  else if (n == "head_in") { a = c->logits; a.p = (void*)c->head_in; dt = SEG_DTYPE_F32; }
  else if (n == "grad_un") { a = c->logits; a.p = c->grad_un; dt = SEG_DTYPE_F32; }
  else if (n == "dzscale") { a.p = c->dzscale; a.N = a.H = a.W = 1; a.C = a.ld = c->ldl; dt = SEG_DTYPE_F32; }
  else if (n == "l1_loss_map" || n == "bootstrap_tau") {
    if (!c->bs_map) return set_err(&c->err, -EINVAL, "%s: bootstrapping was never enabled (seg_set_bootstrap)", name);
    dt = SEG_DTYPE_F32;
    a.C = a.ld = 1;
    if (n == "l1_loss_map") { a.p = c->bs_map; a.N = c->cfg.nb_pp; a.H = c->cfg.height; a.W = c->cfg.width; }
    else { a.p = &c->bs_state->tau; a.N = a.H = a.W = 1; }
  }
  else if (n == "feat") a = c->feat;
  else if (n == "dfeat") a = c->dfeat;
  else if (n == "z0") {   // stem BN + ReLU output (the max-pool input)
    if (c->z0_stale) {   // fused forward: materialise it (same kernel, this step's statistics)
      HIPCALL(c, hipDeviceSynchronize());   // the step's streams may be non-blocking
      Step S{c, nullptr, c->dt};
      if (int r = bn_apply(S, c->stem, c->z0, 0)) return r;
      HIPCALL(c, hipStreamSynchronize(nullptr));
      c->z0_stale = false;
    }
    a = c->z0;
  }
  else if (n.rfind("pyr", 0) == 0 && n.size() == 6 && n.substr(4) == "_z") {
    // a pyramid branch's BN + ReLU output at its pooled resolution (PSP: grids 1, 2, 3, 6;
    // ASPP: 0 = the image pool), the input of its align-corners resize into the concat
    const int b = n[3] - '0';
    if (b < 0 || b >= (int)c->zb.size() || !c->zb[b].p) return set_err(&c->err, -EINVAL, "bad pyramid branch");
    a = c->zb[b];
  }
  else if (n.rfind("head", 0) == 0 && n.size() > 5) {
    int h = n[4] - '0';
    if (h < 0 || h > 2) return set_err(&c->err, -EINVAL, "bad head");
    if (n.substr(5) == "_out") a = c->heads[h].out;
    else if (n.substr(5) == "_dout") a = c->heads[h].dout;
    else return set_err(&c->err, -EINVAL, "unknown tensor %s", name);
  } else if (n.rfind("conv", 0) == 0) {
    size_t us = n.find('_');
    int i = atoi(n.substr(4, us - 4).c_str());
    if (i < 0 || i >= (int)c->convs.size() || us == std::string::npos) return set_err(&c->err, -EINVAL, "bad conv");
    if (n.substr(us) == "_x" && i == c->stem && c->stem_s2d) {
      // the stem reads the space-to-depth image: present the [N][H][W][8] view of it
      const ConvL& st = c->convs[c->stem];
      if (!c->img_dbg) {
        char* p;
        if (int r = dalloc(c, &p, (size_t)st.N * st.H * st.W * 8 * 2)) return r;
        c->img_dbg = p;
      }
      HIPCALL(c, hipDeviceSynchronize());   // the s2d image is written on the step's stream
      HIPCALL(c, launch_unshuffle_s2d(c->img.p, c->img_dbg, st.N, st.H, st.W, c->img.H, c->img.W,
                                      st.pad_h, st.pad_w, 0));
      HIPCALL(c, hipDeviceSynchronize());
      a.p = c->img_dbg; a.N = st.N; a.H = st.H; a.W = st.W; a.C = 3; a.ld = 8;
    } else if (n.substr(us) == "_x") {
      a = c->convs[i].x;
      if (!a.p) {   // before the first forward (which binds the input): the layer's geometry alone
        const ConvL& L = c->convs[i];
        a.N = L.N; a.H = L.H; a.W = L.W; a.C = L.ci;
      }
    }
    else if (n.substr(us) == "_y") a = c->convs[i].y;
    else if (n.substr(us) == "_dy") {
      ConvL& L = c->convs[i];
      if (L.lbf_done && !L.lbf_dy_ready) {   // folded (lbf.h): the step never wrote it; the apply it replaced, now
        HIPCALL(c, hipDeviceSynchronize());
        const BnBwdArgs b = bn_bwd_args(L, L.st, L.y, L.dy, L.lbf_dyhat);   // the gated gradient: no gate
        HIPCALL(c, launch_bn_bwd_apply(c->dt, 0, b, nullptr));
        HIPCALL(c, hipDeviceSynchronize());
        L.lbf_dy_ready = true;
      }
      a = L.dy;
    }
    else if (n.substr(us) == "_dyhat" && c->convs[i].lbf_done) a = c->convs[i].lbf_dyhat;
    else if (n.substr(us) == "_lbfcoef" && c->convs[i].lbf_done) {   // [3][co] = A, B, D (lbf.h)
      a.p = c->convs[i].lbf_coef; a.N = 1; a.H = 1; a.W = 3; a.C = a.ld = c->convs[i].co;
      dt = SEG_DTYPE_F32;
    }
    else return set_err(&c->err, -EINVAL, "unknown tensor %s", name);
  } else {
    return set_err(&c->err, -EINVAL, "unknown tensor %s", name);
  }
  if (ptr) *ptr = a.p;
  if (dims) { dims[0] = a.N; dims[1] = a.H; dims[2] = a.W; dims[3] = a.C; }
  if (ld) *ld = a.ld;
  if (dtype) *dtype = dt;
  return 0;
}

int seg_profile(seg_ctx* c, int enable) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  if (enable && c->prof.ev.empty()) {
    c->prof.ev.resize(16384);
    for (auto& ev : c->prof.ev) HIPCALL(c, hipEventCreate(&ev));
  }
  c->prof.on = enable != 0;
  c->prof.recs.clear();
  c->prof.next = 0;
  return 0;
}

int seg_profile_read(seg_ctx* c, int cls, double* ms_total, double* gflop_total,
                     int64_t* launches, double* ms_max_layer, char* layer_name, int name_len) {
  if (!c) return set_err(nullptr, -EINVAL, "null ctx");
  double tot = 0, gf = 0;
  int64_t n = 0;
  std::vector<double> per_layer(c->convs.size(), 0.0);
  for (auto& r : c->prof.recs) {
    if (r.cls != cls) continue;
    HIPCALL(c, hipEventSynchronize(c->prof.ev[r.e1]));
    float ms = 0;
    HIPCALL(c, hipEventElapsedTime(&ms, c->prof.ev[r.e0], c->prof.ev[r.e1]));
    tot += ms; gf += r.gflop; ++n;
    per_layer[r.layer] += ms;
  }
  int best = -1;
  for (size_t i = 0; i < per_layer.size(); ++i)
    if (best < 0 || per_layer[i] > per_layer[best]) best = (int)i;
  if (ms_total) *ms_total = tot;
  if (gflop_total) *gflop_total = gf;
  if (launches) *launches = n;
  if (ms_max_layer) *ms_max_layer = best >= 0 ? per_layer[best] : 0;
  if (layer_name && name_len > 0) {
    snprintf(layer_name, name_len, "%s", best >= 0 ? c->convs[best].name.c_str() : "");
  }
  return 0;
}

int seg_profile_dump(seg_ctx* c, char* buf, int len) {
  if (!c || !buf || len <= 0) return set_err(c ? &c->err : nullptr, -EINVAL, "bad argument");
  std::string out;
  char line[512];
  for (auto& r : c->prof.recs) {
    HIPCALL(c, hipEventSynchronize(c->prof.ev[r.e1]));
    float ms = 0;
    HIPCALL(c, hipEventElapsedTime(&ms, c->prof.ev[r.e0], c->prof.ev[r.e1]));
    const ConvL& L = c->convs[r.layer];
    snprintf(line, sizeof(line), "%d %s %d %d %d %d %d %d %.6f %.6f %.6f\n", r.cls, L.name.c_str(),
             L.ci, L.co, L.k, L.rate, L.Ho, L.Wo, r.gflop, (double)ms, r.gbytes);
    out += line;
  }
  snprintf(buf, len, "%s", out.c_str());
  return (int)out.size() >= len ? -ENOSPC : 0;
}

}  // extern "C"
