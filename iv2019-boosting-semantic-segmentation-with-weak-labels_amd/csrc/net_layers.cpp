// Per-layer launches of the training step and the argument builders they share with the
// seg_op_conv_* entries: one conv / BN / group-norm / fold launch sequence per function, on the
// stream the Step names; the weight gradients hand off to the side stream here.
#include "net.h"

namespace segnet {

// ------------------------------------------------------------------------------------------
// conv argument builders: shared by the network's launches and the seg_op_conv_* entries
// ------------------------------------------------------------------------------------------
// a forward conv of x [N][H][W][ldx] with w [Co][k][k][C] into y [N][Ho][Wo][ldy]
ConvArgs fwd_conv_args(const void* x, int N, int H, int W, int C, int ldx, const void* w, int Co,
                       int k, int stride, int rate, int pad_h, int pad_w, int Ho, int Wo, void* y,
                       int ldy, float* stats) {
  ConvArgs a{};
  a.x = x; a.N = N; a.H = H; a.W = W; a.C = C; a.ldx = ldx;
  a.w = w; a.ldw = k * k * C;
  a.y = y; a.Ho = Ho; a.Wo = Wo; a.Co = Co; a.ldy = ldy;
  a.KH = a.KW = k; a.sf = stride; a.st = 1; a.pad_h = pad_h; a.pad_w = pad_w;
  a.dil = rate; a.stats = stats;
  return a;
}
// the 16-bit stem: 4 x 4 VALID over the space-to-depth image (conv.h), weights wpad [Co][256]
static void fwd_s2d_args(ConvArgs& a, const void* wpad) {
  a.C = 16; a.ldx = 16; a.tap8 = 2; a.w = wpad; a.ldw = 256;
  a.KH = a.KW = 4; a.sf = 1; a.pad_h = a.pad_w = 0; a.dil = 1;
}
// the weight gradient of that conv from dy [P][lddy]; s2d: the stem's 4 x 4 VALID form (x is
// the space-to-depth image, C = 16)
WgradArgs wgrad_conv_args(const void* dy, int lddy, const void* x, int N, int H, int W, int C, int ldx,
                          int Ho, int Wo, int Co, int k, int stride, int rate, int pad_h, int pad_w,
                          bool s2d) {
  WgradArgs a{};
  a.dy = dy; a.lddy = lddy;
  a.x = x; a.N = N; a.H = H; a.W = W; a.C = C; a.ldx = ldx;
  a.Ho = Ho; a.Wo = Wo; a.Co = Co;
  a.KH = a.KW = k; a.sf = stride; a.pad_h = pad_h; a.pad_w = pad_w; a.dil = rate;
  if (s2d) { a.KH = a.KW = 4; a.sf = 1; a.pad_h = a.pad_w = 0; a.dil = 1; }
  return a;
}

// concurrent = the weight gradient runs on the side stream beside the dgrad -> BN chain:
// at most ~128 workgroups (half the CUs, the chain keeps the other half: 90.4 -> 92.9 img/s
// on C2 against 512, and half the split-K slab traffic); alone (profiled, single stream,
// seg_op_*): at most one wave of the 256 CUs (one workgroup per CU, LDS-bound). The weight-
// gradient kernels run one workgroup per CU, so a launch of 256 + a few workgroups pays a
// whole second wave for the few: tools/wgrad_sweep.py PP_ONLY=1 on the C2 shapes, e.g. block3
// 3x3 (9 tiles) 24 splits 188 us, 32 splits (288 workgroups) 266 us; block3 1x1 (4 tiles) 64
// splits 97 us against the former 2-wave 128 splits 121 us.
int wgrad_splits(const WgradArgs& a, int dt, bool concurrent) {
  const long P = (long)a.N * a.Ho * a.Wo;
  const long tiles = conv_wgrad_plan(dt, a).split_tiles;   // of the kernel launch_conv_wgrad runs
  // workgroups = tiles x splits <= one wave of the CUs the launch may use; each split >= 32
  // K-steps of 64 pixels beside the dgrad chain, >= 16 alone
  const long target = concurrent ? 128 : 256;
  long s = std::max<long>(1, target / std::max<long>(tiles, 1));
  long maxs = std::max<long>(1, P / (concurrent ? 2048 : 1024));
  s = std::min(s, maxs);
  return (int)std::min<long>(s, 256);
}

// the weight-gradient problem of layer L (x / dy pixel strides: the activations' layout,
// channels padded to a multiple of 8); the space-to-depth stem is a 4 x 4 VALID conv over 16
// channels
WgradArgs wgrad_problem(const ConvL& L, bool s2d) {
  const int C = s2d ? 16 : L.ci;
  return wgrad_conv_args(nullptr, (L.co_pad + 7) / 8 * 8, nullptr, L.N, L.H, L.W, C, (C + 7) / 8 * 8,
                         L.Ho, L.Wo, L.co_pad, L.k, L.stride, L.rate, L.pad_h, L.pad_w, s2d);
}

// a data gradient as a forward problem over dy [N][Ho][Wo][Co] with the flipped, transposed
// weights wt [Ci][k][k][Co], into dx [N][H][W][Ci]; (pad_h, pad_w) = the forward conv's padding.
// Shared by the network's launches (dgrad_args) and the op entry seg_op_conv_dgrad_fused
ConvArgs dgrad_conv_args(const void* dy, int N, int Ho, int Wo, int Co, int lddy, const void* wt,
                         int Ci, int k, int stride, int rate, int pad_h, int pad_w, int H, int W,
                         void* dx, int lddx) {
  ConvArgs a{};
  a.x = dy; a.N = N; a.H = Ho; a.W = Wo; a.C = Co; a.ldx = lddy;
  a.w = wt; a.ldw = k * k * Co;
  a.y = dx; a.Ho = H; a.Wo = W; a.Co = Ci; a.ldy = lddx;
  a.KH = a.KW = k;
  const int keff = k + (k - 1) * (rate - 1);
  a.sf = 1; a.st = stride;
  a.pad_h = (keff - 1) - pad_h; a.pad_w = (keff - 1) - pad_w;
  a.dil = rate; a.stats = nullptr;
  return a;
}
// the K-concatenated second data gradient (1 x 1, the same pixels): dx += dy2 . wt2
void dgrad_dual_args(ConvArgs& a, const void* dy2, int lddy2, int Co2, const void* wt2) {
  a.x2 = dy2; a.ldx2 = lddy2; a.C2 = Co2;
  a.w2 = wt2; a.ldw2 = Co2;
}

// dx = dgrad(dy) [+ r1] [+ r2]
ConvArgs dgrad_args(seg_ctx* c, int li, const Act& dx, const Act* r1, const Act* r2) {
  ConvL& L = c->convs[li];
  ConvArgs a = dgrad_conv_args(L.dy.p, L.N, L.Ho, L.Wo, L.co, L.dy.ld, L.wt_lp, L.ci, L.k, L.stride,
                               L.rate, L.pad_h, L.pad_w, L.H, L.W, dx.p, dx.ld);
  if (r1) { a.r = r1->p; a.ldr = r1->ld; }
  if (r2) { a.r2 = r2->p; a.ldr2 = r2->ld; }
  return a;
}

// "can this data gradient store its output masked by `bits`?": asks the plan of the launch
// with the mask set; the mask stays in `a` only when the answer is yes
bool dgrad_takes_mask(int dt, ConvArgs& a, const uint8_t* bits) {
  a.omask = bits; a.ldm = a.Co / 8;
  if (conv_nt_plan(dt, 0, a).omask) return true;
  a.omask = nullptr;
  return false;
}

// pred's output gradient was stored pre-masked: call only once that store is enqueued
void mark_premasked(seg_ctx* c, Unit* pred) {
  pred->dout_masked = true;
  ++c->premask_launches;
}

// the BN backward of layer L over dz: y, the statistics in `st` (L.st, or one image's
// st_img[n] under group norm), the output dy and the reduce partials
BnBwdArgs bn_bwd_args(const ConvL& L, const BnState& st, const Act& y, const Act& dy, const Act& dz) {
  BnBwdArgs a{};
  a.dz = dz.p; a.lddz = dz.ld;
  a.y = y.p; a.ldy = y.ld; a.M = y.M(); a.C = L.co;
  a.mean = st.mean; a.invstd = st.invstd; a.scale = st.scale;
  a.sdy = st.sdy; a.sdyx = st.sdyx;
  a.dy = dy.p; a.lddy = dy.ld;
  a.part = L.bwd_part; a.rb = L.rb;
  return a;
}

// the gate of dz: z (null: none), or its ReLU bits instead when z keeps them for exactly the
// layer's channels and the caller's kernel can read them (bits_ok: its conditions on dz)
static void bn_bwd_gate(BnBwdArgs& a, const ConvL& L, const Act* z, bool bits_ok) {
  if (!z) return;
  a.z = z->p; a.ldz = z->ld;
  if (z->mask && bits_ok && z->C == L.co) { a.mask = z->mask; a.z = nullptr; }
}

// may a projection unit's conv3 and shortcut BN backward run as the dual kernels (one read of
// dz and the bits for both)? Batch norm, no cross-replica exchange, the same shape and row blocks
bool bn_dual_ok(const seg_ctx* c, const Unit& u) {
  if (u.kind != SC_CONV || c->gn || c->sync_fn) return false;
  const ConvL& L3 = c->convs[u.c3];
  const ConvL& Ls = c->convs[u.sc];
  return Ls.co == L3.co && Ls.rb == L3.rb && Ls.y.M() == L3.y.M();
}

// ------------------------------------------------------------------------------------------
// kernel sequencing helpers
// ------------------------------------------------------------------------------------------
// two launches under one record
#define PROFILED2(c, s, cls, layer, gflop, gbytes, first, second)                       \
  [&] {                                                                                 \
    const char* what = #first;                                                          \
    return profiled((c), (s), (cls), (layer), (gflop), (gbytes), what, [&] {            \
      const hipError_t e1 = (first);                                                    \
      if (e1 != hipSuccess) return e1;                                                  \
      what = #second;                                                                   \
      return (second);                                                                  \
    });                                                                                 \
  }()

// one cross-replica exchange (SUM in place, ordered on stream s) through the caller's hook
static int sync_exchange(seg_ctx* c, float* buf, long n, hipStream_t s) {
  const int r = c->sync_fn(c->sync_user, buf, (int64_t)n, s);
  if (r) return set_err(&c->err, -EIO, "cross-replica BN exchange failed (hook returned %d)", r);
  return 0;
}

// record (on the weight-gradient stream ws) the events of every conv-weight bucket whose
// gradients are all written, in order; `final` flushes the remaining weight buckets
int bucket_progress(seg_ctx* c, hipStream_t ws, bool final) {
  const int nw = (int)c->bk_convs.size();
  while (c->bk_next < nw) {
    const int b = c->bk_next;
    bool ok = true;
    for (int li : c->bk_convs[b]) ok = ok && c->wg_done[li];
    if (!ok && !final) return 0;
    HIPCALL(c, hipEventRecord(c->bk_ev[b], ws));
    ++c->bk_next;
  }
  return 0;
}

// the compute-to-side hand-off of layer li's weight gradient: W = the step it runs on. With
// the side stream active, what the compute stream has queued so far (the layer's dy, the
// weight gradient's input) is ready before the side stream goes on
static int wgrad_stream(Step& S, int li, Step& W) {
  seg_ctx* c = S.c;
  W = S;
  if (!c->side_active) return 0;
  HIPCALL(c, hipEventRecord(c->ev_dy[li], S.s));
  HIPCALL(c, hipStreamWaitEvent(c->side, c->ev_dy[li], 0));
  W.s = c->side;
  return 0;
}
// layer li's weight gradient is queued on `stream`
static int wgrad_done(seg_ctx* c, int li, hipStream_t stream) {
  c->wg_done[li] = 1;
  return bucket_progress(c, stream, false);
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
int conv_forward(Step& S, int li, const Act& x) {
  seg_ctx* c = S.c;
  ConvL& L = c->convs[li];
  L.x = x;
  ConvArgs a = fwd_conv_args(x.p, x.N, x.H, x.W, x.C, x.ld, L.w_lp, L.co, L.k, L.stride, L.rate,
                             L.pad_h, L.pad_w, L.Ho, L.Wo, L.y.p, L.y.ld, L.stats_part);
  a.ldw = L.k * L.k * L.ci;   // the weights' row length is the layer's, whatever view x is
  if (li == c->stem && c->stem_s2d) fwd_s2d_args(a, c->stem_wpad);
  long M = (long)x.N * L.Ho * L.Wo;
  const double esz = c->esz;   // x + w + y, each once
  const double gbx = ((double)L.N * L.H * L.W * L.ci + (double)L.co * L.k * L.k * L.ci +
                      (double)M * L.co) * esz * 1e-9;
  if (int r = PROFILED(c, S.s, 0, li, 2.0 * M * L.co * L.k * L.k * L.ci * 1e-9, gbx,
                       launch_conv_nt(S.dt, 0, a, S.s))) return r;
  if (c->gn) {   // group norm: per-image statistics in every mode (no moving statistics)
    GnPartArgs g{};
    g.y = L.y.p; g.ldy = L.y.ld; g.N = x.N; g.hw = (long)L.Ho * L.Wo; g.C = L.co; g.part = L.gn_part;
    HIPCALL(c, launch_gn_partial(S.dt, 0, g, S.s));
    HIPCALL(c, launch_gn_stats_final(L.gn_part, x.N, g.hw, L.co, L.groups, c->params + L.g_off,
                                     L.st_dev, S.s));
    return 0;
  }
  if (c->bn_infer) return 0;   // is_training=False: the statistics were set for every layer
                               // by one launch at the start of the forward
  const bool sync = c->sync_fn != nullptr;
  HIPCALL(c, launch_bn_stats_finalize(L.stats_part, M, L.co, conv_nt_plan(S.dt, 0, a).stat_rows,
                                      c->params + L.g_off, L.st, S.s, sync ? c->sync_pack : nullptr));
  if (sync) {
    if (int r = sync_exchange(c, c->sync_pack, 2L * L.co, S.s)) return r;
    HIPCALL(c, launch_bn_sync_unpack(c->sync_pack, L.co, 1.f / c->sync_world, c->params + L.g_off,
                                     L.st, S.s));
  }
  return 0;
}

static int bn_apply_one(Step& S, int li, const Act& out0, int out_f32, const Act* res0, int rs, int li2,
                        int relu, int img) {
  seg_ctx* c = S.c;
  ConvL& L = c->convs[li];
  const Act out = image_rows(out0, img, out_f32 ? 4 : c->esz);
  Act res_img;
  const Act* res = res0;
  if (res0 && img >= 0) { res_img = image_rows(*res0, img, c->esz); res = &res_img; }
  const Act Y = image_rows(L.y, img, c->esz);
  const BnState& st = img >= 0 ? L.st_img[img] : L.st;
  BnApplyArgs a{};
  a.y = Y.p; a.ldy = Y.ld; a.M = Y.M(); a.C = L.co;
  a.mean = st.mean; a.scale = st.scale; a.beta = c->params + L.b_off;
  a.relu = relu < 0 ? (L.relu ? 1 : 0) : relu;
  if (res) {
    a.res = res->p; a.ldres = res->ld; a.rs = rs; a.Ho = L.Ho; a.Wo = L.Wo; a.Hr = res->H;
    a.Wr = res->W;
  }
  if (li2 >= 0) {
    ConvL& L2 = c->convs[li2];
    const Act Y2 = image_rows(L2.y, img, c->esz);
    const BnState& st2 = img >= 0 ? L2.st_img[img] : L2.st;
    a.y2 = Y2.p; a.ldy2 = Y2.ld; a.mean2 = st2.mean; a.scale2 = st2.scale;
    a.beta2 = c->params + L2.b_off;
  }
  a.out = out.p; a.ldo = out.ld;
  a.mask = a.relu ? out.mask : nullptr;
  const double esz = seg_half(S.dt) ? 2.0 : 4.0;
  const double gb = a.M * (double)a.C * (esz * (1 + (a.res || a.y2 ? 1 : 0)) +
                                         (out_f32 ? 4.0 : esz)) * 1e-9;
  return PROFILED(c, S.s, 3, li, gb, -1.0, launch_bn_apply(S.dt, out_f32, a, S.s));
}

int bn_apply(Step& S, int li, const Act& out, int out_f32, const Act* res, int rs, int li2, int relu) {
  if (!S.c->gn) return bn_apply_one(S, li, out, out_f32, res, rs, li2, relu, -1);
  // group norm: the per-image affine is per channel; one launch per image on row offsets
  for (int n = 0; n < out.N; ++n)
    if (int r = bn_apply_one(S, li, out, out_f32, res, rs, li2, relu, n)) return r;
  return 0;
}

// ------------------------------------------------------------------------------------------
// BN / group-norm backward
// ------------------------------------------------------------------------------------------
// group norm backward (gn.h): per image the batch-norm reduce (S1, S2 per channel) into
// its slice of the partials, one finalize for the layer (dgamma / dbeta, per-image group
// means), per image the batch-norm apply with scale = invstd and the gradient times gamma
static int gn_backward(Step& S, int li, const Act& dz0, int dz_f32, const Act* z0, const Act* dyhat0,
                       const float* dzscale) {
  seg_ctx* c = S.c;
  ConvL& L = c->convs[li];
  const size_t zsz = dz_f32 ? 4 : c->esz;
  Act dzl = dz0;
  if (dzscale) {   // the logits: the loss normalisation first (gamma mixes into it below)
    HIPCALL(c, launch_gn_chscale((const float*)dz0.p, c->gn_gscaled, dz0.M(), dz0.ld, L.co, dzscale, S.s));
    dzl.p = c->gn_gscaled;
  }
  const float* gamma = c->params + L.g_off;
  const bool tb = c->cfg.train_bn != 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1)
      HIPCALL(c, launch_gn_bwd_final(L.bwd_part, dz0.N, L.rb, (long)L.Ho * L.Wo, L.co, L.groups, gamma,
                                     L.st_dev, tb ? c->grads + L.g_off : nullptr,
                                     tb ? c->grads + L.b_off : nullptr, S.s));
    for (int n = 0; n < dz0.N; ++n) {
      const BnState& st = L.st_img[n];
      BnBwdArgs a = bn_bwd_args(L, st, image_rows(L.y, n, c->esz), image_rows(L.dy, n, c->esz),
                                image_rows(dzl, n, zsz));
      if (z0) {
        const Act z = image_rows(*z0, n, zsz);
        bn_bwd_gate(a, L, &z, !dz_f32);
      }
      a.part = L.bwd_part + (size_t)n * L.rb * L.co * 2;
      if (pass == 0) {
        HIPCALL(c, launch_bn_bwd_reduce(S.dt, dz_f32, a, S.s));
      } else {
        if (dyhat0) {
          const Act dh = image_rows(*dyhat0, n, c->esz);
          a.dyhat = dh.p; a.lddyhat = dh.ld;
        }
        a.scale = st.invstd;   // dx = invstd (gamma dyhat - sdy - xhat sdyx)
        a.dzscale = gamma;
        HIPCALL(c, launch_bn_bwd_apply(S.dt, dz_f32, a, S.s));
      }
    }
  }
  return 0;
}

// BN backward for layer li: dz (gradient wrt BN output), z (mask source or null). dshift: a
// per-channel term of dz its producer left out (added before the gate; bits only);
// reduce_only: reduce + finalize (the linear BN-backward fold replaces the apply), the gated
// gradient stored by the reduce when dyhat_out is given
int bn_backward(Step& S, int li, const Act& dz, int dz_f32, const Act* z, const Act* dyhat_out,
                const float* dzscale, const float* dshift, bool reduce_only, float* cs_out) {
  seg_ctx* c = S.c;
  if (c->gn) return gn_backward(S, li, dz, dz_f32, z, dyhat_out, dzscale);
  ConvL& L = c->convs[li];
  BnBwdArgs a = bn_bwd_args(L, L.st, L.y, L.dy, dz);
  bn_bwd_gate(a, L, z, !dz_f32 && !dzscale);
  if (dyhat_out) { a.dyhat = dyhat_out->p; a.lddyhat = dyhat_out->ld; }
  a.dzscale = dzscale;
  a.dshift = dshift;
  a.reduce_dyhat = reduce_only && dyhat_out ? 1 : 0;
  if (cs_out) { a.cs_part = cs_out; a.beta = c->params + L.b_off; }
  if (bn_bwd_reduce_plan(S.dt, a).refusal)
    return set_err(&c->err, -EINVAL, "bn_backward %s: shift / reduce-side dyhat need the ReLU bits", L.name.c_str());
  const double esz = seg_half(S.dt) ? 2.0 : 4.0, zsz = dz_f32 ? 4.0 : esz;
  const double me = a.M * (double)a.C * 1e-9;
  const double gb_in = me * (zsz + (a.mask ? 0.125 : (z ? zsz : 0.0)) + esz);
  if (int r = PROFILED(c, S.s, 4, li, gb_in + (a.reduce_dyhat ? me * esz : 0.0), -1.0,
                       launch_bn_bwd_reduce(S.dt, dz_f32, a, S.s))) return r;
  const bool tb = c->cfg.train_bn != 0;
  // a backward after a moving-statistics forward (TRAIN without
  // batch_norm_accumulate_statistics) differentiates through constant statistics
  HIPCALL(c, launch_bn_bwd_finalize(L.bwd_part, L.rb, a.M, L.co, L.st,
                                    tb ? c->grads + L.g_off : nullptr,
                                    tb ? c->grads + L.b_off : nullptr, S.s, c->bn_infer));
  if (c->sync_fn && !c->bn_infer) {
    // [mean(dyhat) | mean(dyhat * xhat)] (contiguous in the layer's state) averaged over the
    // replicas: dx is the gradient through the global statistics; dgamma / dbeta stay this
    // replica's sums (the gradient all-reduce averages them)
    if (int r = sync_exchange(c, L.st.sdy, 2L * L.co, S.s)) return r;
    HIPCALL(c, launch_scale2(L.st.sdy, 2L * L.co, 1.f / c->sync_world, 0, 1.f, S.s));
  }
  if (reduce_only) return 0;
  const double gb_apply = gb_in + me * esz * (dyhat_out ? 2 : 1);
  return PROFILED(c, S.s, 5, li, gb_apply, -1.0, launch_bn_bwd_apply(S.dt, dz_f32, a, S.s));
}

// BN backward of two layers gated by the same dz / ReLU bits (a projection unit's conv3 and
// shortcut BN): one dual reduce and one dual apply read dz and the bits once for both; each
// layer keeps its own finalize. Batch norm, 16-bit or fp32 dz of the storage type, no
// cross-replica exchange (that path runs the two layers through bn_backward)
// second_only: dz arrived pre-masked and the first layer's apply is folded (lbf.h): after the
// dual reduce and both finalizes only the second layer's apply runs (ungated)
int bn_backward_dual(Step& S, int li, int li2, const Act& dz, const Act& z, bool second_only) {
  seg_ctx* c = S.c;
  ConvL& L = c->convs[li];
  ConvL& L2 = c->convs[li2];
  BnBwdArgs a = bn_bwd_args(L, L.st, L.y, L.dy, dz);
  a.mask = z.mask;
  const BnBwdArgs a2 = bn_bwd_args(L2, L2.st, L2.y, L2.dy, dz);   // alone: ungated
  a.y2 = a2.y; a.ldy2 = a2.ldy;
  a.mean2 = a2.mean; a.invstd2 = a2.invstd; a.scale2 = a2.scale;
  a.sdy2 = a2.sdy; a.sdyx2 = a2.sdyx;
  a.dy2 = a2.dy; a.lddy2 = a2.lddy;
  a.part2 = a2.part;
  const double esz = seg_half(S.dt) ? 2.0 : 4.0;
  const double me = a.M * (double)a.C * 1e-9;
  const double gb_in = me * (esz + 0.125 + 2 * esz);   // dz + bits + both y
  if (int r = PROFILED(c, S.s, 4, li, gb_in, -1.0, launch_bn_bwd_reduce_dual(S.dt, a, S.s))) return r;
  const bool tb = c->cfg.train_bn != 0;
  HIPCALL(c, launch_bn_bwd_finalize(L.bwd_part, L.rb, a.M, L.co, L.st, tb ? c->grads + L.g_off : nullptr,
                                    tb ? c->grads + L.b_off : nullptr, S.s, c->bn_infer));
  HIPCALL(c, launch_bn_bwd_finalize(L2.bwd_part, L2.rb, a.M, L2.co, L2.st,
                                    tb ? c->grads + L2.g_off : nullptr,
                                    tb ? c->grads + L2.b_off : nullptr, S.s, c->bn_infer));
  if (second_only) return PROFILED(c, S.s, 5, li2, me * 3 * esz, -1.0, launch_bn_bwd_apply(S.dt, 0, a2, S.s));
  return PROFILED(c, S.s, 5, li, gb_in + me * 2 * esz, -1.0, launch_bn_bwd_apply_dual(S.dt, a, S.s));
}

// ------------------------------------------------------------------------------------------
// conv backward
// ------------------------------------------------------------------------------------------
// dx = dgrad(dy) [+ r1] [+ r2]; omask: ReLU bits to store dx masked by (premask)
int conv_dgrad(Step& S, int li, const Act& dx, const Act* r1, const Act* r2, const uint8_t* omask) {
  seg_ctx* c = S.c;
  ConvL& L = c->convs[li];
  ConvArgs a = dgrad_args(c, li, dx, r1, r2);
  if (omask) { a.omask = omask; a.ldm = a.Co / 8; }
  long M = (long)L.N * L.H * L.W;
  // dy + w + dx (+ each residual read once)
  const double nres = (r1 ? 1.0 : 0.0) + (r2 ? 1.0 : 0.0);
  const double gbx = ((double)L.N * L.Ho * L.Wo * L.co + (double)L.co * L.k * L.k * L.ci +
                      (double)M * L.ci * (1.0 + nres)) * c->esz * 1e-9;
  return PROFILED(c, S.s, 1, li, 2.0 * M * L.ci * L.k * L.k * L.co * 1e-9 / L.stride / L.stride, gbx,
                  launch_conv_nt(S.dt, 0, a, S.s));
}

// dx = dgrad(li) + dgrad(li2) in one K-concatenated ping-pong launch: a projection unit's conv1
// and shortcut (both 1 x 1, stride 1, the unit input's geometry). Returns 1 when the shapes do
// not fit that path (the caller then runs the two data gradients with the residual add).
// omask (in / out): ReLU bits to store dx masked by (premask_bits), reset to nullptr when the
// launch cannot take them
int conv_dgrad_dual(Step& S, int li, int li2, const Act& dx, const uint8_t** omask) {
  seg_ctx* c = S.c;
  const ConvL& L = c->convs[li];
  const ConvL& L2 = c->convs[li2];
  if (!seg_half(S.dt) || L.k != 1 || L2.k != 1 || L.stride != 1 || L2.stride != 1 ||
      L.ci != L2.ci || L.Ho != L2.Ho || L.Wo != L2.Wo || L.H != L.Ho || L.W != L.Wo ||
      !L.wt_lp || !L2.wt_lp)
    return 1;
  ConvArgs a = dgrad_args(c, li, dx, nullptr, nullptr);
  dgrad_dual_args(a, L2.dy.p, L2.dy.ld, L2.co, L2.wt_lp);
  // the ping-pong dual only: a narrow unit input keeps the two data gradients
  if (a.st != 1 || a.sf != 1 || a.pad_h || a.pad_w || conv_nt_plan(S.dt, 0, a).kernel != NT_PP) return 1;
  // stored masked by the consumer's ReLU bits where that launch exists
  if (omask && *omask && !dgrad_takes_mask(S.dt, a, *omask)) *omask = nullptr;
  const long M = (long)L.N * L.H * L.W;
  const double gbx = ((double)M * (L.co + L2.co) + (double)(L.co + L2.co) * L.ci + (double)M * L.ci) *
                     c->esz * 1e-9;
  return PROFILED(c, S.s, 1, li, 2.0 * M * L.ci * (L.co + L2.co) * 1e-9, gbx, launch_conv_nt(S.dt, 0, a, S.s));
}

static int conv_wgrad_impl(Step& S, int li, const Act& x) {
  seg_ctx* c = S.c;
  ConvL& L = c->convs[li];
  const bool s2d = li == c->stem && c->stem_s2d;
  WgradArgs a = wgrad_conv_args(L.dy.p, L.dy.ld, x.p, x.N, x.H, x.W, x.C, x.ld, L.Ho, L.Wo, L.co_pad,
                                L.k, L.stride, L.rate, L.pad_h, L.pad_w, s2d);
  // the stem's weight gradient is the last work of the step (its dgrad is skipped): nothing
  // runs beside it, so it takes the whole chip (tools/timeline.py: the compute stream idled
  // ~0.75 ms waiting for it)
  a.splits = wgrad_splits(a, S.dt, c->side_active && li != c->stem);
  // the shared slab was sized at creation for these shapes; never exceed it
  a.splits = clamp_splits(a.splits, (long)c->slab_floats, (long)a.Co * a.KH * a.KW * a.C);
  a.out = c->slab;
  long P = (long)L.N * L.Ho * L.Wo;
  // dy + x (16-bit) + the fp32 weight gradient; split-K slab traffic is overhead, not algorithmic
  const double gbx = (((double)P * L.co + (double)L.N * L.H * L.W * L.ci) * c->esz +
                      (double)L.co * L.k * L.k * L.ci * 4.0) * 1e-9;
  if (int r = PROFILED(c, S.s, 2, li, 2.0 * P * L.co * L.k * L.k * L.ci * 1e-9, gbx,
                       launch_conv_wgrad(S.dt, a, S.s))) return r;
  if (s2d) {
    HIPCALL(c, launch_splitk_reduce_s2d(c->slab, a.splits, (long)L.co_pad * 256, L.co,
                                        c->grads + L.w_off, S.s));
    return 0;
  }
  const long n = (long)L.co * L.k * L.k * L.ci;
  // slab rows are co_pad wide only in the Co dimension: rows 0..co-1 are the real ones
  // split z of the slab starts at z*co_pad*ncol; rows >= co are padding and never reduced
  HIPCALL(c, launch_splitk_reduce(c->slab, a.splits, (long)L.co_pad * L.k * L.k * L.ci, n,
                                  c->grads + L.w_off, 0, S.s));
  return 0;
}

int conv_wgrad(Step& S, int li, const Act& x) {
  seg_ctx* c = S.c;
  if (c->side_active && li == c->stem && c->defer_stem) {   // every other weight gradient is queued before it
    HIPCALL(c, hipEventRecord(c->ev_prestem, c->side));
    c->prestem_rec = true;
  }
  Step W;   // the layer's dy (and the wgrad input x) are ready on the compute stream
  if (int r = wgrad_stream(S, li, W)) return r;
  if (int r = conv_wgrad_impl(W, li, x)) return r;
  return wgrad_done(c, li, W.s);
}

// ------------------------------------------------------------------------------------------
// linear BN-backward fold of an identity unit's conv3 (lbf.h)
// ------------------------------------------------------------------------------------------
// the folded data gradient: one K-concatenated GEMM [dyhat | y2] x [A o W3 ; H] into u.dz2
static ConvArgs lbf_dgrad_args(const seg_ctx* c, const Unit& u, const Act& dyhat) {
  const ConvL& L = c->convs[u.c3];
  ConvArgs a{};
  a.x = dyhat.p; a.N = L.N; a.H = L.Ho; a.W = L.Wo; a.C = L.co; a.ldx = dyhat.ld;
  a.w = c->lbf_wts; a.ldw = L.co;
  a.y = u.dz2.p; a.Ho = L.H; a.Wo = L.W; a.Co = L.ci; a.ldy = u.dz2.ld;
  a.x2 = u.z2.p; a.ldx2 = u.z2.ld; a.C2 = L.ci; a.w2 = c->lbf_h; a.ldw2 = L.ci;
  a.KH = a.KW = 1; a.sf = 1; a.st = 1; a.dil = 1;
  return a;
}

// in_masked: u.dout arrived pre-masked (a projection unit folds only then: its gated gradient
// is dout itself, and its dual BN reduce cannot store one)
bool lbf_ok(seg_ctx* c, const Unit& u, bool in_masked) {
  if (!c->lbf_on || !c->lbf_wts || !lbf_shape_ok(c, u)) return false;
  if (u.kind == SC_CONV && (!in_masked || !bn_dual_ok(c, u))) return false;
  const ConvL& L3 = c->convs[u.c3];
  if (!L3.lbf_coef || !L3.wt_lp || !u.out.mask || u.out.C != L3.co || !u.z2.mask ||
      u.z2.C != L3.ci || u.dz2.C != L3.ci)
    return false;
  if (u.kind != SC_CONV && u.dpre.ld != u.dout.ld) return false;
  return conv_nt_plan(c->dt, 0, lbf_dgrad_args(c, u, u.dout)).kernel != NT_INVALID;
}

// the weight gradient of a folded conv3 (on the weight-gradient stream when it is active):
// P1 = dyhat^T y2 and G = y2^T y2 by the weight-gradient kernel, the column sums of y2, then
// dW3 = A o P1 + B (x) colsum + D o (W3 G) into the gradient buffer
static int lbf_wgrad(Step& S, Unit& u, const Act& dyhat) {
  seg_ctx* c = S.c;
  const int li = u.c3;
  ConvL& L = c->convs[li];
  Step W;   // dyhat, y2 and this layer's coefficients are ready on the compute stream
  if (int r = wgrad_stream(S, li, W)) return r;
  const Act& y2 = u.z2;
  const long P = (long)L.N * L.Ho * L.Wo;
  const long n1 = (long)(L.co + L.ci) * L.ci;
  // algorithmic work of the layer's weight gradient; the G rows are time of this class too
  // (the combine is recorded with the BN-backward apply class, lbf_combine)
  const double gbx = (((double)P * L.co + (double)P * L.ci) * c->esz + (double)L.co * L.ci * 4.0) * 1e-9;
  // P1 = dyhat^T y2 and G = y2^T y2 as one launch: output rows co.. co + ci - 1 take y2 as dy.
  // Narrow ci: the tile the heuristic picks; ci >= 256: the ping-pong 256 x 256 tile at every
  // size (the heuristic halves it on small maps)
  WgradArgs a = wgrad_conv_args(dyhat.p, dyhat.ld, y2.p, y2.N, y2.H, y2.W, y2.C, y2.ld, L.Ho, L.Wo,
                                L.co + L.ci, 1, 1, 1, 0, 0);
  a.dy2 = y2.p; a.lddy2 = y2.ld; a.Co1 = L.co;
  a.splits = clamp_splits(wgrad_splits(a, S.dt, c->side_active), (long)c->slab_floats, n1);
  a.out = c->slab;
  const int tile = L.ci < 256 ? 0 : 256;
  if (tile && conv_wgrad_plan(S.dt, a, tile, tile).kernel != WG_PP)
    return set_err(&c->err, -EINVAL, "lbf weight gradient %s: shape", L.name.c_str());
  return PROFILED2(c, W.s, 2, li, 2.0 * P * L.co * L.ci * 1e-9, gbx,
                   launch_conv_wgrad(S.dt, a, W.s, tile, tile),
                   launch_splitk_reduce(c->slab, a.splits, n1, n1, c->lbf_p1, 0, W.s));
}

// dW3 = A o P1 + B (x) colsum + D o (W3 G) into the gradient buffer, after the unit's conv2
// BN-backward reduce has written the column sums of y2 (recomputed there from z2 exactly as
// the forward BN apply formed y2: a separate pass over y2 measured the same step time,
// profiles/r05_s26_premask_cs_wg_ab.txt), on the weight-gradient stream when it is active
int lbf_combine(Step& S, Unit& u) {
  seg_ctx* c = S.c;
  const int li = u.c3;
  ConvL& L = c->convs[li];
  Step W;
  if (int r = wgrad_stream(S, li, W)) return r;
  // profiled as BN-backward apply time with the prep and H (the B and D terms it adds are that
  // pass's affine part); its bytes: P1, G, W3, the column-sum partials and the result
  const double gbc = ((double)L.co * L.ci * (4.0 + c->esz + 4.0) + (double)L.ci * L.ci * 4.0 +
                      (double)c->convs[u.c2].rb * L.ci * 4.0) * 1e-9;
  LbfCombineArgs cb{};
  cb.co = L.co; cb.ci = L.ci; cb.w = L.w_lp; cb.g = c->lbf_p1 + (size_t)L.co * L.ci; cb.p1 = c->lbf_p1;
  cb.cspart = L.lbf_cs; cb.rb = c->convs[u.c2].rb;
  cb.coef = L.lbf_coef; cb.out = c->grads + L.w_off;
  if (int r = PROFILED(c, W.s, 5, li, gbc, -1.0, launch_lbf_combine(S.dt, cb, W.s))) return r;
  return wgrad_done(c, li, W.s);
}

// after the conv3 BN reduce + finalize: the coefficients, the scaled weights, H, the weight
// gradient (side stream) and the conv3 data gradient as one K-concatenated GEMM
// [dyhat | y2] x [A o W3 ; H] into u.dz2 (its constant b is left to c2's BN backward)
int lbf_backward(Step& S, Unit& u, const Act& dyhat) {
  seg_ctx* c = S.c;
  ConvL& L = c->convs[u.c3];
  const int co = L.co, ci = L.ci;
  // profiled as BN-backward apply time (the pass they replace), in two records so that the
  // weight gradient queued between them (one stream when profiling) is not counted twice:
  // the prep's bytes (both weight copies read and written), then H's (its operands, slab and
  // 16-bit result)
  LbfPrepArgs p{};
  p.co = co; p.ci = ci;
  p.mean = L.st.mean; p.invstd = L.st.invstd; p.scale = L.st.scale; p.sdy = L.st.sdy; p.sdyx = L.st.sdyx;
  p.w = L.w_lp; p.wt = L.wt_lp; p.wts = c->lbf_wts; p.xd = c->lbf_xd; p.bpart = c->lbf_bpart;
  p.coef = L.lbf_coef;
  if (int r = PROFILED(c, S.s, 5, u.c3, 4.0 * co * ci * c->esz * 1e-9, -1.0, launch_lbf_prep(S.dt, p, S.s)))
    return r;
  if (int r = lbf_wgrad(S, u, dyhat)) return r;
  const double gbh = (2.0 * co * ci * c->esz + (double)ci * ci * (c->esz + 8.0 * lbf_hsplits(L))) * 1e-9;
  WgradArgs h{};   // H[k][k'] = sum_c (D_c W3[c][k]) W3[c][k']: the channels c are the "pixels"
  h.dy = c->lbf_xd; h.lddy = ci;
  h.x = L.w_lp; h.N = 1; h.H = 1; h.W = co; h.C = ci; h.ldx = ci;
  h.Ho = 1; h.Wo = co; h.Co = ci; h.KH = h.KW = 1; h.sf = 1; h.dil = 1;
  h.splits = lbf_hsplits(L); h.out = c->lbf_hslab;
  if (int r = PROFILED2(c, S.s, 5, u.c3, gbh, -1.0, launch_conv_wgrad(S.dt, h, S.s),
                        launch_lbf_hreduce(S.dt, c->lbf_hslab, h.splits, (long)ci * ci, c->lbf_h, c->lbf_bpart,
                                           co / 128, ci, c->lbf_bias, S.s)))
    return r;
  const ConvArgs a = lbf_dgrad_args(c, u, dyhat);
  const long M = (long)L.N * L.H * L.W;
  const double gbx = ((double)M * (co + ci) + (double)co * ci + (double)ci * ci + (double)M * ci) * c->esz * 1e-9;
  if (int r = PROFILED(c, S.s, 1, u.c3, 2.0 * M * ci * co * 1e-9, gbx, launch_conv_nt(S.dt, 0, a, S.s))) return r;
  L.lbf_done = true;
  L.lbf_dyhat = dyhat;
  ++c->lbf_launches;
  return 0;
}

}  // namespace segnet
