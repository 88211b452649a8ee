// The order of a training step: the unit, pyramid and head sequencing of the forward and of
// the two-stream backward, over the per-layer launches of net_layers.cpp.
#include "net.h"

namespace segnet {
namespace {

int unit_forward(Step& S, Unit& u) {
  if (u.sc >= 0)
    if (int r = conv_forward(S, u.sc, u.in)) return r;
  if (int r = conv_forward(S, u.c1, u.in)) return r;
  if (int r = bn_apply(S, u.c1, u.z1, 0)) return r;
  if (int r = conv_forward(S, u.c2, u.z1)) return r;
  if (int r = bn_apply(S, u.c2, u.z2, 0)) return r;
  if (int r = conv_forward(S, u.c3, u.z2)) return r;
  // out = relu(shortcut + bn3(conv3))
  if (u.kind == SC_CONV) return bn_apply(S, u.c3, u.out, 0, nullptr, 1, u.sc, 1);
  return bn_apply(S, u.c3, u.out, 0, &u.in, u.kind == SC_SUBSAMPLE ? u.stride : 1, -1, 1);
}

// pred = the unit whose output is u's input (nullptr: none). When both are identity units,
// u's conv1 data gradient (+ the residual dpre) is stored already masked by pred's output ReLU
// bits: everything that reads pred's dout wants it masked (pred's c3 BN backward and, as
// pred's dpre, pred's own conv1 residual), so pred's c3 BN backward neither reads the bits nor
// writes dpre (one M x C store pass fewer per such unit)
bool premask_ok(seg_ctx* c, const Unit& u, const Unit* pred, bool accumulate) {
  if (!c->premask || !pred || accumulate || u.kind != SC_IDENTITY || pred->kind == SC_SUBSAMPLE || c->gn)
    return false;
  if (!pred->out.mask || pred->out.C != c->convs[u.c1].ci || c->convs[pred->c3].co != pred->out.C) return false;
  ConvArgs a = dgrad_args(c, u.c1, pred->dout, &u.dpre, nullptr);
  return dgrad_takes_mask(c->dt, a, pred->out.mask);
}

// the ReLU bits of pred's output when the data gradient into it (of C channels) may be stored
// masked by them: pred an identity or subsample unit, so its c3 BN backward then reads dout
// ungated and writes no dpre (block boundaries: a projection unit's dual data gradient,
// decrease_fdims')
const uint8_t* premask_bits(seg_ctx* c, const Unit* pred, int C) {
  if (!c->premask || !pred || pred->kind == SC_CONV || c->gn || !pred->out.mask ||
      pred->out.C != C || c->convs[pred->c3].co != C)
    return nullptr;
  return pred->out.mask;
}

int unit_backward(Step& S, Unit& u, const Act& dx, bool accumulate, Unit* pred = nullptr) {
  seg_ctx* c = S.c;
  // identity / subsample shortcuts: the c3 BN backward also writes the ReLU-masked dout
  // (dpre), the residual of the unit's input gradient -- unless dout arrived masked
  // (dout_masked, premask_ok). (Measured and rejected: reading dout + the bits as the
  // residual in conv1's dgrad epilogue instead of dpre, 1.8 % slower per step.)
  const bool in_masked = u.dout_masked;
  u.dout_masked = false;
  const Act* dpre = u.kind != SC_CONV && !in_masked ? &u.dpre : nullptr;
  const Act& dres = in_masked ? u.dout : u.dpre;   // the masked dout, wherever it lives
  const ConvL& L3 = c->convs[u.c3];
  const bool lbf = lbf_ok(c, u, in_masked);
  if (lbf) {
    // linear BN-backward fold: reduce + finalize of conv3's BN (the gated gradient into dpre
    // by the reduce itself when dout is not pre-masked; a projection unit's dual reduce, then
    // the shortcut BN's apply alone), then no conv3 apply pass (lbf_backward)
    if (u.kind == SC_CONV) {
      if (int r = bn_backward_dual(S, u.c3, u.sc, u.dout, u.out, true)) return r;
    } else if (int r = bn_backward(S, u.c3, u.dout, 0, in_masked ? nullptr : &u.out, dpre, nullptr, nullptr,
                                   true)) {
      return r;
    }
    if (int r = lbf_backward(S, u, u.kind == SC_CONV ? u.dout : dres)) return r;
  } else {
    if (bn_dual_ok(c, u) && u.out.mask && u.out.C == L3.co) {
      if (int r = bn_backward_dual(S, u.c3, u.sc, u.dout, u.out)) return r;
    } else {
      if (int r = bn_backward(S, u.c3, u.dout, 0, in_masked ? nullptr : &u.out, dpre)) return r;
      if (u.kind == SC_CONV)
        if (int r = bn_backward(S, u.sc, u.dout, 0, &u.out, nullptr)) return r;
    }
    if (int r = conv_wgrad(S, u.c3, u.z2)) return r;
    if (int r = conv_dgrad(S, u.c3, u.dz2)) return r;
  }
  if (int r = bn_backward(S, u.c2, u.dz2, 0, &u.z2, nullptr, nullptr, lbf ? c->lbf_bias : nullptr, false,
                         lbf ? L3.lbf_cs : nullptr))
    return r;
  if (lbf)
    if (int r = lbf_combine(S, u)) return r;
  if (int r = conv_wgrad(S, u.c2, u.z1)) return r;
  if (int r = conv_dgrad(S, u.c2, u.dz1)) return r;
  if (int r = bn_backward(S, u.c1, u.dz1, 0, &u.z1, nullptr)) return r;
  if (int r = conv_wgrad(S, u.c1, u.in)) return r;
  switch (u.kind) {
    case SC_IDENTITY:
      if (accumulate) return conv_dgrad(S, u.c1, dx, &dx, &dres);
      if (premask_ok(c, u, pred, accumulate)) {
        if (int r = conv_dgrad(S, u.c1, dx, &dres, nullptr, pred->out.mask)) return r;
        mark_premasked(c, pred);
        return 0;
      }
      return conv_dgrad(S, u.c1, dx, &dres);
    case SC_SUBSAMPLE: {
      if (accumulate) return set_err(&c->err, -EINVAL, "accumulating subsample unit");
      if (int r = conv_dgrad(S, u.c1, dx)) return r;
      HIPCALL(c, launch_add_strided(S.dt, dx.p, dx.H, dx.W, dx.ld, dres.p, dres.N, dres.H,
                                    dres.W, dres.C, dres.ld, u.stride, S.s));
      return 0;
    }
    case SC_CONV: {
      if (int r = conv_wgrad(S, u.sc, u.in)) return r;
      if (!accumulate) {   // one K-concatenated GEMM when both are 1 x 1 stride-1 ping-pong shapes
        const uint8_t* pm = premask_bits(c, pred, c->convs[u.c1].ci);
        const int r = conv_dgrad_dual(S, u.c1, u.sc, dx, &pm);
        if (r == 0 && pm) mark_premasked(c, pred);
        if (r <= 0) return r;
      }
      if (int r = conv_dgrad(S, u.c1, dx, accumulate ? &dx : nullptr)) return r;
      return conv_dgrad(S, u.sc, dx, &dx);
    }
  }
  return 0;
}

DeconvArgs deconv_args(seg_ctx* c) {
  DeconvArgs a{};
  a.x = (const float*)c->logits.p; a.y = c->up_in; a.g = c->grad_un; a.gscale = c->dzscale;
  a.dx = c->dc_dx; a.part = c->dc_part;
  a.N = c->logits.N; a.H = c->logits.H; a.W = c->logits.W; a.ld = c->ldl;
  for (int h = 0; h < 3; ++h) {
    a.c[h] = c->nc[h];
    a.w[h] = c->params + c->dc_w_off[h]; a.b[h] = c->params + c->dc_b_off[h];
    a.gw[h] = c->grads + c->dc_w_off[h]; a.gb[h] = c->grads + c->dc_b_off[h];
  }
  return a;
}

Act logits_slice(seg_ctx* c, int h) {
  int off = 0;
  for (int i = 0; i < h; ++i) off += c->nc[i];
  Act a = c->logits;
  a.p = (float*)c->logits.p + off;
  a.C = c->nc[h];
  return a;
}

// ---- pyramid modules: PSP pools over four grids (branches 0..3 into concat slices 1..4, the
// extension output itself is slice 0); ASPP has one pooled branch, the image pool (slice 0) ----
// every pooled branch's input from z in two launches: row sums per grid cell, then the columns
int pyramid_pool_forward(Step& S, const Act& z) {
  seg_ctx* c = S.c;
  HIPCALL(c, launch_grid_rowreduce(S.dt, z.p, z.N, z.H, z.W, z.C, z.ld, c->pool_grids,
                                   c->grid_part, S.s));
  void* outs[SEG_MAX_GRIDS] = {nullptr, nullptr, nullptr, nullptr};
  for (size_t b = 0; b < c->pooled.size(); ++b) outs[b] = c->pooled[b].p;
  HIPCALL(c, launch_grid_colreduce(S.dt, c->grid_part, z.N, z.H, z.W, z.C, c->pool_grids, outs, S.s));
  return 0;
}

// pooled branch b: 1x1 conv / BN / ReLU at the pooled resolution, align-corners resize into dst
int pool_branch_forward(Step& S, int b, const Act& dst) {
  seg_ctx* c = S.c;
  const Act& zb = c->zb[b];
  if (int r = conv_forward(S, c->pyr_conv[b], c->pooled[b])) return r;
  if (int r = bn_apply(S, c->pyr_conv[b], zb, 0)) return r;
  HIPCALL(c, launch_resize_fwd(S.dt, zb.p, zb.N, zb.H, zb.W, dst.C, zb.ld, dst.p, dst.H, dst.W, dst.ld, S.s));
  return 0;
}

// its backward from d, the branch's slice of the concat gradient: the transpose of the resize
// (row then column reduce), BN, weight gradient, data gradient into dpooled[b]
int pool_branch_backward(Step& S, int b, const Act& d) {
  seg_ctx* c = S.c;
  HIPCALL(c, launch_grid_rowreduce(S.dt, d.p, d.N, d.H, d.W, d.C, d.ld, c->up_grids[b],
                                   c->grid_part, S.s));
  void* outs[SEG_MAX_GRIDS] = {c->dzb[b].p, nullptr, nullptr, nullptr};
  HIPCALL(c, launch_grid_colreduce(S.dt, c->grid_part, d.N, d.H, d.W, d.C, c->up_grids[b], outs, S.s));
  if (int r = bn_backward(S, c->pyr_conv[b], c->dzb[b], 0, &c->zb[b], nullptr)) return r;
  if (int r = conv_wgrad(S, c->pyr_conv[b], c->pooled[b])) return r;
  return conv_dgrad(S, c->pyr_conv[b], c->dpooled[b]);
}

// the final conv over the concat: feat = relu(bn(conv(concat)))
int pyramid_tail_forward(Step& S) {
  seg_ctx* c = S.c;
  if (int r = conv_forward(S, c->pyr_final, c->concat)) return r;
  return bn_apply(S, c->pyr_final, c->feat, 0);
}
int pyramid_tail_backward(Step& S) {
  seg_ctx* c = S.c;
  if (int r = bn_backward(S, c->pyr_final, c->dfeat, 0, &c->feat, nullptr)) return r;
  if (int r = conv_wgrad(S, c->pyr_final, c->concat)) return r;
  return conv_dgrad(S, c->pyr_final, c->dconcat);
}

int pyramid_forward(Step& S) {
  seg_ctx* c = S.c;
  const Act& z = c->z_dfd;
  const int fd = c->cfg.feature_dims;
  if (int r = pyramid_pool_forward(S, z)) return r;
  if (c->cfg.pyramid == SEG_PYRAMID_PSP) {
    for (int b = 0; b < 4; ++b)
      if (int r = pool_branch_forward(S, b, slice(c, c->concat, (b + 1) * fd, fd))) return r;
  } else {
    // image-pool branch: global mean -> 1x1 conv/BN/ReLU -> align-corners broadcast (slice 0)
    if (int r = pool_branch_forward(S, 0, slice(c, c->concat, 0, fd))) return r;
    // 1x1 and the rate-6/12/18 3x3 branches write their BN/ReLU outputs into slices 1..4
    for (int b = 1; b < 5; ++b) {
      if (int r = conv_forward(S, c->pyr_conv[b], z)) return r;
      if (int r = bn_apply(S, c->pyr_conv[b], slice(c, c->concat, b * fd, fd), 0)) return r;
    }
  }
  return pyramid_tail_forward(S);
}

int pyramid_backward(Step& S) {
  seg_ctx* c = S.c;
  const int fd = c->cfg.feature_dims;
  if (int r = pyramid_tail_backward(S)) return r;
  const void* dps[SEG_MAX_GRIDS] = {nullptr, nullptr, nullptr, nullptr};
  for (size_t b = 0; b < c->dpooled.size(); ++b) dps[b] = c->dpooled[b].p;
  if (c->cfg.pyramid == SEG_PYRAMID_PSP) {
    for (int b = 0; b < 4; ++b)
      if (int r = pool_branch_backward(S, b, slice(c, c->dconcat, (b + 1) * fd, fd))) return r;
    Act d0 = slice(c, c->dconcat, 0, fd);
    HIPCALL(c, launch_psp_input_bwd(S.dt, d0.p, d0.ld, c->pool_grids, dps, d0.N, d0.H, d0.W, fd,
                                    c->dz_dfd.p, c->dz_dfd.ld, S.s));
    return 0;
  }
  // image-pool branch: transpose of the broadcast = sum over the map
  if (int r = pool_branch_backward(S, 0, slice(c, c->dconcat, 0, fd))) return r;
  // conv branches: dz_dfd = sum of their data gradients (fixed branch order)
  for (int b = 1; b < 5; ++b) {
    Act db = slice(c, c->dconcat, b * fd, fd);
    Act zb = slice(c, c->concat, b * fd, fd);
    if (int r = bn_backward(S, c->pyr_conv[b], db, 0, &zb, nullptr)) return r;
    if (int r = conv_wgrad(S, c->pyr_conv[b], c->z_dfd)) return r;
    if (int r = conv_dgrad(S, c->pyr_conv[b], c->dz_dfd, b > 1 ? &c->dz_dfd : nullptr)) return r;
  }
  // + the global-average-pool transpose, in place
  HIPCALL(c, launch_psp_input_bwd(S.dt, c->dz_dfd.p, c->dz_dfd.ld, c->pool_grids, dps, c->dz_dfd.N,
                                  c->dz_dfd.H, c->dz_dfd.W, fd, c->dz_dfd.p, c->dz_dfd.ld, S.s));
  return 0;
}

int backward_layers(Step& S) {
  seg_ctx* c = S.c;
  // no pre-masked gradient survives a backward that stopped part-way (unit_backward)
  for (auto& u : c->units) u.dout_masked = false;
  for (auto& u : c->heads) u.dout_masked = false;
  for (auto& L : c->convs) L.lbf_done = L.lbf_dy_ready = false;
  // hybrid: the loss-normalised gradient goes back through the deconvolution first (its
  // weight / bias gradients and dx), then into the logits BN without a further scale
  if (c->hybrid) HIPCALL(c, launch_deconv_bwd(deconv_args(c), S.s));
  for (int h = 0; h < 3; ++h) {
    Act gz = logits_slice(c, h);
    int off = (int)((float*)gz.p - (float*)c->logits.p);
    gz.p = (c->hybrid ? c->dc_dx : c->grad_un) + off;
    if (int r = bn_backward(S, c->logit_conv[h], gz, 1, nullptr, nullptr,
                            c->hybrid ? nullptr : c->dzscale + off)) return r;
    if (int r = conv_wgrad(S, c->logit_conv[h], c->heads[h].out)) return r;
    if (int r = conv_dgrad(S, c->logit_conv[h], c->heads[h].dout)) return r;
    if (int r = unit_backward(S, c->heads[h], c->dfeat, h > 0)) return r;
  }
  if (c->cfg.pyramid == SEG_PYRAMID_PSP || c->cfg.pyramid == SEG_PYRAMID_ASPP)
    if (int r = pyramid_backward(S)) return r;
  if (c->fov >= 0) {
    if (int r = bn_backward(S, c->fov, c->dz_dfd, 0, &c->z_dfd, nullptr)) return r;
    if (int r = conv_wgrad(S, c->fov, c->z_pre)) return r;
    if (int r = conv_dgrad(S, c->fov, c->dz_pre)) return r;
    if (int r = bn_backward(S, c->dfd, c->dz_pre, 0, &c->z_pre, nullptr)) return r;
  } else if (int r = bn_backward(S, c->dfd, c->dz_dfd, 0, &c->z_dfd, nullptr)) {
    return r;
  }
  if (int r = conv_wgrad(S, c->dfd, c->units.back().out)) return r;
  {
    Unit& last = c->units.back();
    const uint8_t* pm = premask_bits(c, &last, c->convs[c->dfd].ci);
    if (pm) {
      ConvArgs a = dgrad_args(c, c->dfd, last.dout, nullptr, nullptr);
      if (!dgrad_takes_mask(S.dt, a, pm)) pm = nullptr;
    }
    if (int r = conv_dgrad(S, c->dfd, last.dout, nullptr, nullptr, pm)) return r;
    if (pm) mark_premasked(c, &last);
  }
  for (int i = (int)c->units.size() - 1; i >= 0; --i) {
    const Act& dx = i == 0 ? c->dp0 : c->units[i - 1].dout;
    if (int r = unit_backward(S, c->units[i], dx, false, i == 0 ? nullptr : &c->units[i - 1])) return r;
  }
  HIPCALL(c, launch_maxpool_bwd(S.dt, c->pool_arg, c->z0.N, c->z0.H, c->z0.W, 64, c->dp0.p,
                                c->dp0.H, c->dp0.W, c->dp0.ld, c->dz0.p, c->dz0.ld, c->pool_ph,
                                c->pool_pw, S.s));
  if (int r = bn_backward(S, c->stem, c->dz0, 0, &c->z0, nullptr)) return r;
  return conv_wgrad(S, c->stem, c->img);
}

}  // namespace

int forward(Step& S, const float* images) {
  seg_ctx* c = S.c;
  if (c->bn_infer)
    HIPCALL(c, launch_bn_infer_finalize_all(c->infer_jobs, (int)c->convs.size(), S.s));
  if (c->stem_s2d) {
    const ConvL& st = c->convs[c->stem];
    HIPCALL(c, launch_cast_s2d(S.dt, images, c->img.p, st.N, st.H, st.W, c->img.H, c->img.W, st.pad_h,
                               st.pad_w, S.s));
  } else {
    HIPCALL(c, hipMemcpyAsync(c->img.p, images, (size_t)c->img.M() * 3 * sizeof(float),
                              hipMemcpyDeviceToDevice, S.s));
  }
  if (int r = conv_forward(S, c->stem, c->img)) return r;
  const ConvL& stl = c->convs[c->stem];
  if (!c->gn && c->z0.mask && c->pool_ph == 0 && c->pool_pw == 0 && c->z0.H == 2 * c->p0.H &&
      c->z0.W == 2 * c->p0.W) {
    // stem BN + ReLU fused into the max-pool: y0 is read once, z0 (the max-pool input) is never
    // written; its ReLU bits (the BN backward's gate) are
    const double esz = c->esz;
    const double gb = (c->z0.M() * 64.0 * (esz + 0.125) + c->p0.M() * 64.0 * (esz + 1.0)) * 1e-9;
    if (int r = PROFILED(c, S.s, 3, c->stem, gb, -1.0,
                         launch_bn_relu_maxpool_fwd(S.dt, stl.y.p, c->z0.N, c->z0.H, c->z0.W, stl.y.ld,
                                          stl.st.mean, stl.st.scale, c->params + stl.b_off,
                                          c->z0.mask, c->p0.p, c->p0.H, c->p0.W, c->p0.ld,
                                          c->pool_ph, c->pool_pw, c->pool_arg, S.s))) return r;
    c->z0_stale = true;
  } else {
    if (int r = bn_apply(S, c->stem, c->z0, 0)) return r;
    HIPCALL(c, launch_maxpool_fwd(S.dt, c->z0.p, c->z0.N, c->z0.H, c->z0.W, 64, c->z0.ld, c->p0.p,
                                  c->p0.H, c->p0.W, c->p0.ld, c->pool_ph, c->pool_pw, c->pool_arg,
                                  S.s));
    c->z0_stale = false;
  }
  for (auto& u : c->units)
    if (int r = unit_forward(S, u)) return r;
  if (int r = conv_forward(S, c->dfd, c->units.back().out)) return r;
  if (c->fov >= 0) {
    if (int r = bn_apply(S, c->dfd, c->z_pre, 0)) return r;
    if (int r = conv_forward(S, c->fov, c->z_pre)) return r;
    if (int r = bn_apply(S, c->fov, c->z_dfd, 0)) return r;
  } else if (int r = bn_apply(S, c->dfd, c->z_dfd, 0)) {
    return r;
  }
  if (c->cfg.pyramid == SEG_PYRAMID_PSP || c->cfg.pyramid == SEG_PYRAMID_ASPP)
    if (int r = pyramid_forward(S)) return r;
  for (int h = 0; h < 3; ++h) {
    if (int r = unit_forward(S, c->heads[h])) return r;
    if (int r = conv_forward(S, c->logit_conv[h], c->heads[h].out)) return r;
    if (int r = bn_apply(S, c->logit_conv[h], logits_slice(c, h), 1)) return r;
  }
  if (c->hybrid) HIPCALL(c, launch_deconv_fwd(deconv_args(c), S.s));
  return 0;
}

int backward(Step& S) {
  seg_ctx* c = S.c;
  std::fill(c->wg_done.begin(), c->wg_done.end(), 0);
  c->bk_next = 0;
  // a profiled backward runs on one stream so the HIP-event kernel timings are kernel-alone
  c->side_active = c->side_on && !c->prof.on;
  c->prestem_rec = false;
  if (c->side_active) {   // the side stream must not run ahead of the previous use of its buffers
    HIPCALL(c, hipEventRecord(c->ev_join, S.s));
    HIPCALL(c, hipStreamWaitEvent(c->side, c->ev_join, 0));
  }
  if (int r = backward_layers(S)) return r;
  if (int r = bucket_progress(c, c->side_active ? c->side : S.s, true)) return r;
  if (c->side_active) {   // join: the update (and the next forward) follow every weight gradient
    HIPCALL(c, hipEventRecord(c->ev_join, c->side));
    if (c->prestem_rec) {   // deferred: only the gradients before the stem's (see seg_apply_update)
      HIPCALL(c, hipStreamWaitEvent(S.s, c->ev_prestem, 0));
      c->stem_pending = true;
    } else {
      HIPCALL(c, hipStreamWaitEvent(S.s, c->ev_join, 0));
    }
  }
  // BN-parameter + statistics tail bucket: written on the compute stream
  HIPCALL(c, hipEventRecord(c->bk_ev.back(), S.s));
  return 0;
}

int refresh_stem_pad(seg_ctx* c, hipStream_t s) {
  if (!c->stem_s2d) return 0;
  const ConvL& st = c->convs[c->stem];
  HIPCALL(c, launch_stem_s2d_weights((const bf16_t*)st.w_lp, c->stem_wpad, st.co, s));
  return 0;
}

// a deferred stem weight gradient (seg_set_defer_stem) must be complete before anything else
// on stream s reads or rewrites the step's buffers. The pending state is kept until the
// gradient is consumed (seg_apply_update) or superseded (seg_backward): a join on another
// stream must not let a later seg_apply_update skip its own join
int join_stem(seg_ctx* c, hipStream_t s, bool consume) {
  if (!c->stem_pending) return 0;
  HIPCALL(c, hipStreamWaitEvent(s, c->ev_join, 0));
  if (consume) c->stem_pending = false;
  return 0;
}

int refresh_compute_weights(seg_ctx* c, hipStream_t s) {
  if (seg_half(c->dt))
    HIPCALL(c, launch_cast_f32_half(c->dt, c->params, c->w_lp_flat, c->n_decay, s));
  if (c->n_flip) HIPCALL(c, launch_weight_flip_batched(c->dt, c->flip_jobs, c->n_flip, c->flip_total, s));
  return refresh_stem_pad(c, s);
}

}  // namespace segnet
