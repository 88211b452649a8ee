/* seg_hip.h — C ABI of libseg_hip.so, the MI355X (gfx950) training path for the
 * hierarchical weak-label segmentation model of pmeletis/IV2019-boosting-semantic-
 * segmentation-with-weak-labels.
 *
 * The reference exposes this path through Python/TF plugin functions; each entry point
 * below replaces the TF graph that one of them builds (paths relative to the reference's
 * code/ directory):
 *
 *   seg_create / seg_destroy      model(...) graph construction + variable creation
 *                                 (models/resnet50_extended_model_hierarchical.py:17-141,
 *                                  models/resnet50_extended_feature_extractor.py:8-51)
 *   seg_forward                   the TRAIN-mode forward pass of model(...) up to the
 *                                 low-resolution logits (hierarchical.py:102-134)
 *   seg_loss                      upsampler + softmax/argmax/decision fusion
 *                                 (hierarchical.py:135-168) and define_losses(TRAIN)
 *                                 (estimator/define_losses_hierarchical.py:14-217)
 *   seg_backward                  tf.gradients inside create_train_op
 *                                 (estimator/define_estimator_hierarchical.py:120-129)
 *   seg_apply_update              MomentumOptimizer.apply_gradients + UPDATE_OPS (BN moving
 *                                 averages, EMA) (estimator/define_optimizer.py:3-26,
 *                                 define_estimator_hierarchical.py:96-111)
 *   seg_confusion                 define_metrics.mean_iou's confusion matrix
 *                                 (estimator/define_metrics.py:5-20)
 *
 * Conventions: every function returns 0 on success or a negative errno-style code;
 * seg_last_error() describes the failure. Device buffers passed in are caller-owned; the
 * context owns activations and workspace. NHWC layout. Every launch goes to the explicit
 * stream argument; no call allocates, frees or synchronises inside a step, so a step can
 * be captured in a hipGraph. One context per device; not re-entrant per context.
 */
#ifndef SEG_HIP_H
#define SEG_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct seg_ctx seg_ctx;

enum { SEG_PYRAMID_NONE = 0, SEG_PYRAMID_PSP = 1, SEG_PYRAMID_ASPP = 2 };
enum { SEG_DTYPE_F32 = 0, SEG_DTYPE_BF16 = 1, SEG_DTYPE_F16 = 2 };
enum { SEG_DATASET_CITYSCAPES = 0, SEG_DATASET_VISTAS = 1 };
enum { SEG_PARAM_WEIGHTS = 0, SEG_PARAM_GAMMA = 1, SEG_PARAM_BETA = 2,
       SEG_PARAM_MOVING_MEAN = 3, SEG_PARAM_MOVING_VAR = 4, SEG_PARAM_BIASES = 5 };
enum { SEG_UPSAMPLING_BILINEAR = 0, SEG_UPSAMPLING_HYBRID = 1 };
enum { SEG_NORM_BATCH = 0, SEG_NORM_GROUP = 1 };

typedef struct seg_cfg {
  int depth;            /* 50 | 101 (name_feature_extractor) */
  int pyramid;          /* SEG_PYRAMID_* (psp_module; ASPP is the commented spec) */
  int height, width;    /* height/width_feature_extractor */
  int nb_pp, nb_pb, nb_pi;  /* per-GPU per-pixel / per-bbox / per-image sub-batches */
  int dtype;            /* SEG_DTYPE_*: compute/storage dtype (accumulation is fp32) */
  int dataset;          /* SEG_DATASET_* (per_pixel_dataset_name) */
  int output_stride;    /* stride_feature_extractor (8) */
  int feature_dims;     /* feature_dims_decreased (256) */
  float bn_decay;       /* batch_norm_decay (0.9) */
  int train_bn;         /* norm_train_variables */
  float weight_decay;   /* regularization_weight (0.00017): l2_regularizer scale */
  int fov_k, fov_rate;  /* fov_expansion_kernel_size / _rate: the optional extension/increase_fov
                           conv (resnet50_extended_feature_extractor.py:44-49); 0 = off */
  int upsampling;       /* SEG_UPSAMPLING_* (upsampling_method, hierarchical.py:143-184): hybrid
                           adds a 3x3 conv2d_transpose + bias per logits head before the resize */
  int norm;             /* SEG_NORM_* (norm_layer, hierarchical.py:293-333): group = per-image
                           tf.contrib.layers.group_norm after every conv, no moving statistics */
  int groups;           /* group-norm groups of the network's convs (0 = 32); the logits convs
                           use 1 (the softmax_classifier arg scope) */
} seg_cfg;

/* lifecycle -------------------------------------------------------------------------- */
int seg_create(int device, const seg_cfg* cfg, seg_ctx** out);
int seg_destroy(seg_ctx* ctx);
const char* seg_last_error(seg_ctx* ctx);   /* ctx may be NULL (creation errors) */

/* parameters: flat fp32 buffers, allocated by the caller (sizes from seg_sizes) --------
 * params  [n_train]            conv weights ([Co][KH][KW][Ci]) then BN gamma/beta
 * grads   [n_train + n_stats]  gradient of the segmentation loss; the tail holds this
 *                              step's BN batch statistics (mean, Bessel variance) so one
 *                              all-reduce averages both across data-parallel ranks
 * momentum[n_train], ema[n_train] (optional, may be NULL), moving[n_moving] */
int seg_sizes(seg_ctx* ctx, int64_t* n_train, int64_t* n_decay, int64_t* n_moving,
              int64_t* n_stats);
int seg_bind_buffers(seg_ctx* ctx, float* params, float* grads, float* momentum, float* ema,
                     float* moving);
int64_t seg_param_count(seg_ctx* ctx);
int seg_param_info(seg_ctx* ctx, int64_t i, const char** name, int64_t* offset,
                   int64_t* numel, int* kind);
/* dims[4]: weights (Co, KH, KW, Ci); BN vectors and biases (C, 1, 1, 1). The hybrid
 * upsampler's conv2d_transpose weights are (Cin, 3, 3, Cout) so that the OHWI -> HWIO export
 * gives TF's [h][w][out][in] filter layout */
int seg_param_shape(seg_ctx* ctx, int64_t i, int64_t* dims);
/* re-derive compute copies (bf16 weights, flipped dgrad weights) after a host write */
int seg_params_updated(seg_ctx* ctx, void* stream);

/* one training step -------------------------------------------------------------------- */
/* images_nhwc [N][H][W][3] fp32 is read (copied / converted into the context) on `stream`;
 * the caller's buffer may be released once the forward's work on that stream is done */
int seg_forward(seg_ctx* ctx, const float* images_nhwc, void* stream);
int seg_loss(seg_ctx* ctx, const int32_t* px_labels, const float* bbox_soft,
             const float* tag_soft, int32_t* decisions_out, void* stream);
int seg_backward(seg_ctx* ctx, void* stream);
/* lr, momentum; ema_decay_eff = min(ema_decay, (1+step)/(10+step)) or 0 to skip EMA;
 * grad_scale multiplies the gradient (1/world_size after a SUM all-reduce) */
int seg_apply_update(seg_ctx* ctx, float lr, float momentum, float ema_decay_eff,
                     float grad_scale, void* stream);
/* tf.train.MomentumOptimizer(use_nesterov=on) for later updates (define_optimizer.py:17-20):
 * var -= lr * (g + momentum * accum) instead of var -= lr * accum; off by default */
int seg_set_nesterov(seg_ctx* ctx, int on);
/* Overlap the update with the backward's last kernel (single-process training loops: nothing
 * may read the gradients between seg_backward and seg_apply_update). With on, seg_backward
 * returns with the stream joined to every weight gradient except the stem's, which is still
 * running on the weight-gradient stream; seg_apply_update updates every other parameter beside
 * it and joins before the stem's weights. Every other call that takes a stream joins first.
 * No reference counterpart (scheduling only; results are unchanged). Off by default.
 * seg_flush_grads makes `stream` wait for that last weight gradient, for a caller that reads
 * the gradient buffer before seg_apply_update. */
int seg_set_defer_stem(seg_ctx* ctx, int on);
int seg_flush_grads(seg_ctx* ctx, void* stream);
/* pre-masked identity-unit gradients (on by default): when an identity unit follows another,
 * its conv1 data gradient stores the previous unit's output gradient already ReLU-masked, and
 * that unit's c3 BN backward skips the mask bits and the separate masked-gradient store.
 * Scheduling of bytes only: results are bitwise identical either way (tests/test_gpu_step.py).
 * No reference counterpart. */
int seg_set_premask(seg_ctx* ctx, int on);
/* linear BN-backward fold (on by default): the training BN backward of a 16-bit bottleneck's
 * expanding conv3 is affine in the gated output gradient and in the conv input, so its apply
 * pass is folded into the conv3 data gradient (a K-concatenated GEMM) and weight gradient
 * (a second GEMM + an fp32 combine); 0 runs the separate BN-backward apply pass (the fold's
 * reference path in the parity tests). Same math, different rounding order. No reference
 * counterpart. */
int seg_set_lbf(seg_ctx* ctx, int on);
/* runtime counters since seg_create (diagnostics; no reference counterpart):
 * "premask_launches" = data gradients stored pre-masked (seg_set_premask): identity units'
 *   conv1, and at block boundaries a projection unit's conv1 + shortcut and decrease_fdims';
 * "lbf_layers" = conv3 layers whose BN-backward apply was folded into their data / weight
 * gradients by linearity (seg_set_lbf);
 * "loss_yf_launches" = seg_loss calls whose loss head ran the y-first kernel (the full-res
 *   columns of every block fit one 256-thread chunk: the 512 x 1024 and 1024 x 2048 shapes).
 * "bootstrap_launches" = seg_loss calls that ran the bootstrapped l1 loss (seg_set_bootstrap):
 *   loss map + threshold select + gated loss head.
 * -ENOENT for an unknown name. */
int seg_counter(seg_ctx* ctx, const char* name, int64_t* value);

/* Bootstrapped per-pixel l1 loss, the reference's --bootstrapping_percentage ("Percentage of
 * pixels to bootstrap while computing the loss. -1 disables bootstrapping. Set it closer to 100
 * the more unlabeled pixels a dataset has."). The reference accepts the flag but its published
 * tree ships no loss code behind it, so the semantics are fixed here: online hard-pixel
 * bootstrapping of the l1 loss, per context (each replica selects over its own sub-batch).
 *   p = percentage: p <= 0 off (later seg_loss calls launch exactly what they launch without
 *     this call); 1..100 on; p > 100 returns -EINVAL and seg_last_error names the flag. With
 *     nb_pp == 0 the call is accepted and does nothing.
 *   m [nb_pp][H][W] f32, the l1 loss map: the l1 sparse softmax cross-entropy of the upsampled
 *     l1 logits of the strong images where the l1 weight is 1 (l1 label <= l1_wmax), exactly
 *     +0.0f where it is 0. Every entry is a finite float >= +0, so bit patterns order as values.
 *   M = nb_pp * H * W (every pixel, labelled or not), K = max(1, p * M / 100) in 64-bit integers,
 *     tau = the K-th largest of the M entries of m.
 *   A pixel is selected iff its l1 weight is 1 and m >= tau: ties at tau are all selected (the
 *     selected count may exceed K), no ordering by index. The weight is read from the stored m.
 *   l1_segmentation = sum of the per-pixel loss over the selected pixels / their count (0 if
 *     none); n1 of seg_outputs is the selected count; the strong images' l1 channels get a
 *     gradient only at selected pixels, scaled by the new 1 / n1. Both l2 terms, the weak-label
 *     gate, the decisions, seg = l1 + 0.1 (l2v + l2h), regularisation and loss scaling are
 *     unchanged; EVAL and PREDICT never see it.
 *   p = 100, or fewer than K positive entries (tau = 0), selects every weighted pixel: the
 *     outputs are bitwise those of the off path.
 * seg_loss then runs: map pass -> exact radix select of tau (three digit passes of 11 + 11 + 10
 * bits on the float bits, integer histograms, no host synchronisation, no float atomics, bitwise
 * reproducible) -> the gated loss head. The map and the select's workspace are allocated by the
 * first enabling call (outside a step) and freed by seg_destroy. */
int seg_set_bootstrap(seg_ctx* ctx, int percentage);

/* outputs ------------------------------------------------------------------------------
 * losses: device float[10] = {segmentation, l1, l2_vehicle, l2_human, n1, n2v, n2h,
 *         f1, f2v, f2h}; reg: device float[1] regularisation value of the last update
 *         (weights before the update) */
int seg_outputs(seg_ctx* ctx, const float** losses, const float** reg,
                const float** logits_lowres, int* ld_logits, int* h_low, int* w_low);
int seg_confusion(seg_ctx* ctx, const int32_t* labels, const int32_t* decisions, int64_t n,
                  int num_classes, int32_t* cm, void* stream);

/* boundary-band (trimap) confusion: the confusion matrix restricted to the pixels within w pixels
 * of a ground-truth label boundary, for several w (the boundary accuracy of the DenseCRF and
 * DeepLab papers; no reference counterpart: the semantics are fixed here). Integers throughout.
 * Inputs: labels int32 [n][H][W] (the EVAL branch's prolabels, evaluation cids), decisions int32
 *   [n][H][W], num_classes nc in 1..256 as for seg_confusion, ignore = a class id or -1 for none,
 *   widths = w_0 < ... < w_{K-1}, K in 1..8, each w in 1..64. All pointers but widths are device
 *   memory; widths is read on the host during the call.
 * Counted label: l with 0 <= l < nc and l != ignore.
 * Boundary pixel: a pixel that carries a counted label and has at least one 4-neighbour in the
 *   same image that carries another counted label; both pixels of such a pair are boundary pixels.
 *   An ignored or out-of-range pixel is never a boundary pixel and never makes a neighbour one.
 * Squared distance: d2 of a pixel = the minimum of dy^2 + dx^2 over the boundary pixels of the
 *   same image, capped at 64^2 + 1: no wrap-around, nothing crosses between images of the batch.
 * Band of width w: the pixels with d2 <= w^2; bands are nested.
 * Band confusion: cm[k][l][d] = the number of pixels in the band of w_k with labels == l and
 *   decisions == d, both in [0, nc): the acceptance rule of seg_confusion, ignored labels
 *   included (the host drops the void row and column of every matrix as it does there).
 *
 * seg_boundary_distance: d2_out uint16 [n][H][W] = d2 capped at max_width^2 + 1 instead
 *   (max_width in 1..64): exact up to max_width^2, and max_width^2 + 1 wherever d2 is larger. The
 *   one byte per pixel the two passes exchange lives in a buffer of ctx, grown by the call that
 *   needs more (a device allocation, which synchronises) and freed by seg_destroy.
 * seg_band_confusion_workspace: the bytes of workspace seg_band_confusion needs (n * H * W rounded
 *   up to 16). The workspace is the caller's; seg_band_confusion neither allocates nor synchronises.
 * seg_band_confusion: cm_out int32 [n_widths][nc][nc], overwritten (zeroed on the stream first),
 *   not accumulated. Two passes sized by w_{K-1}, not by the limit of 64: per row the horizontal
 *   distance to the nearest boundary pixel, capped at w_{K-1} + 1, one byte per pixel; then per
 *   pixel the minimum over |dy| <= w_{K-1} of dy^2 + that distance squared, one count in the
 *   histogram of the smallest band that holds the pixel, and a sum over k at the end. The counts
 *   are integers, exact in any order.
 * -EINVAL with a seg_last_error text naming the function and the argument, and no launch, for: a
 *   null ctx, labels, decisions, widths, workspace, cm_out, d2_out or bytes; n, H or W < 1 (n above
 *   65535); num_classes outside 1..256; ignore < -1 or >= num_classes; n_widths outside 1..8; a
 *   width or max_width outside 1..64; widths not strictly increasing; a workspace that is too
 *   small. */
int seg_boundary_distance(seg_ctx* ctx, const int32_t* labels, int n, int H, int W,
                          int num_classes, int ignore, int max_width, uint16_t* d2_out,
                          void* stream);
int seg_band_confusion_workspace(int n, int H, int W, int n_widths, int num_classes,
                                 int64_t* bytes);
int seg_band_confusion(seg_ctx* ctx, const int32_t* labels, const int32_t* decisions,
                       int n, int H, int W, int num_classes, int ignore,
                       const int32_t* widths, int n_widths,
                       void* workspace, int64_t workspace_bytes,
                       int32_t* cm_out /* [n_widths][nc][nc] */, void* stream);

/* EVAL / PREDICT (define_estimator_hierarchical.py:161-232) ------------------------------
 * seg_set_bn_inference(ctx, 1): later seg_forward calls normalise with the moving statistics
 * (tf.contrib.layers.batch_norm is_training = batch_norm_accumulate_statistics = False,
 * models/resnet50_extended_model_hierarchical.py:40-49,306-307); 0 restores training BN.
 * Turning it on snapshots the bound buffers (call it again after seg_bind_buffers); the
 * statistics of every layer are then set by one launch at the start of each forward.
 * seg_predict: decisions of the last seg_forward at out_h x out_w: fused hierarchical argmax
 * (hierarchical.py:88-130) -> cid_map[n_map] (training -> evaluation/inference cids, -1 =
 * void -> max+1; _map_predictions_to_new_cids :490-522) -> optional _replace_voids
 * (:577-630) -> NEAREST_NEIGHBOR align_corners resize to out_h x out_w (_resize_predictions
 * :524-575). decisions_out: device int32 [N][out_h][out_w].
 * replace_voids: 0 = none; 1 = the EVAL order above (replace at network resolution, then the
 * nearest resize); 2 = the PREDICT order (:227-231): nearest-resize the decisions and
 * ResizeBilinear(align_corners) the l1 probabilities to out_h x out_w first, then replace
 * voids from the top-2 of the RESIZED probabilities. 1 and 2 agree when out = network size. */
int seg_set_bn_inference(seg_ctx* ctx, int on);
int seg_predict(seg_ctx* ctx, const int32_t* cid_map, int n_map, int replace_voids, int out_h,
                int out_w, int32_t* decisions_out, void* stream);
/* seg_full_predictions: the model's full-resolution `predictions` of the last seg_forward
 * (hierarchical.py:84-130) at network resolution H x W, C = c1 + c2 + c3 channels (l1 | l2
 * vehicle | l2 human): logits_out f32 [N][H][W][C] (align-corners bilinear upsampling of the
 * low-res logits), probs_out f32 [N][H][W][C] (per-head softmax), head_decisions_out int32
 * [N][H][W][3] (per-head argmax), decisions_out int32 [N][H][W] (fused, common cids). Every
 * output is optional (NULL skips it); float outputs 16-byte aligned. */
int seg_full_predictions(seg_ctx* ctx, float* logits_out, float* probs_out,
                         int32_t* head_decisions_out, int32_t* decisions_out, void* stream);

/* test-time augmentation: multi-scale and flip inference (no reference counterpart; the semantics
 * are fixed here). The caller runs one moving-statistics forward per entry -- a scale s of the
 * batch, mirrored in x or not -- in a context of that entry's size, and hands the entries'
 * low-resolution logits (what seg_outputs returns as logits_lowres) to one decision launch.
 * seg_resize_images: the image pyramid. in fp32 [n][H][W][3] -> out fp32 [n][h_out][w_out][3] by
 *   TF 1.12's legacy bilinear resize with align_corners = False, the arithmetic of
 *   seg_prepare_images: scale = (float)in / (float)out, in_f = o * scale, lo = (int)in_f,
 *   hi = min(lo + 1, in - 1), top = tl + (tr - tl) * xl, bot likewise, v = top + (bot - top) * yl,
 *   every operation rounded to fp32 on its own. flip = 1 reads source column W - 1 - x_src: the
 *   mirror, then the resize. With equal sizes the lerp weights are exactly 0, so flip = 0 copies
 *   and flip = 1 mirrors bit for bit (a -0.0f may come out as +0.0f). -EINVAL for a null
 *   pointer with n > 0, n < 0, a size < 1 or flip outside 0..1.
 * seg_tta_decisions: N, H, W (the network size) and the head tables come from ctx; the context's
 *   own logits are not read. entries is a host array of n_entries records: logits device fp32
 *   [N][h_low][w_low][ld] (channels l1 | l2 vehicle | l2 human, ld >= c1 + c2 + c3 the pixel
 *   stride), flip = 1 when the entry saw the mirrored image. For network pixel (n, y, x) and
 *   entry e: u_e = ResizeBilinear(align_corners = True) of the entry's logits to H x W at column
 *   x, or W - 1 - x for a flipped entry; p_e = the per-head softmax of u_e (max-subtracted, fast
 *   exp, one reciprocal), both exactly as seg_predict forms them; sum = p_1 + ... + p_E in entry
 *   order in fp32, starting from p_1; mean = sum * (1.0f / E). Decisions: per-head first-maximum
 *   argmax of the sums -> hierarchical fusion (hierarchical.py:113-117) -> cid_map as in
 *   seg_predict (-1 -> max + 1) -> replace_voids = 1: the stable top-2 of the l1 sums, as mode 1
 *   of seg_predict -> NEAREST_NEIGHBOR align_corners resize to out_h x out_w; only the network
 *   pixels the output pixels select are computed, and no full-resolution tensor is written.
 *   replace_voids = 2 (seg_predict's PREDICT order on resized probabilities) is not defined for
 *   averaged probabilities: -EINVAL. decisions_out: device int32 [N][out_h][out_w].
 *   mean_probs_out: optional (NULL skips it) device fp32 [N][H][W][c1 + c2 + c3], 16-byte
 *   aligned; needs out_h x out_w = H x W.
 *   With one unflipped entry holding the context's own logits, decisions_out is bitwise what
 *   seg_predict writes in modes 0 and 1 and mean_probs_out is bitwise probs_out of
 *   seg_full_predictions.
 *   -EINVAL with a seg_last_error text, and no launch, for: n_entries outside
 *   1..SEG_TTA_MAX_ENTRIES; a null ctx, entries, logits, cid_map or decisions_out; h_low or
 *   w_low < 1; ld < c1 + c2 + c3; flip outside 0..1; replace_voids outside 0..1; a cid map of
 *   the wrong length or with an entry < -1; an output size < 1; mean_probs_out misaligned or
 *   given with an output size other than H x W. */
#define SEG_TTA_MAX_ENTRIES 16
typedef struct seg_tta_entry { const float* logits; int h_low, w_low, ld, flip; } seg_tta_entry;
int seg_resize_images(const float* in, int n, int H, int W, int h_out, int w_out, int flip,
                      float* out, void* stream);
int seg_tta_decisions(seg_ctx* ctx, const seg_tta_entry* entries, int n_entries,
                      const int32_t* cid_map, int n_map, int replace_voids, int out_h, int out_w,
                      float* mean_probs_out, int32_t* decisions_out, void* stream);

/* sliding-window inference (the [tile] ... [stich] of the reference's system sketch,
 * utils/utils.py above --height_system; it builds neither, the semantics are fixed here). The
 * caller prepares the batch at a canvas of canvas_h x canvas_w >= the network size H x W, runs one
 * moving-statistics forward of the SAME context per entry -- the H x W window of the canvas at
 * origin (ys[iy], xs[ix]), mirrored in x or not -- and hands the entries' low-resolution logits
 * to one decision launch. The window grid is the product ys x xs; the entry order is rows of ys
 * outermost, then xs, then, with flip, the unflipped entry followed by the mirrored one:
 * entry (iy * nx + ix) * (1 + flip) + mirrored.
 * seg_window_images: out[b][y][x][c] = in[b][y0 + y][x0 + (flip ? W - 1 - x : x)][c] for fp32
 *   [n][Hc][Wc][3] -> [n][H][W][3]: a copy, bit for bit. -EINVAL with a seg_last_error text
 *   naming the function, and no launch, for a null pointer with n > 0, n < 0, a size < 1, a
 *   window that is not inside the canvas, or flip outside 0..1.
 * seg_window_decisions: N, H, W (the network size = the window size) and the head tables come
 *   from ctx; the context's own logits are not read. logits is a host array of ny * nx *
 *   (1 + flip) device pointers in entry order, each fp32 [N][h_low][w_low][ld] (channels l1 | l2
 *   vehicle | l2 human, ld >= c1 + c2 + c3 the pixel stride). For canvas pixel (n, Y, X) and each
 *   entry whose window contains it, in entry order: (y, x) = (Y - y0, X - x0); u =
 *   ResizeBilinear(align_corners = True) of the entry's logits to H x W at (y, x), or at column
 *   W - 1 - x for a mirrored entry; p = the per-head softmax of u, both exactly as
 *   seg_tta_decisions forms them; sum = the first covering entry's p plus the others' in entry
 *   order in fp32; k = the number of covering entries; mean = sum * r_k with r_k the correctly
 *   rounded fp32 1 / k (1.0f / (float)k divided on the host, the bits seg_tta_decisions uses for
 *   k entries). Decisions on the sums exactly as in seg_tta_decisions: per-head first-maximum
 *   argmax -> hierarchical fusion -> cid_map (-1 -> max + 1) -> replace_voids = 1: the stable
 *   top-2 of the l1 sums -> NEAREST_NEIGHBOR align_corners resize from the CANVAS to out_h x
 *   out_w; only the canvas pixels the output pixels select are computed, and no full-resolution
 *   tensor is written. decisions_out: device int32 [N][out_h][out_w]. mean_probs_out: optional
 *   (NULL skips it) device fp32 [N][canvas_h][canvas_w][c1 + c2 + c3], 16-byte aligned; needs
 *   out_h x out_w = canvas_h x canvas_w.
 *   With canvas = network size (ys = xs = {0}) the outputs are bitwise those of
 *   seg_tta_decisions on the same one or two entries; with windows that do not overlap, every
 *   window's part of the outputs is bitwise seg_tta_decisions on that window's entries alone.
 *   -EINVAL with a seg_last_error text naming the function, and no launch, for: a null ctx,
 *   logits array, logits entry, ys, xs, cid_map or decisions_out; ny or nx < 1; more than
 *   SEG_WIN_MAX_ENTRIES entries; h_low or w_low < 1; ld < c1 + c2 + c3; flip outside 0..1;
 *   replace_voids outside 0..1 (2, seg_predict's PREDICT order, is not defined for averaged
 *   probabilities); a canvas smaller than the network size on either axis; an origin list that
 *   is not strictly increasing, does not start at 0, leaves a gap (ys[i + 1] > ys[i] + H) or
 *   whose last window does not end at the canvas edge (ys[ny - 1] + H != canvas_h), likewise xs
 *   with W and canvas_w -- together they give every canvas pixel k >= 1; a cid map of the wrong
 *   length or with an entry < -1; an output size < 1; mean_probs_out misaligned or given with an
 *   output size other than the canvas. */
#define SEG_WIN_MAX_ENTRIES 64
int seg_window_images(const float* in, int n, int Hc, int Wc, int y0, int x0, int H, int W,
                      int flip, float* out, void* stream);
int seg_window_decisions(seg_ctx* ctx, const float* const* logits, int h_low, int w_low, int ld,
                         const int* ys, int ny, const int* xs, int nx, int flip,
                         int canvas_h, int canvas_w, const int32_t* cid_map, int n_map,
                         int replace_voids, int out_h, int out_w,
                         float* mean_probs_out, int32_t* decisions_out, void* stream);

/* mean-field CRF refinement of the probabilities before the argmax (no reference counterpart: its
 * predict.py stops at the argmax; the semantics are fixed here). A Potts model with a bilateral
 * (position + colour) kernel plus a spatial kernel over a finite neighbourhood.
 * Inputs: probs = P, device fp32 [n][H][W][CT], the per-head probabilities (channels l1 | l2
 *   vehicle | l2 human, CT = c1 + c2 + c3 from ctx's head tables: 14 + 7 + 3 for Cityscapes,
 *   53 + 12 + 5 for Vistas) -- probs_out of seg_full_predictions, mean_probs_out of
 *   seg_tta_decisions or of seg_window_decisions; images = I, device fp32 [n][H][W][3], the
 *   prepared images in [-1, 1) at the same H x W. n, H, W are this call's arguments: H x W is
 *   whatever size the probabilities have (the network size, or the canvas of sliding windows) and
 *   need not be ctx's size; only the head tables and the cid-map rules come from ctx.
 * Parameters (seg_crf_params): iterations T, radius r, dilation d, the weights w_appearance (w_a)
 *   and w_smoothness (w_s), theta_alpha in pixels, theta_beta in grey levels of the 0..255 image,
 *   theta_gamma in pixels.
 * Neighbourhood: offsets o = (dy * d, dx * d) for dy, dx in -r..r without (0, 0), in row-major
 *   order of (dy, dx): K = (2r + 1)^2 - 1 offsets. A neighbour outside the image contributes
 *   nothing: no padding value, no renormalisation.
 * Kernel weight, the same for the three heads, from the image only; for pixel i and neighbour
 *   j = i + o:
 *     k_ij  = ga[o] * exp(-(|I_i - I_j|^2) * inv2b) + gs[o]
 *     ga[o] = (float)(w_a * exp(-|o|^2 / (2 theta_alpha^2)))
 *     gs[o] = (float)(w_s * exp(-|o|^2 / (2 theta_gamma^2)))
 *     inv2b = (float)(1 / (2 (theta_beta * 2 / 255)^2))
 *   ga[o], gs[o] and inv2b are formed on the host in double (|o|^2 = (dy^2 + dx^2) d^2) and
 *   rounded to float: they are part of the definition, like the resize tables elsewhere. One grey
 *   level is 2 / 255 in the prepared image. |I_i - I_j|^2 is the sum of the three squared channel
 *   differences in channel order; exp is the fast exp (__expf).
 * Iteration: Q^0 = P; for t = 0..T-1 every pixel is updated from Q^t (a parallel update over two
 *   buffers):
 *     m_i(c) = sum over o, in offset order, of k_ij * Q^t_j(c)             (fp32 accumulation)
 *     per head h: M_h = max over the head of m_i; v(c) = P_i(c) * exp(m_i(c) - M_h);
 *                 Z_h = sum of v in channel order; Q^{t+1}_i(c) = v(c) * (1 / Z_h)
 *   P_i(c) in v(c) is the unary, the original probability, not Q^t. If Z_h is not >= 1e-30f the
 *   head keeps P_i for that pixel. In the Potts model this is Q ~ exp(log P + message), written
 *   without a logarithm.
 * Decisions on Q^T exactly as seg_tta_decisions forms them on its sums: per-head first-maximum
 *   argmax -> hierarchical fusion -> cid_map (-1 -> max + 1) -> replace_voids = 1: the stable top-2
 *   of the l1 values (2, seg_predict's PREDICT order, is not defined here: -EINVAL) ->
 *   NEAREST_NEIGHBOR align_corners resize from H x W to out_h x out_w. decisions_out: device int32
 *   [n][out_h][out_w]. probs_out: optional (NULL skips it) device fp32 [n][H][W][CT] = Q^T,
 *   16-byte aligned, overlapping neither probs nor the workspace.
 * T = 0: no mean-field launch runs and Q = P exactly: decisions_out is bitwise what
 *   seg_tta_decisions writes for the single unflipped entry whose mean_probs_out is this P, and
 *   probs_out, if given, is a copy of P.
 * seg_crf_workspace: the bytes of the two Q buffers seg_crf_decisions needs when T >= 1 (each
 *   n * H * W * ct floats rounded up to 16 bytes). The workspace is the caller's; the entry
 *   neither allocates, frees nor synchronises.
 * -EINVAL with a seg_last_error text naming the function and the parameter, and no launch, for:
 *   iterations outside 0..32; radius outside 1..5; dilation outside 1..4; a weight < 0; a theta
 *   <= 0; any non-finite parameter; a null ctx, probs, images, p, cid_map or decisions_out; a null
 *   or too small workspace when T >= 1; probs, probs_out or the workspace not 16-byte aligned; n,
 *   H, W or an output size < 1; replace_voids outside 0..1; a cid map of the wrong length or with
 *   an entry < -1. */
typedef struct seg_crf_params {
  int iterations, radius, dilation;
  float w_appearance, w_smoothness;
  float theta_alpha, theta_beta, theta_gamma;
} seg_crf_params;
int seg_crf_workspace(int n, int H, int W, int ct, int64_t* bytes);
int seg_crf_decisions(seg_ctx* ctx, const float* probs, const float* images,
                      int n, int H, int W, const seg_crf_params* p,
                      void* workspace, int64_t workspace_bytes,
                      const int32_t* cid_map, int n_map, int replace_voids,
                      int out_h, int out_w,
                      float* probs_out, int32_t* decisions_out, void* stream);

/* box-constrained pseudo-labels: per-head probabilities plus the box list of a weakly labelled
 * image become per-pixel training labels (no reference counterpart; the semantics are fixed here).
 * Notation: t = ctx's head tables: c1, c2, c3, cid_l1_vehicle, cid_l1_human, pb2veh[15],
 *   pb2hum[15], l1_to_common, veh_to_common, hum_to_common, n_pp. The void channel of a head is its
 *   last channel. IGNORE = n_pp - 1, the void training cid (19 Cityscapes, 65 Vistas). CT = c1 +
 *   c2 + c3, channels l1 | l2 vehicle | l2 human as for seg_crf_decisions.
 * Box kinds: a box of weak class k (0..13) is a vehicle box if pb2veh[k] != c2 - 1, a human box if
 *   pb2hum[k] != c3 - 1, inert otherwise (classes 11..13 in both datasets).
 * Cover: boxes, cids, box_off, geom and max_boxes are those of seg_bbox_labels (below) without
 *   flip, and so is the mapping: rectangles are (int)((double)coord * size) at the source size;
 *   pixel (y, x) of the H x W map has the source pixel
 *   min((int)floorf((float)(y + oy) * ((float)src_h / (float)rh)), src_h - 1), likewise in x;
 *   inclusion is >= min && <= max on both axes. Pixel i is covered by box b if its source pixel
 *   lies in b's rectangle. mask_i has bit k set if some box of class k covers i.
 *   AV_i = { pb2veh[k] : bit k set, vehicle box }, AH_i likewise with pb2hum for human boxes.
 * n, H, W are each call's own, as for seg_crf_decisions; only the tables come from ctx. All
 *   pointers are device memory.
 *
 * seg_box_constrain: probs = P, fp32 [n][H][W][CT] -> probs_out = P', same layout, not P. The l1
 *   channels are copied bit for bit. Vehicle head: AV_i empty: copied bit for bit. Otherwise the
 *   channels outside AV_i become +0.0f (the void channel included), s = the fp32 sum of the kept
 *   channels in channel order, and the kept channels become P(c) * (1.f / s); if !(s >= 1e-30f)
 *   the head is copied unchanged (the CRF's rule). Human head: the same with AH_i. mask_out:
 *   optional (NULL skips it) uint16 [n][H][W] = mask_i. seg_crf_decisions multiplies its message
 *   into the unary, so a zero of P' stays zero through every mean-field step: constrain first,
 *   refine second.
 * seg_box_decisions: q = Q, fp32 [n][H][W][CT] (P', or probs_out of seg_crf_decisions run on P')
 *   -> labels_out int32 [n][H][W], training cids at the size of the probabilities. d1 = the
 *   first-maximum argmax of the l1 values, conf = Q_l1[d1]. d1 == cid_l1_vehicle: IGNORE if AV_i
 *   is empty (a vehicle with no box behind it), else veh_to_common[d2], d2 the first maximum over
 *   the channels of AV_i only, in channel order. d1 == cid_l1_human: the same with AH_i and
 *   hum_to_common. Any other d1: l1_to_common[d1]. If !(conf >= tau) the label is IGNORE.
 *   conf_out: optional fp32 [n][H][W]. counts_out: int32 [total_boxes][2] = (area_b, hit_b):
 *   area_b the pixels of its image covered by b; hit_b those of them whose label equals
 *   veh_to_common[pb2veh[k]] for a vehicle box of class k, hum_to_common[pb2hum[k]] for a human
 *   box, 0 for an inert box. The entry zeroes counts_out itself, on the stream; the sums are
 *   integers, exact in any order.
 * seg_box_finalize: labels int32 [n][H][W], reject int32 [total_boxes] -> out int32
 *   [n][out_h][out_w]: every output pixel takes the label of its NEAREST_NEIGHBOR align_corners
 *   source pixel (as the decision entries resize) and becomes IGNORE if any box with
 *   reject[b] != 0 covers that source pixel. The caller forms reject on the host: 1 if b is a
 *   vehicle or human box (seg_box_kinds), area_b > 0 and hit_b < min_fill * area_b in float64; inert
 *   boxes and boxes of zero area are never rejected.
 * -EINVAL with a seg_last_error text naming the function and the parameter, no launch and the
 *   outputs unwritten, for: a null ctx, probs / q / labels, boxes, cids, box_off, geom, probs_out,
 *   labels_out, counts_out, reject or out; n, H, W or an output size < 1 (n above 65535);
 *   max_boxes outside 0..1024; probs, q or probs_out not 16-byte aligned; probs_out == probs; tau
 *   not finite or outside [0, 1]. Head widths other than the two datasets' are an error. Class ids
 *   outside 0..13 and a geom whose crop leaves the resized map are the caller's to refuse. */
/* seg_box_kinds: the kind of every weak class under ctx's head tables, host int32 kinds[14]:
 *   1 vehicle box, 2 human box, 0 inert -- what the host's reject rule needs to know. Host-only. */
int seg_box_kinds(seg_ctx* ctx, int32_t* kinds);
int seg_box_constrain(seg_ctx* ctx, const float* probs, int n, int H, int W,
                      const float* boxes, const int32_t* cids, const int32_t* box_off,
                      const int32_t* geom, int max_boxes,
                      float* probs_out, uint16_t* mask_out, void* stream);
int seg_box_decisions(seg_ctx* ctx, const float* q, int n, int H, int W,
                      const float* boxes, const int32_t* cids, const int32_t* box_off,
                      const int32_t* geom, int max_boxes, float tau,
                      int32_t* labels_out, float* conf_out, int32_t* counts_out, void* stream);
int seg_box_finalize(seg_ctx* ctx, const int32_t* labels, int n, int H, int W,
                     const float* boxes, const int32_t* cids, const int32_t* box_off,
                     const int32_t* geom, int max_boxes, const int32_t* reject,
                     int out_h, int out_w, int32_t* out, void* stream);

/* input preprocessing (input_cityscapes.py:66-96,190-209), after the host
 * decodes TFRecord -> tf.train.Example -> PNG (input_pipelines/tfrecords.py):
 * seg_prepare_images: raw uint8 [n][src_h][src_w][3] -> convert_image_dtype -> bilinear
 *   resize_images (align_corners = False) to H x W -> from_0_1_to_m1_1 -> fp32 [n][H][W][3]
 * seg_prepare_labels: raw uint8 label ids [n][src_h][src_w] -> lids2cids[n_lids] (-1 = void
 *   -> max + 1) -> nearest resize to H x W -> int32 [n][H][W] (-1 for ids outside the table) */
int seg_prepare_images(const uint8_t* raw, int n, int src_h, int src_w, int H, int W, float* out,
                       void* stream);
int seg_prepare_labels(const uint8_t* raw, int n, int src_h, int src_w, int H, int W,
                       const int32_t* lids2cids, int n_lids, int32_t* out, void* stream);
/* seg_prepare_images_crop: the weak-label streams' image path (resize_images_and_labels with
 *   preserve_aspect_ratio, input_pipelines/utils.py:181-241, under the OpenImages train inputs,
 *   input_subset_bboxes_v2.py:111-125): convert_image_dtype -> bilinear resize (align_corners =
 *   False) to resized_h x resized_w -> the H x W window at (crop_y, crop_x) -> from_0_1_to_m1_1.
 *   Only the window is computed; bitwise the same values as resizing and slicing. */
int seg_prepare_images_crop(const uint8_t* raw, int n, int src_h, int src_w, int resized_h,
                            int resized_w, int crop_y, int crop_x, int H, int W, float* out,
                            void* stream);

/* checkpoint interop (define_initializers.py:72-131, define_savers.py:38-66): CRC-32C of
 * host bytes, continuing from `crc` (0 to start) — the checksum TF tensor bundles
 * (<prefix>.index / <prefix>.data-*) keep per tensor and per table block. Host-only. */
uint32_t seg_crc32c(uint32_t crc, const void* data, size_t n);

/* loss scaling (fp16 storage, BASELINE config C5: fp16 with fp32 master gradients). The
 * gradient seed of seg_loss is multiplied by `scale`; seg_apply_update first flags non-finite
 * weight/BN gradients (device int, seg_found_inf), unscales them by grad_scale / scale (the BN
 * batch-statistics tail by grad_scale only) and skips the parameter update of a flagged step.
 * The caller adjusts the scale from the flag (dynamic loss scaling). */
int seg_set_loss_scale(seg_ctx* ctx, float scale);
int seg_found_inf(seg_ctx* ctx, const int32_t** flag_device);

/* cross-replica (synchronised) batch norm, the reference's --cross_replica_norm
 * (models/resnet50_extended_model_hierarchical.py:327-328 -> utils/cross_replica_batch_
 * normalization.py:393-476). With a hook set, every BN layer of seg_forward exchanges its
 * per-channel [mean | E[x^2]] (2C floats) and normalises with the replica average: mean,
 * variance E[x^2] - mean^2 (biased; it also feeds the moving variance, as the reference's
 * non-fused path does); every BN layer of seg_backward exchanges [mean(dyhat) |
 * mean(dyhat * xhat)] so dx is the gradient through the global statistics. `allreduce` must
 * SUM `n` floats at the device pointer `buf` in place across the `world` replicas, ordered
 * on `stream` (e.g. torch.distributed.all_reduce on that stream, RCCL or gloo), and return 0;
 * a nonzero return fails the step. fn = NULL turns synchronisation off; world = 1 with a hook
 * still calls it (a one-replica exchange: the sync-BN arithmetic over one replica). */
typedef int (*seg_allreduce_fn)(void* user, float* buf, int64_t n, void* stream);
int seg_set_bn_sync(seg_ctx* ctx, seg_allreduce_fn allreduce, void* user, int world);

/* gradient all-reduce buckets, in the order the backward completes them: n buckets
 * [lo[i], hi[i]) of the flat [grads | BN stats] buffer (conv-weight ranges cut at layer
 * boundaries, about SEG_BUCKET_MB = 32 MB each, then the BN-parameter + statistics tail);
 * returns n (fills at most max_buckets). seg_backward records one event per bucket when its
 * gradients are written; seg_stream_wait_bucket makes `stream` wait for it (the caller's
 * collective for bucket i then overlaps the rest of the backward). */
int seg_grad_buckets(seg_ctx* ctx, int max_buckets, int64_t* lo, int64_t* hi);
int seg_stream_wait_bucket(seg_ctx* ctx, int bucket, void* stream);

/* weak-label maps on the device (input_subset_bboxes_v2.py:74-98 rasterisation fused with the
 * aspect-preserving nearest-neighbour resize + crop of input_pipelines/utils.py:181-241;
 * input_subset_image_labels.py:73-107 for tags). All pointers are device memory:
 *   boxes [total][4] (xmin, xmax, ymin, ymax) normalised to [0,1], cids [total] in [0,13],
 *   box_off [n+1] per-image prefix offsets into boxes, geom [n][6] = (src_h, src_w, resized_h,
 *   resized_w, crop_y, crop_x); max_boxes = the largest per-image count (<= 1024);
 *   out [n][H][W][15] fp32 multinomials (channel 14 = void). tags [n][15] normalised. */
int seg_bbox_labels(const float* boxes, const int32_t* cids, const int32_t* box_off,
                    const int32_t* geom, int n, int max_boxes, int H, int W, float* out,
                    void* stream);
int seg_tag_labels(const float* tags, int n, int H, int W, float* out, void* stream);

/* seg_bbox_labels with a per-image mirror (random_flipping applied to a bbox-weak image and its
 * label map, augmentation_library.py:298-321): flip is device int32 [n], a nonzero entry makes
 * output pixel x rasterise column W-1-x of the unflipped map; NULL = no image flipped. */
int seg_bbox_labels_flip(const float* boxes, const int32_t* cids, const int32_t* box_off,
                         const int32_t* geom, const int32_t* flip, int n, int max_boxes, int H,
                         int W, float* out, void* stream);

/* training augmentation on the device (preprocessing/augmentation_library.py: random_color
 * :359-406, random_blur :408-466, random_flipping :298-321, random_scaling :21-296), the call
 * block the reference's train pipelines hold between the resize and from_0_1_to_m1_1
 * (input_cityscapes.py:106-118). The random draws are the caller's: one record per image, and
 * the kernels are pure functions of (raw input, record). Per image: resize (as
 * seg_prepare_images_crop) -> colour -> blur -> flip stage -> scaling -> (x - 0.5) / 0.5.
 *   colour  color_order -1 = none, else the op order 0: B S H C, 1: S B C H, 2: C H B S,
 *           3: H S C B, then clip to [0, 1]. B: x + brightness_delta; S / H: through HSV,
 *           s = clip(s * saturation_factor, 0, 1) / h = frac(h + hue_delta);
 *           C: (x - m) * contrast_factor + m, m = per-channel mean of the image entering the op
 *   blur    blur.mode 0 = none; 1 median, as cv2.medianBlur on 8-bit data: q = trunc(x * 255),
 *           per-channel median of the blur.ksize^2 window with replicated borders, q / 255;
 *           2 bilateral, as cv2.bilateralFilter on float data with sigmaColor = sigmaSpace =
 *           blur.sigma: taps (i, j) with i^2 + j^2 <= (blur.ksize / 2)^2, reflect-101 borders,
 *           weight exp(-(i^2 + j^2) / (2 sigma^2)) * exp(-(|dR| + |dG| + |dB|)^2 / (2 sigma^2)),
 *           weighted mean per channel (the closed form; cv2's interpolated colour-weight table
 *           is not reproduced). blur.ksize is odd, 3..9. An all-zero blur (what a caller that
 *           zeroes the former padding words passes) is no blur. Labels are untouched
 *   flip    quantize = 1 (the stage is enabled): the image goes through uint8 (trunc(x * 255.5))
 *           and back (q * (1 / 255)), flipped or not; flip = 1 mirrors image and label in x
 *   scale   scale_mode 0 none; 1 up: crop (sh, sw) at (oy, ox), uint8 round trip, legacy bilinear
 *           resize back to H x W (labels: nearest); 2 down: legacy bilinear resize to (sh, sw)
 *           (labels: nearest) placed at ((H - sh) / 2, (W - sw) / 2), the rest filled with the
 *           scalar mean of the resized image (labels: void_cid)
 * A record is SEG_AUG_PARAMS_BYTES = 64 bytes. */
#define SEG_AUG_PARAMS_BYTES 64
typedef struct seg_aug_blur {   /* the last 12 bytes of the record */
  int32_t mode, ksize;
  float sigma;
} seg_aug_blur;
typedef struct seg_aug_params {
  int32_t color_order;
  float brightness_delta, saturation_factor, hue_delta, contrast_factor;
  int32_t quantize, flip;
  int32_t scale_mode;
  int32_t sh, sw;
  int32_t oy, ox;
  int32_t void_cid;
  seg_aug_blur blur;
} seg_aug_params;
/* The table is passed twice: params_host (host memory) is validated before anything is launched
 * and supplies the host-divided resize scales, params_dev (device memory, the same n records) is
 * what the kernels read. -EINVAL with a seg_last_error text, and no launch, for: a scaled size
 * outside 1..H x 1..W, a crop outside the image, color_order outside -1..3, scale_mode outside
 * 0..2, blur.mode outside 0..2, with a blur an even blur.ksize or one outside 3..9, for the
 * bilateral a blur.sigma that is not finite and positive or min(H, W) < blur.ksize / 2 + 1, a window outside the resized image, a workspace smaller than seg_augment_workspace says,
 * out or workspace not 16-byte aligned.
 * seg_augment_images: raw uint8 [n][src_h][src_w][3] + the geometry of seg_prepare_images_crop
 *   (plain resize: resized = H x W, crop 0, 0) -> fp32 [n][H][W][3]. workspace (device) holds the
 *   stage between the colour pass and the geometric pass (the blur pass moves an image between
 *   the stage and out, never in place) and the partial sums of the two means;
 *   both means are reduced in a fixed order (no atomics): same inputs, bitwise same output.
 *   With an all-off record the output is bitwise seg_prepare_images_crop's.
 * seg_augment_labels: raw uint8 ids [n][src_h][src_w] + lids2cids as seg_prepare_labels -> one
 *   gather (scaling's nearest resize / void_cid pad, flip, the prepare step's nearest resize)
 *   -> int32 [n][H][W]. Colour fields are ignored. */
int seg_augment_workspace(int n, int H, int W, int64_t* bytes);
int seg_augment_images(const uint8_t* raw, int n, int src_h, int src_w, int resized_h,
                       int resized_w, int crop_y, int crop_x, int H, int W,
                       const seg_aug_params* params_host, const seg_aug_params* params_dev,
                       float* out, void* workspace, int64_t ws_bytes, void* stream);
int seg_augment_labels(const uint8_t* raw, int n, int src_h, int src_w, int H, int W,
                       const int32_t* lids2cids, int n_lids, const seg_aug_params* params_host,
                       const seg_aug_params* params_dev, int32_t* out, void* stream);
/* pass timing of seg_augment_images (diagnostics, tools/aug_table.py; no reference counterpart):
 * enable != 0 makes later calls record events around their four passes (contrast mean, colour,
 * down-scale mean, geometry); with pass_ms != NULL the call first waits for the last recorded
 * call and stores its four pass times in milliseconds (0 for a skipped pass). Synchronises; not
 * for use while a stream is being captured. */
int seg_augment_profile(int enable, float* pass_ms);
/* the blur pass (between colour and down-scale mean) of the same recorded call, in milliseconds;
 * the empty interval between two events (microseconds) when no image of the call had a blur.
 * Profiling must be enabled; synchronises. */
int seg_augment_profile_blur(float* blur_ms);

/* internal tensors for parity tests: "logits", "grad_un", "dzscale", "feat", "dfeat", "z0",
 * "head<h>_out", "head<h>_dout", "pyr<b>_z" (pyramid branch b's BN + ReLU output at its pooled
 * resolution), "conv<i>_x" (input of the last forward), "conv<i>_y", "conv<i>_dy" (i =
 * creation index); after seg_set_bootstrap enabled it once: "l1_loss_map" ([nb_pp, H, W, 1] f32)
 * and "bootstrap_tau" (one float) of the last bootstrapped seg_loss.
 * dims = N, H, W, C; ld = pixel stride; dtype = SEG_DTYPE_* of the storage */
int seg_debug_tensor(seg_ctx* ctx, const char* name, void** ptr, int* dims, int* ld, int* dtype);

/* kernel-time profiling: conv classes 0 fwd, 1 dgrad, 2 wgrad (gflop = algorithmic flops);
 * BN classes 3 apply, 4 bwd reduce, 5 bwd apply (gflop field = algorithmic GB moved) ---- */
int seg_profile(seg_ctx* ctx, int enable);
int seg_profile_read(seg_ctx* ctx, int cls, double* ms_total, double* gflop_total,
                     int64_t* launches, double* ms_max_layer, char* layer_name, int name_len);
/* one text line per recorded launch: cls name ci co k rate Ho Wo gflop ms gbytes
 * (gbytes = the launch's compulsory HBM GB: every operand read / written once) */
int seg_profile_dump(seg_ctx* ctx, char* buf, int len);

/* single-op entry points (parity tests of individual kernels) -------------------------- */
int seg_op_conv_fwd(int dtype, const void* x, int N, int H, int W, int C, int ldx,
                    const void* w, int Co, int k, int stride, int rate, int explicit_pad,
                    void* y, int ldy, float* stats, void* stream);
/* rows per BN-statistics partial written by seg_op_conv_fwd for this shape (128 or 256) */
int seg_op_conv_stat_rows(int dtype, int N, int H, int W, int C, int ldx, int Co, int ldy, int k,
                          int stride, int rate, int explicit_pad);
int seg_op_conv_dgrad(int dtype, const void* dy, int N, int Ho, int Wo, int Co, int lddy,
                      const void* w, int Ci, int k, int stride, int rate, int explicit_pad,
                      int H, int W, void* dx, int lddx, void* stream);
/* a 1 x 1 stride-1 data gradient with the identity units' epilogue: dx = dgrad(dy) + r (r may
 * be NULL; it may alias dx), stored masked by omask (ReLU bits [M][Ci/8], bit e of byte n/8 =
 * channel n; NULL = unmasked) -- the launches of the pre-masked residual chain (DESIGN.md §5b'',
 * §5f); 16-bit dtypes take the ping-pong kernel for Ci > 128: with r, persistent with the
 * residual tile by LDS-DMA and one rounding of dgrad + r (RQP); without, one tile per
 * workgroup */
int seg_op_conv_dgrad_res(int dtype, const void* dy, int N, int H, int W, int Co, int lddy,
                          const void* wt, int Ci, void* dx, int lddx, const void* r, int ldr,
                          const uint8_t* omask, void* stream);
int seg_op_conv_wgrad(int dtype, const void* dy, int N, int Ho, int Wo, int Co, int lddy,
                      const void* x, int H, int W, int Ci, int ldx, int k, int stride, int rate,
                      int explicit_pad, float* dw, void* workspace, int64_t ws_bytes,
                      void* stream);
/* bf16 weight gradient with an explicit tile (bm co x bn columns, each 64/128/256) and
 * split count: reaches every kernel configuration at test sizes (256 x 256 = ping-pong) */
int seg_op_conv_wgrad_cfg(int dtype, const void* dy, int N, int Ho, int Wo, int Co, int lddy,
                          const void* x, int H, int W, int Ci, int ldx, int k, int stride, int rate,
                          int explicit_pad, float* dw, void* workspace, int64_t ws_bytes, int bm,
                          int bn, int splits, void* stream);
/* the fused data-gradient launches of the runtime, stride 1, k in {1, 3} (rate 1 for k = 1),
 * SAME geometry: dx = dgrad(dy) [+ dy2 . wt2 (1 x 1, Co2 channels)] [+ r1] [+ r2], stored masked
 * by omask (as seg_op_conv_dgrad_res; NULL = unmasked). wt [Ci][k][k][Co] flipped, wt2 [Ci][Co2];
 * r1 may alias dx. -EINVAL for the combinations the runtime never launches: r2 without r1, dy2
 * with a residual, with k = 3 or with a 32-bit dtype, a mask where no masked launch exists */
int seg_op_conv_dgrad_fused(int dtype, const void* dy, int N, int H, int W, int Co, int lddy,
                            const void* wt, int Ci, int k, int rate, void* dx, int lddx,
                            const void* r1, int ldr1, const void* r2, int ldr2, const void* dy2,
                            int Co2, int lddy2, const void* wt2, const uint8_t* omask,
                            void* stream);
/* read-only: which kernel a conv request runs on (csrc/conv_select.h), written into buf as one
 * line of key=value words, e.g. "kernel=pp tile=256x256 st=0 persist=1 ... stat_rows=128
 * omask=0 wgs=4096 lds=131072", or "kernel=invalid reason=..." (the reason runs to the end of
 * the line). No GPU is touched. f = the nf scalar fields of the argument struct in declaration
 * order (csrc/conv_args.h):
 *   conv (nf 24): N H W C ldx ldw Ho Wo Co ldy ldr ldr2 KH KW sf st pad_h pad_w dil tap8 ldx2 C2
 *                 ldw2 ldm; flags: 1 residual, 2 second residual, 4 statistics, 8 mask,
 *                 16 second GEMM
 *   wgrad (nf 18): lddy N H W C ldx Ho Wo Co KH KW sf pad_h pad_w dil splits lddy2 Co1;
 *                 flags: 1 second dy source; force_bm / force_bn: 0, or the forced tile of
 *                 seg_op_conv_wgrad_cfg
 * Returns 0, -EINVAL for a bad argument, -ENOSPC when len is too small. */
int seg_op_conv_plan(int dtype, int out_f32, const int* f, int nf, int flags, char* buf, int len);
int seg_op_conv_wgrad_plan(int dtype, const int* f, int nf, int flags, int force_bm, int force_bn,
                           char* buf, int len);
/* the threshold select of seg_set_bootstrap on any device array of n finite floats >= +0 (a set
 * sign bit, -0.0f included, is outside the contract): *tau_out = the k-th largest entry,
 * *n_ge_out = the count of entries >= tau (both host pointers; the call synchronises `stream`
 * and allocates its own workspace). -EINVAL for k < 1, k > n or n > 2^31 - 1. */
int seg_op_bootstrap_threshold(const float* map, int64_t n, int64_t k, float* tau_out,
                               int64_t* n_ge_out, void* stream);

/* single batch-norm launches, as the network issues them (csrc/bn.h). Every buffer is
 * a caller-owned device buffer, per-channel vectors are [C] floats, rows are pixels (ld = pixel
 * stride in elements). dtype = SEG_DTYPE_* of y and of the 16-bit outputs. -EINVAL with a
 * seg_last_error text, and no launch, for a bad argument and for every combination the
 * launchers refuse. */
/* the row blocks of the backward reduce for M rows: the caller sizes seg_bn_bwd_args.part as
 * [rb][C][2] floats and cs_part as [rb][C] */
int seg_op_bn_rowblocks(int64_t M, int C);
/* forward statistics from the conv epilogue's per-tile partials part [ceil(M / tile_rows)][C][2]
 * = (sum, M2 about the tile mean) of tile_rows rows each (the last tile ragged): mean, invstd =
 * rsqrt(var + eps), scale = gamma invstd, var_unb = var N / (N - 1), and pack [2C] = [mean |
 * E[x^2]] when not NULL */
int seg_op_bn_stats_finalize(const float* part, int64_t M, int C, int tile_rows, const float* gamma,
                             float* mean, float* invstd, float* scale, float* var_unb, float* pack,
                             void* stream);
/* out = act((y - mean) scale + beta [+ res | + (y2 - mean2) scale2 + beta2]); res subsampled by rs
 * over an [N][Hr][Wr] grid when rs > 1 (the output grid is [N][Ho][Wo]); mask (nullable, with
 * relu, 8-wide layouts only): bits [M][C/8] of out > 0 as stored */
typedef struct seg_bn_apply_args {
  const void* y; int ldy;
  int64_t M; int C;
  const float* mean; const float* scale; const float* beta;
  int relu;
  const void* res; int ldres; int rs; int Ho, Wo, Hr, Wr;
  const void* y2; int ldy2; const float* mean2; const float* scale2; const float* beta2;
  void* out; int ldo;
  uint8_t* mask;
} seg_bn_apply_args;
int seg_op_bn_apply(int dtype, int out_f32, const seg_bn_apply_args* a, void* stream);
/* one layer's backward: reduce into part, finalize (dgamma, dbeta nullable; sdy = dbeta / M,
 * sdyx = dgamma / M, both 0 when frozen), then, unless reduce_only, the apply
 * dy = scale (dyhat - sdy - xhat sdyx), where dyhat = gate(dz + dshift) dzscale. The gate is z > 0
 * or the bits in mask, not both; with the bits, dzscale reaches the apply only (group norm's
 * gamma: the sums are those of the gated dz). dyhat (nullable) receives the gated gradient before dzscale,
 * from the apply, or from the reduce when reduce_only. cs_part with beta (16-bit, with dshift):
 * per row block column sums of the forward output relu((y - mean) scale + beta) as stored. */
typedef struct seg_bn_bwd_args {
  const void* dz; int lddz;          /* dtype, or float when dz_f32 */
  const void* z; int ldz;            /* the type of dz */
  const uint8_t* mask;
  const void* y; int ldy;
  int64_t M; int C;
  const float* mean; const float* invstd; const float* scale;
  float* sdy; float* sdyx;
  void* dy; int lddy;
  void* dyhat; int lddyhat;
  const float* dzscale; const float* dshift;
  const float* beta; float* cs_part;
  float* part;
  float* dgamma; float* dbeta;
} seg_bn_bwd_args;
int seg_op_bn_backward(int dtype, int dz_f32, int frozen, int reduce_only, const seg_bn_bwd_args* a,
                       void* stream);
/* two layers gated by the same dz and bits (a->dz, a->mask): one dual reduce, a finalize each,
 * one dual apply; b supplies the second layer's y, statistics, outputs and partials (same M, C).
 * second_only: dz arrived gated, and only the second layer's apply runs, ungated. */
int seg_op_bn_backward_dual(int dtype, int frozen, int second_only, const seg_bn_bwd_args* a,
                            const seg_bn_bwd_args* b, void* stream);

#ifdef __cplusplus
}
#endif
#endif
