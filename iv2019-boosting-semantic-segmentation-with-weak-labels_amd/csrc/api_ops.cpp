// The context-free entries of the C ABI (include/seg_hip.h): single conv launches for tests and
// tools, label / input / augmentation preparation, the test-time augmentation image pyramid, the
// sliding-window extraction, the bootstrap threshold and the checkpoint CRC.
#include "net.h"

using namespace segnet;

namespace {

int bbox_labels(const char* who, const float* boxes, const int32_t* cids,
                const int32_t* box_off, const int32_t* geom, const int32_t* flip, int n,
                int max_boxes, int H, int W, float* out, void* stream) {
  if (n < 0 || H <= 0 || W <= 0 || (n > 0 && (!box_off || !geom || !out)))
    return set_err(nullptr, -EINVAL, "%s: bad arguments", who);
  if (max_boxes < 0 || max_boxes > 1024)
    return set_err(nullptr, -E2BIG, "%s: at most 1024 boxes per image (reference 516)", who);
  static_assert(sizeof(BboxGeom) == 6 * sizeof(int32_t), "geom layout");
  hipError_t e = launch_bbox_labels(boxes, cids, box_off, (const BboxGeom*)geom, flip, n, H, W, out,
                                    (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, who);
}

LidMap lid_map(const int32_t* lids2cids, int n_lids) {
  LidMap m{};
  m.n = n_lids;
  int mx = -1;
  for (int i = 0; i < n_lids; ++i) mx = std::max(mx, (int)lids2cids[i]);
  for (int i = 0; i < n_lids; ++i)   // utils._replacevoids: -1 -> max + 1
    m.cid[i] = lids2cids[i] == -1 ? mx + 1 : lids2cids[i];
  return m;
}

static_assert(sizeof(seg_aug_params) == sizeof(AugParams) && sizeof(AugParams) == SEG_AUG_PARAMS_BYTES,
              "seg_aug_params layout");
static_assert(offsetof(seg_aug_params, blur) == offsetof(AugParams, blur_mode) &&
              offsetof(seg_aug_params, blur) + offsetof(seg_aug_blur, ksize) == offsetof(AugParams, blur_ksize) &&
              offsetof(seg_aug_params, blur) + offsetof(seg_aug_blur, sigma) == offsetof(AugParams, blur_sigma) &&
              offsetof(AugParams, blur_mode) == 52, "seg_aug_params blur words");

// the shared checks of the two augmentation entries: the table is validated from the caller's
// host copy before anything is launched
int aug_check(const char* who, int n, int H, int W, const seg_aug_params* params_host,
              const seg_aug_params* params_dev) {
  if (n > 0 && (!params_host || !params_dev))
    return set_err(nullptr, -EINVAL, "%s: the parameter table is required on the host and on the device", who);
  char msg[256];
  if (aug_validate((const AugParams*)params_host, n, H, W, msg, sizeof msg))
    return set_err(nullptr, -EINVAL, "%s: %s", who, msg);
  return 0;
}

void op_geom(int H, int W, int k, int stride, int rate, int explicit_pad, int* Ho, int* Wo,
             int* ph, int* pw) {
  ConvL L;
  L.k = k; L.stride = stride; L.rate = rate; L.explicit_pad = explicit_pad != 0;
  conv_geom(L, 1, H, W);
  *Ho = L.Ho; *Wo = L.Wo; *ph = L.pad_h; *pw = L.pad_w;
}

bool bad_dtype(int dtype) {
  return dtype != SEG_DTYPE_F32 && dtype != SEG_DTYPE_BF16 && dtype != SEG_DTYPE_F16;
}

// the pointers and strides every BN-backward entry needs (dy only where an apply runs)
int bn_bwd_check(const char* who, int dtype, const seg_bn_bwd_args* p, bool need_dy) {
  if (!p || bad_dtype(dtype) || !p->dz || !p->y || !p->mean || !p->invstd || !p->scale || !p->sdy ||
      !p->sdyx || !p->part || p->M < 1 || p->C < 1 || p->lddz < p->C || p->ldy < p->C ||
      (need_dy && (!p->dy || p->lddy < p->C)))
    return set_err(nullptr, -EINVAL, "%s: bad arguments", who);
  return 0;
}

// the network's bn_bwd_args (net_layers.cpp) from the C struct; rb as the network sizes it
BnBwdArgs bn_bwd_op_args(const seg_bn_bwd_args* p) {
  BnBwdArgs a{};
  a.dz = p->dz; a.lddz = p->lddz;
  a.z = p->z; a.ldz = p->ldz; a.mask = p->mask;
  a.y = p->y; a.ldy = p->ldy; a.M = (long)p->M; a.C = p->C;
  a.mean = p->mean; a.invstd = p->invstd; a.scale = p->scale;
  a.sdy = p->sdy; a.sdyx = p->sdyx;
  a.dy = p->dy; a.lddy = p->lddy;
  a.dyhat = p->dyhat; a.lddyhat = p->lddyhat;
  a.dzscale = p->dzscale; a.dshift = p->dshift;
  a.beta = p->beta; a.cs_part = p->cs_part;
  a.part = p->part; a.rb = bn_bwd_rowblocks(a.M);
  return a;
}

// ---- checkpoint interop: CRC-32C (Castagnoli) of host bytes, the checksum TF 1.12 tensor
// bundles store per tensor and per table block (tensorflow/core/lib/hash/crc32c.h), used by
// utils/tf_checkpoint.py to read / write <prefix>.index + <prefix>.data-* checkpoints
struct Crc32cTables {
  uint32_t t[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFF];
  }
};
const Crc32cTables& crc_tables() {
  static const Crc32cTables tb;
  return tb;
}

}  // namespace

extern "C" {

int seg_op_bootstrap_threshold(const float* map, int64_t n, int64_t k, float* tau_out,
                               int64_t* n_ge_out, void* stream) {
  if (!map || !tau_out || !n_ge_out) return set_err(nullptr, -EINVAL, "seg_op_bootstrap_threshold: null argument");
  if (n < 1 || n > 2147483647ll || k < 1 || k > n)
    return set_err(nullptr, -EINVAL, "seg_op_bootstrap_threshold: need 1 <= k <= n <= 2^31 - 1 (k %lld, n %lld)",
                   (long long)k, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  void* ws = nullptr;
  hipError_t e = hipMalloc(&ws, BOOTSTRAP_SLAB_BYTES + sizeof(BootstrapState));
  if (e != hipSuccess) return hip_fail(nullptr, e, "seg_op_bootstrap_threshold");
  BootstrapState* st = (BootstrapState*)((char*)ws + BOOTSTRAP_SLAB_BYTES);
  BootstrapState host{};
  e = launch_bootstrap_select(map, n, k, (unsigned*)ws, st, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&host, st, sizeof(host), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(ws);
  if (e != hipSuccess) return hip_fail(nullptr, e, "seg_op_bootstrap_threshold");
  *tau_out = host.tau;
  *n_ge_out = host.n_ge;
  return 0;
}

int seg_bbox_labels(const float* boxes, const int32_t* cids, const int32_t* box_off,
                    const int32_t* geom, int n, int max_boxes, int H, int W, float* out,
                    void* stream) {
  return bbox_labels("seg_bbox_labels", boxes, cids, box_off, geom, nullptr, n, max_boxes, H, W, out,
                     stream);
}

int seg_bbox_labels_flip(const float* boxes, const int32_t* cids, const int32_t* box_off,
                         const int32_t* geom, const int32_t* flip, int n, int max_boxes, int H,
                         int W, float* out, void* stream) {
  return bbox_labels("seg_bbox_labels_flip", boxes, cids, box_off, geom, flip, n, max_boxes, H, W,
                     out, stream);
}

int seg_tag_labels(const float* tags, int n, int H, int W, float* out, void* stream) {
  if (n < 0 || H <= 0 || W <= 0 || (n > 0 && (!tags || !out)))
    return set_err(nullptr, -EINVAL, "seg_tag_labels: bad arguments");
  hipError_t e = launch_tag_labels(tags, n, H, W, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_tag_labels");
}

int seg_prepare_images(const uint8_t* raw, int n, int src_h, int src_w, int H, int W, float* out,
                       void* stream) {
  if (n < 0 || src_h <= 0 || src_w <= 0 || H <= 0 || W <= 0 || (n > 0 && (!raw || !out)))
    return set_err(nullptr, -EINVAL, "seg_prepare_images: bad arguments");
  hipError_t e = launch_prepare_images(raw, n, src_h, src_w, H, W, 0, 0, H, W, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_prepare_images");
}

int seg_prepare_images_crop(const uint8_t* raw, int n, int src_h, int src_w, int resized_h,
                            int resized_w, int crop_y, int crop_x, int H, int W, float* out,
                            void* stream) {
  if (n < 0 || src_h <= 0 || src_w <= 0 || H <= 0 || W <= 0 || (n > 0 && (!raw || !out)) ||
      crop_y < 0 || crop_x < 0 || crop_y + H > resized_h || crop_x + W > resized_w)
    return set_err(nullptr, -EINVAL, "seg_prepare_images_crop: bad arguments (window %d,%d + %dx%d "
                   "outside the resized %dx%d)", crop_y, crop_x, H, W, resized_h, resized_w);
  hipError_t e = launch_prepare_images(raw, n, src_h, src_w, resized_h, resized_w, crop_y, crop_x,
                                       H, W, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_prepare_images_crop");
}

int seg_resize_images(const float* in, int n, int H, int W, int h_out, int w_out, int flip,
                      float* out, void* stream) {
  if (n < 0 || H <= 0 || W <= 0 || h_out <= 0 || w_out <= 0 || (n > 0 && (!in || !out)))
    return set_err(nullptr, -EINVAL, "seg_resize_images: bad arguments");
  if (flip < 0 || flip > 1) return set_err(nullptr, -EINVAL, "seg_resize_images: flip = %d (0 or 1)", flip);
  hipError_t e = launch_resize_images(in, n, H, W, h_out, w_out, flip, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_resize_images");
}

int seg_window_images(const float* in, int n, int Hc, int Wc, int y0, int x0, int H, int W,
                      int flip, float* out, void* stream) {
  const char* who = "seg_window_images";
  if (n < 0 || Hc <= 0 || Wc <= 0 || H <= 0 || W <= 0 || (n > 0 && (!in || !out)))
    return set_err(nullptr, -EINVAL, "%s: bad arguments", who);
  if (y0 < 0 || x0 < 0 || (long)y0 + H > Hc || (long)x0 + W > Wc)
    return set_err(nullptr, -EINVAL, "%s: the %dx%d window at (%d, %d) is not inside the %dx%d canvas",
                   who, H, W, y0, x0, Hc, Wc);
  if (flip < 0 || flip > 1) return set_err(nullptr, -EINVAL, "%s: flip = %d (0 or 1)", who, flip);
  hipError_t e = launch_window_images(in, n, Hc, Wc, y0, x0, H, W, flip, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, who);
}

int seg_prepare_labels(const uint8_t* raw, int n, int src_h, int src_w, int H, int W,
                       const int32_t* lids2cids, int n_lids, int32_t* out, void* stream) {
  if (n < 0 || src_h <= 0 || src_w <= 0 || H <= 0 || W <= 0 || (n > 0 && (!raw || !out)) ||
      !lids2cids || n_lids <= 0 || n_lids > SEG_MAX_LIDS)
    return set_err(nullptr, -EINVAL, "seg_prepare_labels: bad arguments");
  hipError_t e = launch_prepare_labels(raw, n, src_h, src_w, H, W, lid_map(lids2cids, n_lids), out,
                                       (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_prepare_labels");
}

int seg_augment_workspace(int n, int H, int W, int64_t* bytes) {
  if (n < 0 || H <= 0 || W <= 0 || !bytes)
    return set_err(nullptr, -EINVAL, "seg_augment_workspace: bad arguments");
  *bytes = (int64_t)aug_workspace_bytes(n, H, W);
  return 0;
}

int seg_augment_profile(int enable, float* pass_ms) {
  hipError_t e = aug_profile_enable(enable != 0);
  if (e == hipSuccess && pass_ms) e = aug_profile_read(pass_ms);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_augment_profile");
}

int seg_augment_profile_blur(float* blur_ms) {
  if (!blur_ms) return set_err(nullptr, -EINVAL, "seg_augment_profile_blur: bad arguments");
  const hipError_t e = aug_profile_read_blur(blur_ms);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_augment_profile_blur");
}

int seg_augment_images(const uint8_t* raw, int n, int src_h, int src_w, int resized_h,
                       int resized_w, int crop_y, int crop_x, int H, int W,
                       const seg_aug_params* params_host, const seg_aug_params* params_dev,
                       float* out, void* workspace, int64_t ws_bytes, void* stream) {
  if (n < 0 || src_h <= 0 || src_w <= 0 || H <= 0 || W <= 0 || (n > 0 && (!raw || !out)))
    return set_err(nullptr, -EINVAL, "seg_augment_images: bad arguments");
  if (crop_y < 0 || crop_x < 0 || (int64_t)crop_y + H > resized_h || (int64_t)crop_x + W > resized_w)
    return set_err(nullptr, -EINVAL, "seg_augment_images: window %d,%d + %dx%d outside the resized "
                   "%dx%d", crop_y, crop_x, H, W, resized_h, resized_w);
  if (int r = aug_check("seg_augment_images", n, H, W, params_host, params_dev)) return r;
  if (((uintptr_t)out & 15) || ((uintptr_t)workspace & 15))
    return set_err(nullptr, -EINVAL, "seg_augment_images: out / workspace must be 16-byte aligned");
  const int64_t need = (int64_t)aug_workspace_bytes(n, H, W);
  if (n > 0 && (!workspace || ws_bytes < need))
    return set_err(nullptr, -EINVAL, "seg_augment_images: workspace of %lld bytes, %lld needed "
                   "(seg_augment_workspace)", (long long)ws_bytes, (long long)need);
  const AugResize r{src_h, src_w, resized_h, resized_w, crop_y, crop_x};
  hipError_t e = launch_augment_images(raw, n, r, H, W, (const AugParams*)params_host,
                                       (const AugParams*)params_dev, out, workspace,
                                       (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_augment_images");
}

int seg_augment_labels(const uint8_t* raw, int n, int src_h, int src_w, int H, int W,
                       const int32_t* lids2cids, int n_lids, const seg_aug_params* params_host,
                       const seg_aug_params* params_dev, int32_t* out, void* stream) {
  if (n < 0 || src_h <= 0 || src_w <= 0 || H <= 0 || W <= 0 || (n > 0 && (!raw || !out)) ||
      !lids2cids || n_lids <= 0 || n_lids > SEG_MAX_LIDS)
    return set_err(nullptr, -EINVAL, "seg_augment_labels: bad arguments");
  if (int r = aug_check("seg_augment_labels", n, H, W, params_host, params_dev)) return r;
  hipError_t e = launch_augment_labels(raw, n, src_h, src_w, H, W, lid_map(lids2cids, n_lids),
                                       (const AugParams*)params_host, (const AugParams*)params_dev,
                                       out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_augment_labels");
}

int seg_op_conv_fwd(int dtype, const void* x, int N, int H, int W, int C, int ldx, const void* w,
                    int Co, int k, int stride, int rate, int explicit_pad, void* y, int ldy,
                    float* stats, void* stream) {
  int Ho, Wo, ph, pw;
  op_geom(H, W, k, stride, rate, explicit_pad, &Ho, &Wo, &ph, &pw);
  const ConvArgs a = fwd_conv_args(x, N, H, W, C, ldx, w, Co, k, stride, rate, ph, pw, Ho, Wo, y, ldy, stats);
  hipError_t e = launch_conv_nt(dt_of(dtype), 0, a, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_conv_fwd");
}

int seg_op_conv_stat_rows(int dtype, int N, int H, int W, int C, int ldx, int Co, int ldy, int k,
                          int stride, int rate, int explicit_pad) {
  int Ho, Wo, ph, pw;   // the ConvArgs seg_op_conv_fwd builds (the kernel choice is shape-dependent)
  op_geom(H, W, k, stride, rate, explicit_pad, &Ho, &Wo, &ph, &pw);
  const ConvArgs a = fwd_conv_args(nullptr, N, H, W, C, ldx, nullptr, Co, k, stride, rate, ph, pw, Ho, Wo,
                                   nullptr, ldy, nullptr);
  return conv_nt_plan(dt_of(dtype), 0, a).stat_rows;
}

int seg_op_conv_dgrad(int dtype, const void* dy, int N, int Ho, int Wo, int Co, int lddy,
                      const void* wt, int Ci, int k, int stride, int rate, int explicit_pad, int H,
                      int W, void* dx, int lddx, void* stream) {
  int ho, wo, ph, pw;
  op_geom(H, W, k, stride, rate, explicit_pad, &ho, &wo, &ph, &pw);
  if (ho != Ho || wo != Wo) return set_err(nullptr, -EINVAL, "dgrad geometry mismatch");
  const ConvArgs a = dgrad_conv_args(dy, N, Ho, Wo, Co, lddy, wt, Ci, k, stride, rate, ph, pw, H, W, dx, lddx);
  hipError_t e = launch_conv_nt(dt_of(dtype), 0, a, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_conv_dgrad");
}

int seg_op_conv_dgrad_res(int dtype, const void* dy, int N, int H, int W, int Co, int lddy,
                          const void* wt, int Ci, void* dx, int lddx, const void* r, int ldr,
                          const uint8_t* omask, void* stream) {
  if (!r && !omask) return set_err(nullptr, -EINVAL, "dgrad_res: a residual or a mask is required");
  if (omask && Ci % 8) return set_err(nullptr, -EINVAL, "dgrad_res: masked outputs need Ci %% 8 == 0");
  ConvArgs a = dgrad_conv_args(dy, N, H, W, Co, lddy, wt, Ci, 1, 1, 1, 0, 0, H, W, dx, lddx);
  if (r) { a.r = r; a.ldr = ldr; }
  if (omask) { a.omask = omask; a.ldm = Ci / 8; }
  hipError_t e = launch_conv_nt(dt_of(dtype), 0, a, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_conv_dgrad_res");
}

int seg_op_conv_dgrad_fused(int dtype, const void* dy, int N, int H, int W, int Co, int lddy,
                            const void* wt, int Ci, int k, int rate, void* dx, int lddx,
                            const void* r1, int ldr1, const void* r2, int ldr2, const void* dy2,
                            int Co2, int lddy2, const void* wt2, const uint8_t* omask, void* stream) {
  if (!dy || !wt || !dx || N < 1 || H < 1 || W < 1 || Co < 1 || Ci < 1)
    return set_err(nullptr, -EINVAL, "dgrad_fused: bad argument");
  if ((k != 1 && k != 3) || rate < 1 || (k == 1 && rate != 1))
    return set_err(nullptr, -EINVAL, "dgrad_fused: k must be 1 (rate 1) or 3");
  if (r2 && !r1) return set_err(nullptr, -EINVAL, "dgrad_fused: a second residual needs a first");
  if ((dy2 != nullptr) != (wt2 != nullptr))
    return set_err(nullptr, -EINVAL, "dgrad_fused: dy2 and wt2 come together");
  // the combinations the runtime launches: a dual GEMM has no residual (conv_dgrad_dual)
  if (dy2 && (r1 || r2 || k != 1 || !seg_half(dt_of(dtype)) || Co2 < 1))
    return set_err(nullptr, -EINVAL, "dgrad_fused: the dual GEMM is 1 x 1, 16-bit, without residuals");
  int ho, wo, ph, pw;
  op_geom(H, W, k, 1, rate, 0, &ho, &wo, &ph, &pw);   // stride 1, SAME: ho = H, wo = W
  ConvArgs a = dgrad_conv_args(dy, N, H, W, Co, lddy, wt, Ci, k, 1, rate, ph, pw, H, W, dx, lddx);
  if (r1) { a.r = r1; a.ldr = ldr1; }
  if (r2) { a.r2 = r2; a.ldr2 = ldr2; }
  if (dy2) dgrad_dual_args(a, dy2, lddy2, Co2, wt2);
  if (omask) {
    if (Ci % 8) return set_err(nullptr, -EINVAL, "dgrad_fused: masked outputs need Ci %% 8 == 0");
    a.omask = omask; a.ldm = Ci / 8;
  }
  const ConvNtPlan p = conv_nt_plan(dt_of(dtype), 0, a);
  if (omask && !p.omask) return set_err(nullptr, -EINVAL, "dgrad_fused: no masked launch for this shape");
  if (dy2 && p.kernel == NT_INVALID) return set_err(nullptr, -EINVAL, "dgrad_fused: %s", p.reason);
  hipError_t e = launch_conv_nt(dt_of(dtype), 0, a, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_conv_dgrad_fused");
}

int seg_op_conv_wgrad(int dtype, const void* dy, int N, int Ho, int Wo, int Co, int lddy,
                      const void* x, int H, int W, int Ci, int ldx, int k, int stride, int rate,
                      int explicit_pad, float* dw, void* workspace, int64_t ws_bytes, void* stream) {
  int ho, wo, ph, pw;
  op_geom(H, W, k, stride, rate, explicit_pad, &ho, &wo, &ph, &pw);
  if (ho != Ho || wo != Wo) return set_err(nullptr, -EINVAL, "wgrad geometry mismatch");
  WgradArgs a = wgrad_conv_args(dy, lddy, x, N, H, W, Ci, ldx, Ho, Wo, Co, k, stride, rate, ph, pw);
  a.splits = wgrad_splits(a, dt_of(dtype));
  const long n = (long)Co * k * k * Ci;
  if ((int64_t)a.splits * n * 4 > ws_bytes) a.splits = (int)std::max<int64_t>(1, ws_bytes / (n * 4));
  a.out = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = launch_conv_wgrad(dt_of(dtype), a, s);
  if (e == hipSuccess) e = launch_splitk_reduce((float*)workspace, a.splits, n, n, dw, 0, s);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_conv_wgrad");
}

int seg_op_conv_wgrad_cfg(int dtype, const void* dy, int N, int Ho, int Wo, int Co, int lddy,
                          const void* x, int H, int W, int Ci, int ldx, int k, int stride, int rate,
                          int explicit_pad, float* dw, void* workspace, int64_t ws_bytes, int bm,
                          int bn, int splits, void* stream) {
  if (dtype != SEG_DTYPE_BF16 && dtype != SEG_DTYPE_F16)
    return set_err(nullptr, -EINVAL, "wgrad_cfg: 16-bit dtypes only");
  if ((bm != 64 && bm != 128 && bm != 256) || (bn != 64 && bn != 128 && bn != 256) || splits < 1)
    return set_err(nullptr, -EINVAL, "wgrad_cfg: tile must be 64/128/256, splits >= 1");
  int ho, wo, ph, pw;
  op_geom(H, W, k, stride, rate, explicit_pad, &ho, &wo, &ph, &pw);
  if (ho != Ho || wo != Wo) return set_err(nullptr, -EINVAL, "wgrad geometry mismatch");
  WgradArgs a = wgrad_conv_args(dy, lddy, x, N, H, W, Ci, ldx, Ho, Wo, Co, k, stride, rate, ph, pw);
  a.splits = splits;
  const long n = (long)Co * k * k * Ci;
  if ((int64_t)splits * n * 4 > ws_bytes) return set_err(nullptr, -EINVAL, "wgrad_cfg: workspace");
  if (conv_wgrad_plan(dt_of(dtype), a, bm, bn).kernel == WG_INVALID)
    return set_err(nullptr, -EINVAL, "wgrad_cfg: shape not on the v2 path");
  a.out = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = launch_conv_wgrad(dt_of(dtype), a, s, bm, bn);
  if (e == hipSuccess) e = launch_splitk_reduce((float*)workspace, splits, n, n, dw, 0, s);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_conv_wgrad_cfg");
}

int seg_op_bn_rowblocks(int64_t M, int C) {
  if (M < 1 || C < 1) return set_err(nullptr, -EINVAL, "seg_op_bn_rowblocks: bad arguments");
  return bn_bwd_rowblocks((long)M);
}

int seg_op_bn_stats_finalize(const float* part, int64_t M, int C, int tile_rows, const float* gamma,
                             float* mean, float* invstd, float* scale, float* var_unb, float* pack,
                             void* stream) {
  if (!part || !gamma || !mean || !invstd || !scale || !var_unb || M < 1 || C < 1 || tile_rows < 1)
    return set_err(nullptr, -EINVAL, "seg_op_bn_stats_finalize: bad arguments");
  BnState st{};
  st.mean = mean; st.invstd = invstd; st.scale = scale; st.var_unb = var_unb;
  hipError_t e = launch_bn_stats_finalize(part, (long)M, C, tile_rows, gamma, st,
                                          (hipStream_t)stream, pack);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_bn_stats_finalize");
}

int seg_op_bn_apply(int dtype, int out_f32, const seg_bn_apply_args* p, void* stream) {
  if (!p || bad_dtype(dtype) || !p->y || !p->out || !p->mean || !p->scale || !p->beta || p->M < 1 ||
      p->C < 1 || p->ldy < p->C || p->ldo < p->C)
    return set_err(nullptr, -EINVAL, "seg_op_bn_apply: bad arguments");
  if (dtype == SEG_DTYPE_F32 && !out_f32)
    return set_err(nullptr, -EINVAL, "seg_op_bn_apply: a 32-bit input has a 32-bit output");
  if (p->y2 && (p->res || !p->mean2 || !p->scale2 || !p->beta2 || p->ldy2 < p->C))
    return set_err(nullptr, -EINVAL, "seg_op_bn_apply: the second BN takes the place of the residual "
                   "and needs its own mean2 / scale2 / beta2");
  if (p->res && (p->ldres < p->C || p->rs < 1 ||
                 (p->rs > 1 && (p->Ho < 1 || p->Wo < 1 || p->M % ((int64_t)p->Ho * p->Wo) ||
                                (p->Ho - 1) * p->rs >= p->Hr || (p->Wo - 1) * p->rs >= p->Wr))))
    return set_err(nullptr, -EINVAL, "seg_op_bn_apply: the subsampled residual grid does not cover "
                   "the output grid");
  BnApplyArgs a{};
  a.y = p->y; a.ldy = p->ldy; a.M = (long)p->M; a.C = p->C;
  a.mean = p->mean; a.scale = p->scale; a.beta = p->beta; a.relu = p->relu;
  a.res = p->res; a.ldres = p->ldres; a.rs = p->rs;
  a.Ho = p->Ho; a.Wo = p->Wo; a.Hr = p->Hr; a.Wr = p->Wr;
  a.y2 = p->y2; a.ldy2 = p->ldy2; a.mean2 = p->mean2; a.scale2 = p->scale2; a.beta2 = p->beta2;
  a.out = p->out; a.ldo = p->ldo; a.mask = p->mask;
  if (a.mask && (!a.relu || !bn_apply_plan(a).wide))
    return set_err(nullptr, -EINVAL, "seg_op_bn_apply: ReLU bits exist on the 8-wide path only, "
                   "with relu");
  hipError_t e = launch_bn_apply(dt_of(dtype), out_f32, a, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, "seg_op_bn_apply");
}

int seg_op_bn_backward(int dtype, int dz_f32, int frozen, int reduce_only, const seg_bn_bwd_args* p,
                       void* stream) {
  const char* who = "seg_op_bn_backward";
  if (int r = bn_bwd_check(who, dtype, p, !reduce_only)) return r;
  if (dtype == SEG_DTYPE_F32) dz_f32 = 0;   // dz is of the storage type
  if (p->z && p->mask) return set_err(nullptr, -EINVAL, "%s: the gate is z or the bits, not both", who);
  if (p->z && p->ldz < p->C) return set_err(nullptr, -EINVAL, "%s: bad arguments", who);
  if (p->dyhat && p->lddyhat < p->C) return set_err(nullptr, -EINVAL, "%s: bad arguments", who);
  BnBwdArgs a = bn_bwd_op_args(p);
  a.reduce_dyhat = reduce_only && p->dyhat ? 1 : 0;
  const char* why = bn_bwd_reduce_plan(dt_of(dtype), a).refusal;
  if (!why && !reduce_only) why = bn_bwd_apply_plan(a).refusal;
  if (why) return set_err(nullptr, -EINVAL, "%s: %s", who, why);
  hipStream_t s = (hipStream_t)stream;
  BnState st{};
  st.sdy = p->sdy; st.sdyx = p->sdyx;
  hipError_t e = launch_bn_bwd_reduce(dt_of(dtype), dz_f32, a, s);
  if (e == hipSuccess) e = launch_bn_bwd_finalize(a.part, a.rb, a.M, a.C, st, p->dgamma, p->dbeta, s, frozen);
  if (e == hipSuccess && !reduce_only) e = launch_bn_bwd_apply(dt_of(dtype), dz_f32, a, s);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, who);
}

int seg_op_bn_backward_dual(int dtype, int frozen, int second_only, const seg_bn_bwd_args* p,
                            const seg_bn_bwd_args* q, void* stream) {
  const char* who = "seg_op_bn_backward_dual";
  if (int r = bn_bwd_check(who, dtype, p, !second_only)) return r;
  if (int r = bn_bwd_check(who, dtype, q, true)) return r;
  if (q->M != p->M || q->C != p->C || !p->mask || q->part == p->part || p->dshift || p->cs_part)
    return set_err(nullptr, -EINVAL, "%s: two layers of one shape with partials of their own, gated "
                   "by the first's bits", who);
  BnBwdArgs a = bn_bwd_op_args(p);
  seg_bn_bwd_args alone = *q;   // the second layer alone: ungated, dz of the storage type
  alone.dz = p->dz; alone.lddz = p->lddz;
  alone.z = nullptr; alone.mask = nullptr; alone.dyhat = nullptr;
  alone.dzscale = nullptr; alone.dshift = nullptr; alone.cs_part = nullptr;
  const BnBwdArgs a2 = bn_bwd_op_args(&alone);
  a.y2 = a2.y; a.ldy2 = a2.ldy;
  a.mean2 = a2.mean; a.invstd2 = a2.invstd; a.scale2 = a2.scale;
  a.sdy2 = a2.sdy; a.sdyx2 = a2.sdyx;
  a.dy2 = a2.dy; a.lddy2 = a2.lddy;
  a.part2 = a2.part;
  hipStream_t s = (hipStream_t)stream;
  BnState st{}, st2{};
  st.sdy = p->sdy; st.sdyx = p->sdyx;
  st2.sdy = q->sdy; st2.sdyx = q->sdyx;
  if (const char* why = bn_bwd_dual_plan(a).refusal) return set_err(nullptr, -EINVAL, "%s: %s", who, why);
  hipError_t e = launch_bn_bwd_reduce_dual(dt_of(dtype), a, s);
  if (e == hipSuccess) e = launch_bn_bwd_finalize(a.part, a.rb, a.M, a.C, st, p->dgamma, p->dbeta, s, frozen);
  if (e == hipSuccess) e = launch_bn_bwd_finalize(a2.part, a2.rb, a.M, a.C, st2, q->dgamma, q->dbeta, s, frozen);
  if (e == hipSuccess)
    e = second_only ? launch_bn_bwd_apply(dt_of(dtype), 0, a2, s) : launch_bn_bwd_apply_dual(dt_of(dtype), a, s);
  return e == hipSuccess ? 0 : hip_fail(nullptr, e, who);
}

uint32_t seg_crc32c(uint32_t crc, const void* data, size_t n) {
  const uint32_t(*t)[256] = crc_tables().t;
  const uint8_t* p = (const uint8_t*)data;
  uint32_t c = ~crc;
  while (n >= 8) {   // slicing-by-8
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = t[7][lo & 0xFF] ^ t[6][(lo >> 8) & 0xFF] ^ t[5][(lo >> 16) & 0xFF] ^ t[4][lo >> 24] ^
        t[3][hi & 0xFF] ^ t[2][(hi >> 8) & 0xFF] ^ t[1][(hi >> 16) & 0xFF] ^ t[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n--) c = t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
  return ~c;
}

}  // extern "C"
