// seg_op_conv_plan / seg_op_conv_wgrad_plan (include/seg_hip.h): the kernel selection of a
// request as one line of key=value words, for tests and tools. No HIP call; plain host C++
// like conv_select.cpp. Formatting lives here only, never on the launch path.
#include <errno.h>
#include <stdio.h>

#include "conv_select.h"

namespace {
const char* const NT_NAMES[] = {"invalid", "mfma", "v2", "v2_dual", "patch", "patch_s2d", "pp",
                                "skinny_n", "skinny_k"};
const char* const WG_NAMES[] = {"invalid", "mfma", "v2", "pp", "patch"};
char ONE;   // any non-null, 16-byte-neutral address stands for "pointer present"
}  // namespace

extern "C" {

int seg_op_conv_plan(int dtype, int out_f32, const int* f, int nf, int flags, char* buf, int len) {
  if (!f || nf != 24 || !buf || len <= 0) return -EINVAL;
  ConvArgs a{};
  a.N = f[0]; a.H = f[1]; a.W = f[2]; a.C = f[3]; a.ldx = f[4]; a.ldw = f[5];
  a.Ho = f[6]; a.Wo = f[7]; a.Co = f[8]; a.ldy = f[9]; a.ldr = f[10]; a.ldr2 = f[11];
  a.KH = f[12]; a.KW = f[13]; a.sf = f[14]; a.st = f[15]; a.pad_h = f[16]; a.pad_w = f[17];
  a.dil = f[18]; a.tap8 = f[19]; a.ldx2 = f[20]; a.C2 = f[21]; a.ldw2 = f[22]; a.ldm = f[23];
  if (flags & 1) a.r = &ONE;
  if (flags & 2) a.r2 = &ONE;
  if (flags & 4) a.stats = (float*)&ONE;
  if (flags & 8) a.omask = (const uint8_t*)&ONE;
  if (flags & 16) { a.x2 = &ONE; a.w2 = &ONE; }
  // a.w stays null: a 16-byte aligned weight pointer (every allocation of the library is)
  const ConvNtPlan p = conv_nt_plan(dtype, out_f32, a);
  int n;
  if (p.kernel == NT_INVALID)
    n = snprintf(buf, len, "kernel=invalid reason=%s", p.reason);   // the reason runs to the end
  else
    n = snprintf(buf, len,
                 "kernel=%s tile=%dx%d st=%d persist=%d tap8=%d small=%d generic=%d out_f32=%d "
                 "stat_rows=%d omask=%d wgs=%ld lds=%d",
                 NT_NAMES[p.kernel], p.bm, p.bn, p.st, p.persist, p.tap8, p.small, p.generic,
                 p.out_f32, p.stat_rows, p.omask, p.wgs, p.lds);
  return n >= len ? -ENOSPC : 0;
}

int seg_op_conv_wgrad_plan(int dtype, const int* f, int nf, int flags, int force_bm, int force_bn,
                           char* buf, int len) {
  if (!f || nf != 18 || !buf || len <= 0) return -EINVAL;
  WgradArgs a{};
  a.lddy = f[0]; a.N = f[1]; a.H = f[2]; a.W = f[3]; a.C = f[4]; a.ldx = f[5];
  a.Ho = f[6]; a.Wo = f[7]; a.Co = f[8]; a.KH = f[9]; a.KW = f[10]; a.sf = f[11];
  a.pad_h = f[12]; a.pad_w = f[13]; a.dil = f[14]; a.splits = f[15]; a.lddy2 = f[16]; a.Co1 = f[17];
  if (flags & 1) a.dy2 = &ONE;
  const ConvWgradPlan p = conv_wgrad_plan(dtype, a, force_bm, force_bn);
  int n;
  if (p.kernel == WG_INVALID)
    n = snprintf(buf, len, "kernel=invalid split_tiles=%ld reason=%s", p.split_tiles, p.reason);
  else
    n = snprintf(buf, len, "kernel=%s tile=%dx%d generic=%d fast=%d tiles=%ld split_tiles=%ld lds=%d",
                 WG_NAMES[p.kernel], p.bm, p.bn, p.generic, p.fast, p.tiles, p.split_tiles, p.lds);
  return n >= len ? -ENOSPC : 0;
}

}  // extern "C"
