// Batch normalisation (TF 1.12 fused training semantics) as HBM-streaming kernels.
//   forward : per-channel (mean, biased var) from the conv epilogue's tile partials
//             (Chan merge, fixed order), out = act((y-mean)*gamma*rsqrt(var+eps) + beta [+res])
//   backward: dyhat = dz * [z>0]; dgamma = sum dyhat*xhat; dbeta = sum dyhat;
//             dy = gamma*invstd*(dyhat - mean(dyhat) - xhat*mean(dyhat*xhat))
#pragma once
#include "seg_common.h"

#define SEG_BN_EPS 1.001e-5f  // tf.nn.fused_batch_norm clamps 1e-5 up to this

struct BnState {     // per-layer per-step device vectors, each [C]
  float* mean;
  float* invstd;
  float* scale;      // gamma * invstd
  float* var_unb;    // Bessel-corrected batch variance (moving-average input)
  float* sdy;        // backward: mean(dyhat)
  float* sdyx;       // backward: mean(dyhat * xhat)
};

struct BnApplyArgs {
  const void* y; int ldy;          // conv output (T)
  long M; int C;
  const float* mean; const float* scale; const float* beta;
  int relu;
  // residual 1: plain tensor (T) with optional spatial subsampling (stride rs over an
  // [N][Hr][Wr] grid; the output grid is [N][Ho][Wo])
  const void* res; int ldres; int rs; int Ho, Wo, Hr, Wr;
  // residual 2: second BN (shortcut conv): (y2-mean2)*scale2+beta2
  const void* y2; int ldy2; const float* mean2; const float* scale2; const float* beta2;
  void* out; int ldo;              // output (T or f32)
  uint8_t* mask;                   // optional ReLU bits of out: [M][C/8], bit e = out[c0+e] > 0
};

struct BnBwdArgs {
  const void* dz; int lddz;        // incoming gradient (T or f32)
  const void* z; int ldz;          // activation whose >0 mask gates dz (nullable)
  const uint8_t* mask;             // the same gate as bits [M][C/8] (preferred over z when set)
  const void* y; int ldy;          // conv output (T)
  long M; int C;
  const float* mean; const float* invstd; const float* scale;
  const float* sdy; const float* sdyx;   // apply: means from finalize
  void* dy; int lddy;              // output gradient wrt y (T)
  void* dyhat; int lddyhat;        // optional masked gradient (T)
  const float* dzscale;            // optional per-channel factor applied to dz
  // optional per-channel term added to dz before the gate (8-wide masked path only): the
  // constant part of a data gradient whose producer left it out (net_layers.cpp, linear BN-backward
  // fold of the consumer's expansion conv)
  const float* dshift;
  int reduce_dyhat;                // the reduce (not the apply) stores the gated gradient in dyhat
  // optional (8-wide masked reduce with dshift): per row block column sums of the forward
  // output relu((y - mean) * scale + beta) rounded to T as the forward BN apply stored it,
  // recomputed from y, [rb][C] (the linear BN-backward fold's colsum of the next conv's input)
  const float* beta;
  float* cs_part;
  float* part;                     // reduce partials [rb][C][2]
  int rb;                          // number of row blocks
  // dual (launch_bn_bwd_*_dual): a second BN layer gated by the same dz and bits, e.g. a
  // projection unit's conv3 and shortcut BN; dz and the bits are read once for both
  const void* y2; int ldy2;
  const float* mean2; const float* invstd2; const float* scale2;
  const float* sdy2; const float* sdyx2;
  void* dy2; int lddy2;
  float* part2;
};

// ---- kernel selection: what a launch's arguments choose, asked by the launchers and their callers
// The 8-channel streaming kernels' layout rule: C and every row stride in use (or-ed into lds)
// a multiple of 8, p16 (the first 16-byte access) aligned. Otherwise the scalar kernels run.
inline bool bn_wide(int C, int lds, const void* p16) {
  return ((C | lds) & 7) == 0 && (uintptr_t)p16 % 16 == 0;
}

enum { RES_NONE = 0, RES_PLAIN = 1, RES_SUB = 2, RES_BN2 = 3 };
struct BnApplyPlan {
  bool wide;   // the 8-channel kernels (the only ones that write ReLU bits)
  int res;     // RES_*
  bool relu;
};
inline BnApplyPlan bn_apply_plan(const BnApplyArgs& a) {
  BnApplyPlan p;
  p.wide = bn_wide(a.C, a.ldy | a.ldo | (a.res ? a.ldres : 0) | (a.y2 ? a.ldy2 : 0), a.out);
  p.res = a.y2 ? RES_BN2 : (a.res ? (a.rs > 1 ? RES_SUB : RES_PLAIN) : RES_NONE);
  p.relu = a.relu != 0;
  return p;
}

// The backward's variants (the table: DESIGN.md, batch norm). The values are the 8-wide kernels'
// HZ and HS template arguments.
enum { BN_GATE_NONE = 0, BN_GATE_Z = 1, BN_GATE_BITS = 2 };
enum { BN_TERM_NONE = 0, BN_TERM_DZSCALE = 1, BN_TERM_DSHIFT = 2 };
struct BnBwdPlan {
  bool wide;
  int gate;              // BN_GATE_*: the bits win over z
  int term;              // BN_TERM_*: the per-channel term of dz
  bool dyhat;            // this launch stores the gated gradient
  bool colsum;           // the reduce also forms cs_part
  const char* refusal;   // nullptr: launch; else why the launcher returns hipErrorInvalidValue
};
inline BnBwdPlan bn_bwd_plan_base(const BnBwdArgs& a) {
  BnBwdPlan p{};
  p.wide = bn_wide(a.C, a.lddz | a.ldy | (a.z ? a.ldz : 0) | (a.dy ? a.lddy : 0) | (a.dyhat ? a.lddyhat : 0), a.dz);
  p.gate = a.mask ? BN_GATE_BITS : (a.z ? BN_GATE_Z : BN_GATE_NONE);
  if (a.mask && !p.wide) p.refusal = "ReLU bits exist on the 8-wide path only";
  return p;
}
inline BnBwdPlan bn_bwd_reduce_plan(int dtype, const BnBwdArgs& a) {
  BnBwdPlan p = bn_bwd_plan_base(a);
  p.dyhat = a.reduce_dyhat && a.dyhat;   // reduce_dyhat moves the store out of the apply
  p.colsum = a.cs_part != nullptr;
  // with the bits the reduce drops dzscale (group norm's gamma: the apply alone carries it)
  p.term = a.dshift ? BN_TERM_DSHIFT : (a.dzscale && !a.mask ? BN_TERM_DZSCALE : BN_TERM_NONE);
  if (p.refusal) return p;
  if ((a.dshift || p.dyhat) && (!a.mask || a.dzscale || !p.wide))
    p.refusal = "dshift / a reduce-side dyhat need the ReLU bits, the 8-wide path and no dzscale";
  else if (p.colsum && (!a.dshift || p.dyhat || !a.beta || !seg_half(dtype)))
    p.refusal = "cs_part needs dshift, beta, a 16-bit type and no reduce-side dyhat";
  return p;
}
inline BnBwdPlan bn_bwd_apply_plan(const BnBwdArgs& a) {
  BnBwdPlan p = bn_bwd_plan_base(a);
  p.dyhat = a.dyhat != nullptr;
  p.term = a.dshift ? BN_TERM_DSHIFT : (a.dzscale ? BN_TERM_DZSCALE : BN_TERM_NONE);
  if (!p.refusal && a.dshift && (!a.mask || a.dzscale || a.dyhat || !p.wide))
    p.refusal = "dshift in the apply needs the ReLU bits, the 8-wide path, no dzscale and no dyhat";
  return p;
}
// the dual launches (reduce and apply alike): two layers of 8-wide layouts gated by the bits
inline BnBwdPlan bn_bwd_dual_plan(const BnBwdArgs& a) {
  BnBwdPlan p{};
  p.wide = bn_wide(a.C, a.lddz | a.ldy | a.ldy2 | a.lddy | a.lddy2, a.dz);
  p.gate = BN_GATE_BITS;
  if (!a.mask || a.z || a.dzscale || a.dyhat || !p.wide)
    p.refusal = "the dual kernels take 8-wide layouts, the bits, and no z / dzscale / dyhat";
  return p;
}

// pack (nullable, [2C]): also writes [mean | E[x^2]] for a cross-replica exchange
hipError_t launch_bn_stats_finalize(const float* tile_part, long M, int C, int tile_rows,
                                    const float* gamma, BnState st, hipStream_t s,
                                    float* pack = nullptr);
// cross-replica BN: the replica-summed pack -> global mean / biased variance in st
hipError_t launch_bn_sync_unpack(const float* pack, int C, float inv_world, const float* gamma,
                                 BnState st, hipStream_t s);
// inference mode (st from the moving statistics), every layer in one launch (one workgroup per job)
struct BnInferJob { const float* mov_mean; const float* mov_var; const float* gamma; BnState st; int C; };
hipError_t launch_bn_infer_finalize_all(const BnInferJob* jobs, int n, hipStream_t s);
hipError_t launch_bn_apply(int dtype, int out_f32, const BnApplyArgs& a, hipStream_t s);
int bn_bwd_rowblocks(long M);
// the backward launchers map their plan to a kernel: hipErrorInvalidValue, nothing launched,
// where the plan refuses
hipError_t launch_bn_bwd_reduce(int dtype, int dz_f32, const BnBwdArgs& a, hipStream_t s);
// frozen: is_training=False statistics (moving averages): the batch means do not depend on
// the input, so sdy = sdyx = 0 and dy = gamma * invstd * dyhat (FusedBatchNormGrad, inference)
hipError_t launch_bn_bwd_finalize(const float* part, int rb, long M, int C, BnState st,
                                  float* dgamma, float* dbeta, hipStream_t s, int frozen = 0);
hipError_t launch_bn_bwd_apply(int dtype, int dz_f32, const BnBwdArgs& a, hipStream_t s);
// dual forms (16-bit or fp32 dz of the storage type, ReLU bits, no dzscale / dyhat)
hipError_t launch_bn_bwd_reduce_dual(int dtype, const BnBwdArgs& a, hipStream_t s);
hipError_t launch_bn_bwd_apply_dual(int dtype, const BnBwdArgs& a, hipStream_t s);
hipError_t launch_moving_update(float* mov_mean, float* mov_var, const float* bmean,
                                const float* bvar, int n, float decay, hipStream_t s);
