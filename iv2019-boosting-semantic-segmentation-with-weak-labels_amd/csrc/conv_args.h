// The plain-data argument blocks of the convolution launches (conv.h describes the three
// problems). No ROCm header: the kernel selection (conv_select.h) compiles with a host compiler.
#pragma once
#include <stdint.h>

struct ConvArgs {
  const void* x;  // A source, NHWC [N][H][W][ldx]
  int N, H, W, C, ldx;
  const void* w;  // B, [Co][K] with row stride ldw (K = KH*KW*C)
  int ldw;
  void* y;        // output NHWC [N][Ho][Wo][ldy]
  int Ho, Wo, Co, ldy;
  const void* r;  // optional residual added in the epilogue (may alias y), ld = ldr
  int ldr;
  const void* r2; // optional second residual, ld = ldr2
  int ldr2;
  int KH, KW;
  int sf;         // forward stride: src = o*sf - pad + k*dil
  int st;         // transposed stride: src valid iff divisible by st (1 = plain conv)
  int pad_h, pad_w, dil;
  float* stats;   // BN partials [mtiles][Co] x {sum, M2} (nullptr = none)
  int tap8;       // tap mode: a tap is tap8 16-B chunks of K (2: the space-to-depth stem, 16
                  // channels per tap); K = KH*KW*C is padded to a multiple of 64 with zero weights
  // K-concatenated second GEMM (dense 1x1: the ping-pong path, and v2 for Co <= 128): y = x w^T + x2 w2^T, x2 [..][ldx2]
  // with C2 channels on the same pixels, w2 [Co][ldw2]; a projection unit's conv1 + shortcut
  // data gradients into the unit input in one accumulation (x2 = nullptr: single GEMM)
  const void* x2;
  int ldx2, C2;
  const void* w2;
  int ldw2;
  // optional ReLU bits of the output's consumer, [M][ldm] bytes (bit e of byte n/8 = channel n):
  // outputs whose bit is 0 are stored as zero (launches whose plan has omask set, conv_select.h)
  const uint8_t* omask;
  int ldm;
};

struct WgradArgs {
  const void* dy;  // [P][lddy], P = N*Ho*Wo
  int lddy;
  const void* x;   // NHWC [N][H][W][ldx]
  int N, H, W, C, ldx;
  int Ho, Wo, Co;
  int KH, KW, sf, pad_h, pad_w, dil;
  float* out;      // fp32 [splits][Co][KH*KW*C]
  int splits;
  // optional second dy source (16-bit v2 / ping-pong kernels): rows co >= Co1 of the output
  // take dy2 [P][lddy2] column co - Co1 (Co1 % 8 == 0; the ping-pong kernel Co1 % 256 == 0):
  // two weight-gradient GEMMs over the same x in one launch (csrc/lbf.h: dyhat^T y2, y2^T y2)
  const void* dy2;
  int lddy2, Co1;
};
