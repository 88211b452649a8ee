"""Generates tests/golden/conv_plan_parent.json: the answers of the conv dispatch predicates
as they stood before the kernel selection moved into csrc/conv_select.cpp, for every request of
tests/conv_plan_cases.py in fp32, bf16 and fp16.

    python tests/golden/make_conv_plan_fixture.py <libseg_hip.so built from the parent commit>

The parent library exports its C++ predicates (conv_nt_uses_v2, conv_nt_v2_ok, conv_nt_pp_ok,
conv_nt_omask_ok, conv_nt_v2_dual_ok, conv_skinny_ok, conv_nt_stat_rows; conv_wgrad_patch_ok,
conv_wgrad_v2_ok, conv_wgrad_pp_ok, conv_wgrad_v2_tile) and seg_op_conv_stat_rows; a few lines of
C++ linked against it ask them. ConvArgs / WgradArgs are laid out as in csrc/conv_args.h (moved
there unchanged). The fixture holds the recorded answers only; tests/test_conv_plan.py rebuilds
the requests and checks their digest."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import conv_plan_cases as cases  # noqa: E402

SHIM = r"""
#include <cstdio>
#include "conv_args.h"
bool conv_nt_uses_v2(int dtype, int out_f32, const ConvArgs& a);
bool conv_nt_v2_ok(const ConvArgs& a);
bool conv_nt_pp_ok(const ConvArgs& a);
bool conv_nt_omask_ok(int dtype, const ConvArgs& a);
bool conv_nt_v2_dual_ok(const ConvArgs& a);
bool conv_skinny_ok(int dtype, int out_f32, const ConvArgs& a);
int conv_nt_stat_rows(int dtype, int out_f32, const ConvArgs& a);
bool conv_wgrad_patch_ok(const WgradArgs& a);
bool conv_wgrad_v2_ok(const WgradArgs& a);
bool conv_wgrad_pp_ok(const WgradArgs& a);
void conv_wgrad_v2_tile(int Co, int Ncol, long P, int* bm, int* bn);
extern "C" int seg_op_conv_stat_rows(int dtype, int N, int H, int W, int C, int ldx, int Co, int ldy,
                                     int k, int stride, int rate, int explicit_pad);
static char ONE;
int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'n') {
      int dt, of, fl, f[24];
      scanf("%d %d %d", &dt, &of, &fl);
      for (int i = 0; i < 24; ++i) scanf("%d", &f[i]);
      ConvArgs a{};
      a.N = f[0]; a.H = f[1]; a.W = f[2]; a.C = f[3]; a.ldx = f[4]; a.ldw = f[5];
      a.Ho = f[6]; a.Wo = f[7]; a.Co = f[8]; a.ldy = f[9]; a.ldr = f[10]; a.ldr2 = f[11];
      a.KH = f[12]; a.KW = f[13]; a.sf = f[14]; a.st = f[15]; a.pad_h = f[16]; a.pad_w = f[17];
      a.dil = f[18]; a.tap8 = f[19]; a.ldx2 = f[20]; a.C2 = f[21]; a.ldw2 = f[22]; a.ldm = f[23];
      if (fl & 1) a.r = &ONE;
      if (fl & 2) a.r2 = &ONE;
      if (fl & 4) a.stats = (float*)&ONE;
      if (fl & 8) a.omask = (const uint8_t*)&ONE;
      if (fl & 16) { a.x2 = &ONE; a.w2 = &ONE; }
      printf("%d %d %d %d %d %d %d\n", (int)conv_nt_uses_v2(dt, of, a), (int)conv_nt_v2_ok(a),
             (int)conv_nt_pp_ok(a), (int)conv_nt_omask_ok(dt, a), (int)conv_nt_v2_dual_ok(a),
             (int)conv_skinny_ok(dt, of, a), conv_nt_stat_rows(dt, of, a));
    } else if (kind == 'w') {
      int fl, f[18];
      scanf("%d", &fl);
      for (int i = 0; i < 18; ++i) scanf("%d", &f[i]);
      WgradArgs a{};
      a.lddy = f[0]; a.N = f[1]; a.H = f[2]; a.W = f[3]; a.C = f[4]; a.ldx = f[5];
      a.Ho = f[6]; a.Wo = f[7]; a.Co = f[8]; a.KH = f[9]; a.KW = f[10]; a.sf = f[11];
      a.pad_h = f[12]; a.pad_w = f[13]; a.dil = f[14]; a.splits = f[15]; a.lddy2 = f[16]; a.Co1 = f[17];
      if (fl & 1) a.dy2 = &ONE;
      int bm, bn;
      conv_wgrad_v2_tile(a.Co, a.KH * a.KW * a.C, (long)a.N * a.Ho * a.Wo, &bm, &bn);
      printf("%d %d %d %d %d\n", (int)conv_wgrad_patch_ok(a), (int)conv_wgrad_v2_ok(a),
             (int)conv_wgrad_pp_ok(a), bm, bn);
    } else {   // 's': seg_op_conv_stat_rows through the C ABI
      int v[12];
      for (int i = 0; i < 12; ++i) scanf("%d", &v[i]);
      printf("%d\n", seg_op_conv_stat_rows(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9],
                                           v[10], v[11]));
    }
  }
  return 0;
}
"""


def requests():
    """the shim's input lines, in fixture order"""
    nt, wg, abi = [], [], []
    for dt in (0, 1, 2):
        for _, of, f, fl in cases.nt_requests():
            nt.append("n %d %d %d %s" % (dt, of, fl, " ".join(map(str, f))))
        for _, f, fl in cases.wg_requests():
            wg.append("w %d %s" % (fl, " ".join(map(str, f))))   # the predicates take no dtype
        for _, (N, H, W, Ci, Co, k, s, r, ep) in cases.shapes():
            abi.append("s %d %d %d %d %d %d %d %d %d %d %d %d" % (dt, N, H, W, Ci, cases.pad8(Ci), Co,
                                                                   cases.co_pad(Co), k, s, r, ep))
    return nt, wg[:len(wg) // 3], abi


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main(lib):
    lib = os.path.abspath(lib)
    nt, wg, abi = requests()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ask.cpp"), os.path.join(tmp, "ask")
        open(src, "w").write(SHIM)
        csrc = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd", "csrc")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wno-unused-result", "-I", csrc, src, "-o", exe, lib,
                        "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"], check=True)
        out = subprocess.run([exe], input="\n".join(nt + wg + abi) + "\n", capture_output=True,
                             text=True, check=True).stdout.split("\n")
    rows = [[int(v) for v in line.split()] for line in out if line]
    assert len(rows) == len(nt) + len(wg) + len(abi)
    fixture = {
        "nt_columns": ["uses_v2", "v2_ok", "pp_ok", "omask_ok", "v2_dual_ok", "skinny_ok", "stat_rows"],
        "wg_columns": ["patch_ok", "v2_ok", "pp_ok", "tile_bm", "tile_bn"],
        "requests_sha256": digest(nt + wg + abi),
        "nt": rows[:len(nt)],
        "wg": rows[len(nt):len(nt) + len(wg)],
        "abi_stat_rows": [r[0] for r in rows[len(nt) + len(wg):]],
    }
    path = os.path.join(HERE, "conv_plan_parent.json")
    with open(path, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
    print(path, len(nt), "conv,", len(wg), "wgrad,", len(abi), "C-ABI rows")


if __name__ == "__main__":
    main(sys.argv[1])
