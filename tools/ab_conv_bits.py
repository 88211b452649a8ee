"""Per-launch bit comparison of the conv kernels of two libraries (sibling of ab_grads.py): the
forward (with BN partial statistics), data-gradient and weight-gradient launches of
tests/test_gpu_conv.py's CASES, RES_CASES, LD_CASES, WGRAD_PATCH_CASES and WGRAD_CFG_CASES, in
bf16 and fp16 on seeded inputs, from the working-tree library and from an A/B build
(SEG_HIP_LIB), each in its own child process, one after the other; seg_crc32c of every output and
statistics buffer must be equal.
    python tools/ab_conv_bits.py ab/<variant>/libseg_hip.so"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")


def child(out):
    sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests")]
    import numpy as np
    import torch
    import test_gpu_conv as T
    from seg_hip import LIB

    cuda = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=cuda)
    rows = []

    def crc(t):
        torch.cuda.synchronize()
        b = t.contiguous().view(torch.uint8).cpu().numpy().tobytes()
        return LIB.seg_crc32c(0, b, len(b))

    def rec(label, rc, *bufs):
        rows.append([label, rc] + ([crc(b) for b in bufs] if rc == 0 else []))

    def dev(a, tdt, ld=None):
        """host [..][C] -> device rows of ld >= C elements (the tail zero)"""
        a = np.asarray(a, np.float32)
        if ld is not None and ld != a.shape[-1]:
            p = np.zeros(a.shape[:-1] + (ld,), np.float32)
            p[..., :a.shape[-1]] = a
            a = p
        return torch.as_tensor(a).to(cuda, tdt).contiguous()

    def conv_case(tag, case, dtype, pad):
        """fwd + stats, dgrad, wgrad of one (N, H, W, Ci, Co, k, stride, rate, explicit_pad)"""
        N, H, W, Ci, Co, k, s, r, ep = case
        tdt, abi = T.TDT[dtype], T.ABI[dtype]
        x, w = T._tensors(case)
        _, Ho, Wo = T._geom(case)
        g = np.random.default_rng(1).standard_normal((N, Ho, Wo, Co)).astype(np.float32)
        cop = T._pad16(Co)
        ldx, ldo = Ci + pad, cop + pad
        xd, wd = dev(x, tdt, ldx), dev(w, tdt)
        M = N * Ho * Wo
        yd = torch.zeros((M, ldo), dtype=tdt, device=cuda)
        # one (sum, M2) per statistics block of the kernel the plan picks: 64 rows at the least
        stats = torch.zeros(((M + 63) // 64, Co, 2), dtype=torch.float32, device=cuda)
        rec(f"{tag} fwd", LIB.seg_op_conv_fwd(abi, xd.data_ptr(), N, H, W, Ci, ldx, wd.data_ptr(), Co, k, s, r,
                                             int(ep), yd.data_ptr(), ldo, stats.data_ptr(), st), yd, stats)
        gd = dev(g, tdt, ldo)
        if Ci != 3:
            wt = np.ascontiguousarray(np.flip(w, (1, 2)).transpose(3, 1, 2, 0))
            wtd = dev(wt, tdt)
            dx = torch.zeros((N * H * W, ldx), dtype=tdt, device=cuda)
            rec(f"{tag} dgrad", LIB.seg_op_conv_dgrad(abi, gd.data_ptr(), N, Ho, Wo, Co, ldo, wtd.data_ptr(), Ci, k,
                                                     s, r, int(ep), H, W, dx.data_ptr(), ldx, st), dx)
        dw = torch.zeros((cop, k, k, Ci), dtype=torch.float32, device=cuda)
        rec(f"{tag} wgrad", LIB.seg_op_conv_wgrad(abi, gd.data_ptr(), N, Ho, Wo, cop, ldo, xd.data_ptr(), H, W, Ci,
                                                 ldx, k, s, r, int(ep), dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 st), dw)

    for dtype in ("bf16", "fp16"):
        tdt, abi = T.TDT[dtype], T.ABI[dtype]
        for i, c in enumerate(T.CASES):
            conv_case(f"{dtype} CASES[{i}]", c, dtype, 0)
        for i, c in enumerate(T.LD_CASES):
            conv_case(f"{dtype} LD_CASES[{i}]", c, dtype, 64)
        for i, c in enumerate(T.WGRAD_PATCH_CASES):
            conv_case(f"{dtype} WGRAD_PATCH_CASES[{i}]", c, dtype, 0)
        for i, c in enumerate(T.RES_CASES):
            N, H, W, Co, Ci, with_r, with_m = c
            g = np.random.default_rng(7)
            dyd = dev(g.standard_normal((N * H * W, Co)), tdt)
            wtd = dev((g.standard_normal((Co, Ci)) * np.sqrt(2.0 / Ci)).T, tdt)
            rd = dev(g.standard_normal((N * H * W, Ci)), tdt) if with_r else None
            md = torch.as_tensor(g.integers(0, 256, size=(N * H * W, Ci // 8), dtype=np.uint8)).to(cuda) if with_m else None
            dx = torch.zeros((N * H * W, Ci), dtype=tdt, device=cuda)
            rec(f"{dtype} RES_CASES[{i}] dgrad_res",
                LIB.seg_op_conv_dgrad_res(abi, dyd.data_ptr(), N, H, W, Co, Co, wtd.data_ptr(), Ci, dx.data_ptr(), Ci,
                                          rd.data_ptr() if with_r else None, Ci,
                                          md.data_ptr() if with_m else None, st), dx)
        for i, (c, bm, bn, splits) in enumerate(T.WGRAD_CFG_CASES):
            N, H, W, Ci, Co, k, s, r, ep = c
            x, _ = T._tensors(c)
            _, Ho, Wo = T._geom(c)
            gd = dev(np.random.default_rng(3).standard_normal((N, Ho, Wo, Co)), tdt)
            xd = dev(x, tdt)
            dw = torch.zeros((Co, k, k, Ci), dtype=torch.float32, device=cuda)
            slabs = torch.zeros((splits * Co * k * k * Ci,), dtype=torch.float32, device=cuda)
            rec(f"{dtype} WGRAD_CFG_CASES[{i}] wgrad_cfg",
                LIB.seg_op_conv_wgrad_cfg(abi, gd.data_ptr(), N, Ho, Wo, Co, Co, xd.data_ptr(), H, W, Ci, Ci, k, s, r,
                                          int(ep), dw.data_ptr(), slabs.data_ptr(), slabs.numel() * 4, bm, bn,
                                          splits, st), dw, slabs)
    json.dump(rows, open(out, "w"))


def run(lib, out):
    env = dict(os.environ)
    env.pop("SEG_HIP_LIB", None)
    if lib:
        env["SEG_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, capture_output=True,
                       text=True, timeout=420)
    if r.returncode:
        print(r.stdout[-2000:], r.stderr[-2000:])
        r.check_returncode()
    return json.load(open(out))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    a = run(None, "/tmp/ab_conv_bits_a.json")
    b = run(os.path.abspath(sys.argv[1]), "/tmp/ab_conv_bits_b.json")
    assert [r[0] for r in a] == [r[0] for r in b]
    bad = [(x, y) for x, y in zip(a, b) if x != y]
    failed = [x for x in a if x[1] != 0]
    for x, y in bad:
        print("DIFFERENT", x, y)
    for x in failed:
        print("not launched (same return code from both libraries)", x)
    nbuf = sum(len(x) - 2 for x in a)
    print(f"{len(a)} launches ({len(failed)} turned away by both), {nbuf} buffers: "
          f"{'all checksums equal' if not bad else f'{len(bad)} launches differ'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
