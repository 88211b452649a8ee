"""Cost table of test-time augmentation (csrc/tta.hip, estimator/tta.py), on the GPU.

Kernel table (default): seg_tta_decisions at 1024 x 2048, N = 1, on seeded random low-resolution
logits of the sizes the scale sets give, beside the PyTorch composition a user has to write
without it (interpolate(align_corners=True) to H x W, per-head softmax, flip, sum, argmax,
gathers), both timed with device events in alternating rounds of one process; medians of REPS
rounds after WARM warm-up rounds, and the share of pixels on which the two disagree.

    6 entries   scales 0.75 1 1.25 with flip          Cityscapes widths 14 | 7 | 3
    14 entries  scales 0.5 0.75 1 1.25 1.5 1.75 2 with flip, Cityscapes widths
    6 entries   scales 0.75 1 1.25 with flip          Vistas widths 53 | 12 | 5

--pass: the whole EVAL pass per image (forwards + decisions) of a 1024 x 2048 PSP context at
Nb = 1 for both scale sets against the single-scale pass, and the device memory the scale contexts
hold (torch.cuda.mem_get_info before and after they are built).

    python tools/tta_table.py > profiles/tta_table.txt
    python tools/tta_table.py --pass [--dtype bf16] >> profiles/tta_table.txt"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")]

WARM, REPS = 3, 15
H, W = 1024, 2048
SETS = {"3 scales": (0.75, 1.0, 1.25), "7 scales": (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)}
WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}


def tables(dataset, torch, dev):
    from oracle.tfseg import TABLES
    t = TABLES[dataset]
    lt = lambda v: torch.as_tensor(v, dtype=torch.long, device=dev)
    return t["cid_l1_vehicle"], t["cid_l1_human"], lt(t["l1_to_common"]), lt(t["veh_to_common"]), lt(t["hum_to_common"])


def torch_composition(entries, dataset, torch, tb):
    """What the parent commit leaves to the user: full-resolution probabilities per entry."""
    import torch.nn.functional as F
    c1, c2, c3 = WIDTHS[dataset]
    total = None
    for lg, flip in entries:
        up = F.interpolate(lg.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True)
        p = torch.cat([torch.softmax(up[:, :c1], 1), torch.softmax(up[:, c1:c1 + c2], 1),
                       torch.softmax(up[:, c1 + c2:], 1)], 1)
        if flip:
            p = torch.flip(p, dims=(3,))
        total = p if total is None else total + p
    veh, hum, l1c, vc, hc = tb
    l1d, vd, hd = total[:, :c1].argmax(1), total[:, c1:c1 + c2].argmax(1), total[:, c1 + c2:].argmax(1)
    return torch.where(l1d == veh, vc[vd], torch.where(l1d == hum, hc[hd], l1c[l1d])).to(torch.int32)


def kernel_table(torch, dev):
    from estimator.tta import tta_sizes
    from seg_hip import SegContext
    print(f"# {torch.cuda.get_device_name(0)}; seg_tta_decisions vs the PyTorch composition at {H} x {W}, "
          f"N = 1; device events, alternating rounds, medians of {REPS} after {WARM} warm-up rounds")
    print(f"{'case':<28} {'entries':>7} {'fused ms':>9} {'min':>8} {'torch ms':>9} {'min':>8} {'x':>7} {'differ':>9}")
    for dataset, setname in (("cityscapes", "3 scales"), ("cityscapes", "7 scales"), ("vistas", "3 scales")):
        ct = sum(WIDTHS[dataset])
        ctx = SegContext(pyramid="none", height=H, width=W, nb_pp=1, dtype="bf16", dataset=dataset)
        g = torch.Generator().manual_seed(7)
        entries = []
        for h, w in tta_sizes(H, W, SETS[setname]):
            for flip in (False, True):
                entries.append((3.0 * torch.randn((1, h // 8, w // 8, ct), generator=g).to(dev), flip))
        n_map = 66 if dataset == "vistas" else 20
        out = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        tb = tables(dataset, torch, dev)
        fused = lambda: ctx.tta_decisions(entries, list(range(n_map)), out)
        base = lambda: torch_composition(entries, dataset, torch, tb)
        ts = {"fused": [], "torch": []}
        for r in range(WARM + REPS):
            for name, fn in (("fused", fused), ("torch", base)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = fn()
                b.record()
                b.synchronize()
                if r >= WARM:
                    ts[name].append(a.elapsed_time(b))
        differ = float((out != res).float().mean())
        f, t = np.asarray(ts["fused"]), np.asarray(ts["torch"])
        print(f"{dataset + ' ' + setname + ' + flip':<28} {len(entries):>7} {np.median(f):9.4f} {f.min():8.4f} "
              f"{np.median(t):9.4f} {t.min():8.4f} {np.median(t) / np.median(f):7.1f} {differ:9.2e}")
        ctx.close()
        del entries, res
        torch.cuda.empty_cache()


def pass_table(torch, dev, dtype):
    from estimator.mode_keys import ModeKeys
    from estimator.tta import TTADriver
    from models.resnet50_extended_model_hierarchical import get_context, release_contexts
    print(f"# whole EVAL pass per image at {H} x {W}, PSP, {dtype}, Nb = 1: forwards + decisions; host "
          f"clock around {REPS} passes ending in a device synchronise, after {WARM} warm-up passes")
    s = argparse.Namespace(Nb=1, height_feature_extractor=H, width_feature_extractor=W,
                           per_pixel_dataset_name="cityscapes", compute_dtype=dtype, pyramid="psp",
                           name_feature_extractor="resnet_v1_50")
    import time
    x = torch.rand((1, H, W, 3), device=dev) * 2 - 1
    out = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    cid_map = list(range(19)) + [-1]

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / REPS * 1e3
    primary = get_context(None, s, mode=ModeKeys.EVAL)
    primary.set_bn_inference(True)

    def single():
        primary.forward(x)
        primary.predict(cid_map, out)
    print(f"{'single scale':<22} {timed(single):9.2f} ms / image")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]   # the 7-scale set contains the 3-scale set's contexts
    for name, scales in SETS.items():
        try:
            drv = TTADriver(primary, None, s, ModeKeys.EVAL, scales, True)

            def multi():
                primary.forward(x)
                drv.decisions(x, cid_map, out)
            ms = timed(multi)
        except RuntimeError as e:   # the pyramid does not fit beside the primary context
            print(f"{name + ' + flip':<22} not run: {str(e).splitlines()[0][:120]}")
            continue
        held = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 30
        print(f"{name + ' + flip':<22} {ms:9.2f} ms / image; scale contexts (and torch's cache) hold "
              f"{held:.2f} GiB more than the primary alone")
    release_contexts()


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tta_table.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass", dest="whole", action="store_true")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    a = ap.parse_args()
    if a.whole:
        pass_table(torch, dev, a.dtype)
    else:
        kernel_table(torch, dev)


if __name__ == "__main__":
    main()
