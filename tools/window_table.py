"""Cost table of sliding-window inference (csrc/window.hip, estimator/windows.py), on the GPU.

Kernel table (default): seg_window_decisions at canvas 1024 x 2048, windows 512 x 1024, stride
(342, 683) -- ys = [0, 342, 512], xs = [0, 683, 1024], 9 windows -- N = 1, on seeded random
64 x 128 logits, Cityscapes and Vistas widths, with and without flip. The yardstick is
seg_tta_decisions (the same arithmetic per entry, no window geometry) at network size
1024 x 2048 with 4 and with 8 entries of 64 x 128 logits, timed in the same process. Device
events, alternating rounds, medians and minima of REPS rounds after WARM warm-up rounds. The
unit both are reported in is ns per (pixel, entry) pair: for the window kernel the pairs are
the covering entries summed over the canvas pixels, for the yardstick pixels x entries. The rows
in brackets are not the yardstick: seg_tta_decisions at 512 x 1024, where a low-resolution cell
spans 8 pixels as in the windows (16 in the yardstick).

--pass: the whole EVAL pass per image, R50 + PSP, Nb = 1: the 9 window forwards at 512 x 1024
plus seg_window_decisions against one 1024 x 2048 forward plus seg_predict, and the device
memory held beyond the primary context while the entries' logits are alive.

    python tools/window_table.py > profiles/window_table.txt
    python tools/window_table.py --pass [--dtype bf16] >> profiles/window_table.txt"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")]

WARM, REPS = 3, 15
H, W = 512, 1024            # the network = window size
HC, WC = 1024, 2048         # the canvas, and the yardstick's network size
STRIDE = (342, 683)
LOW = (64, 128)
WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}


def kernel_table(torch, dev):
    from estimator.windows import window_grid
    from seg_hip import SegContext
    print(f"# {torch.cuda.get_device_name(0)}; seg_window_decisions at canvas {HC} x {WC}, windows {H} x {W}, "
          f"stride {STRIDE}, beside seg_tta_decisions at network size {HC} x {WC}; N = 1, {LOW[0]} x {LOW[1]} "
          f"logits; device events, alternating rounds, medians of {REPS} after {WARM} warm-up rounds")
    print(f"{'case':<34} {'entries':>7} {'pairs':>10} {'ms':>8} {'min':>8} {'ns/pair':>8} "
          f"{'x tta 4':>8} {'x tta 8':>8}")
    for dataset in ("cityscapes", "vistas"):
        ct = sum(WIDTHS[dataset])
        n_map = 66 if dataset == "vistas" else 20
        cid_map = list(range(n_map))
        small = SegContext(pyramid="none", height=H, width=W, nb_pp=1, dtype="bf16", dataset=dataset)
        big = SegContext(pyramid="none", height=HC, width=WC, nb_pp=1, dtype="bf16", dataset=dataset)
        g = torch.Generator().manual_seed(7)
        logits = [3.0 * torch.randn((1,) + LOW + (ct,), generator=g).to(dev) for _ in range(18)]
        out = torch.empty((1, HC, WC), dtype=torch.int32, device=dev)
        out_small = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        cases = {}
        for flip in (False, True):
            ys, xs = window_grid((HC, WC), (H, W), STRIDE, flip)
            assert (ys, xs) == ([0, 342, 512], [0, 683, 1024])
            n = len(ys) * len(xs) * (2 if flip else 1)
            ents = logits[:n]
            cases[f"{dataset} windows{' + flip' if flip else ''}"] = (
                n, n * H * W,
                lambda ents=ents, ys=ys, xs=xs, flip=flip: small.window_decisions(
                    ents, ys, xs, flip, (HC, WC), cid_map, out))
        for e in (4, 8):
            ents = [(lg, bool(i & 1)) for i, lg in enumerate(logits[:e])]
            cases[f"{dataset} seg_tta_decisions {e}"] = (
                e, e * HC * WC, lambda ents=ents: big.tta_decisions(ents, cid_map, out))
        # not the yardstick: the same kernel at the windows' own upsampling factor (8 instead of
        # 16 pixels per low-resolution cell), to tell the geometry's share from the kernel's
        for e in (4, 8):
            ents = [(lg, bool(i & 1)) for i, lg in enumerate(logits[:e])]
            cases[f"({dataset} tta {e} at {H} x {W})"] = (
                e, e * H * W, lambda ents=ents: small.tta_decisions(ents, cid_map, out_small))
        ts = {k: [] for k in cases}
        for r in range(WARM + REPS):
            for name, (_, _, fn) in cases.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if r >= WARM:
                    ts[name].append(a.elapsed_time(b))
        per = {k: np.median(ts[k]) * 1e6 / cases[k][1] for k in cases}
        t4, t8 = per[f"{dataset} seg_tta_decisions 4"], per[f"{dataset} seg_tta_decisions 8"]
        for name, (n, pairs, _) in cases.items():
            t = np.asarray(ts[name])
            ratios = "" if "seg_tta" in name else f"{per[name] / t4:8.2f} {per[name] / t8:8.2f}"
            print(f"{name:<34} {n:>7} {pairs:>10} {np.median(t):8.4f} {t.min():8.4f} {per[name]:8.4f} {ratios}")
        small.close()
        big.close()
        del logits, cases
        torch.cuda.empty_cache()


def pass_table(torch, dev, dtype):
    import time
    from estimator.mode_keys import ModeKeys
    from estimator.windows import WindowDriver, default_stride
    from models.resnet50_extended_model_hierarchical import get_context, release_contexts
    print(f"# whole EVAL pass per image, R50 + PSP, {dtype}, Nb = 1: forwards + decisions; host clock around "
          f"{REPS} passes ending in a device synchronise, after {WARM} warm-up passes")

    def settings(h, w):
        return argparse.Namespace(Nb=1, height_feature_extractor=h, width_feature_extractor=w,
                                  per_pixel_dataset_name="cityscapes", compute_dtype=dtype, pyramid="psp",
                                  name_feature_extractor="resnet_v1_50")

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / REPS * 1e3
    x = torch.rand((1, HC, WC, 3), device=dev) * 2 - 1
    out = torch.empty((1, HC, WC), dtype=torch.int32, device=dev)
    cid_map = list(range(19)) + [-1]
    primary = get_context(None, settings(H, W), mode=ModeKeys.EVAL)
    primary.set_bn_inference(True)
    drv = WindowDriver(primary, (HC, WC), default_stride(H, W), False)
    assert (drv.ys, drv.xs) == ([0, 342, 512], [0, 683, 1024])
    torch.cuda.synchronize()
    free0, alloc0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_allocated()
    ents = drv.decisions(x, cid_map, out)
    torch.cuda.synchronize()
    held = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20
    live = (torch.cuda.memory_allocated() - alloc0) / 2 ** 20
    ms = timed(lambda: drv.decisions(x, cid_map, out))
    print(f"{len(ents)} windows of {H} x {W} on {HC} x {WC}: {ms:9.2f} ms / image; beyond the primary context "
          f"{live:.2f} MiB of live tensors (the cloned logits), {held:.2f} MiB with torch's cache")
    del ents
    full = get_context(None, settings(HC, WC), mode=ModeKeys.EVAL)
    full.set_bn_inference(True)

    def single():
        full.forward(x)
        full.predict(cid_map, out)
    print(f"one {HC} x {WC} forward + seg_predict: {timed(single):9.2f} ms / image")
    release_contexts()


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("window_table.py measures on the GPU; none is visible")
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
