"""Cost table of the device-side training augmentation (csrc/augment.hip), on the GPU, through
the library only. For C2's per-pixel batch (4 x 1024 x 2048 from same-size raw images) and for
one weak-stream image of C1's shape (512 x 1024 window of a 768 x 1024 JPEG's aspect-preserving
resize; the bbox / tag sub-batches go through image by image), one row per setting:

    all off (seg_prepare_images[_crop] + seg_prepare_labels: the baseline) | colour only |
    flip only | scale up | scale down | all on

with, per pass (contrast mean, colour, down-scale mean, geometry; seg_augment_profile's device
events) and for the labels gather and the total (device events around the calls): time, the
compulsory bytes (every operand read / written once) and GB/s. Times are medians of REPS calls
after WARM warm-up calls per row. The added time is also given as a share of the 34.91 ms C2
step of BENCH_r06.json.

With --blur: the blur pass (seg_augment_profile_blur's device events) on the same C2 batch for
the median and the bilateral filter at k = 3, 5, 7, 9, beside its HBM floor (12 B read + 12 B
written per pixel at the COPY_TBS copy rate of DESIGN 0a'), and the whole augmentation with all
four stages on, as milliseconds and as a share of BLUR_STEP_MS (a plain bench.py run of the
commit before the blur, same session).

    python tools/aug_table.py > profiles/augment_table.txt
    python tools/aug_table.py --blur > profiles/augment_blur_table.txt"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")]

WARM, REPS = 5, 30
STEP_MS = 34.91          # BENCH_r06.json ms_per_step (C2)
BLUR_STEP_MS = 34.66     # bench.py --steps 20 --warmup 5 of the parent commit: 34.69 / 34.67 / 34.62
COPY_TBS = 6.29          # DESIGN 0a': the copy ceiling
L2C = [-1] * 7 + list(range(19)) + [-1] * 8
PASSES = ("contrast mean", "colour", "down mean", "geometry")


def records(kind, n, H, W):
    from input_pipelines.augment import off_params
    p = off_params(n, H, W, void_cid=19)
    if kind in ("colour", "all"):
        p["color_order"] = 1
        p["brightness_delta"], p["saturation_factor"] = 0.05, 1.2
        p["hue_delta"], p["contrast_factor"] = -0.04, 0.8
    if kind in ("flip", "all"):
        p["quantize"], p["flip"] = 1, 1
    if kind in ("up", "all"):
        sh, sw = int(0.75 * H), int(0.75 * W)
        if kind == "up":
            p["scale_mode"], p["sh"], p["sw"], p["oy"], p["ox"] = 1, sh, sw, (H - sh) // 2, (W - sw) // 2
        else:   # all on: half the images up, half down, as the draws do on average
            p["scale_mode"] = [1 + (i % 2) for i in range(n)]
            p["sh"], p["sw"] = sh, sw
            p["oy"], p["ox"] = [(H - sh) // 2 * (1 - i % 2) for i in range(n)], [0] * n
    if kind == "down":
        p["scale_mode"], p["sh"], p["sw"] = 2, int(0.75 * H), int(0.75 * W)
    return p


def pass_bytes(p, raw_px, H, W):
    """Compulsory bytes of the four image passes and of the labels gather."""
    npix = H * W
    col = int((p["color_order"] >= 0).sum())
    geo = (p["flip"] != 0) | (p["scale_mode"] != 0)
    down = p["scale_mode"] == 2
    src = np.where(p["scale_mode"] == 1, p["sh"].astype(np.int64) * p["sw"], npix)   # up reads its crop
    return [col * raw_px * 3, len(p) * (raw_px * 3 + npix * 12), int(down.sum()) * npix * 12,
            int((src[geo] * 12).sum()) + int(geo.sum()) * npix * 12], len(p) * (raw_px + npix * 4)


def median_ms(fn, torch):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def table(title, n, src, H, W, resized, offset, weak, torch, dev):
    from input_pipelines.augment import augment_images, augment_labels
    from input_pipelines.tfrecords import prepare_images, prepare_images_crop, prepare_labels
    from seg_hip import LIB, check
    g = torch.Generator().manual_seed(1)
    raw = torch.randint(0, 256, (n,) + src + (3,), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 34, (n,) + src, dtype=torch.uint8, generator=g).to(dev)
    raw_px = src[0] * src[1]
    print(f"== {title}: n = {n}, raw {src[0]}x{src[1]} -> {H}x{W}"
          + (f" (resized {resized[0]}x{resized[1]}, window at {offset})" if weak else ""))
    print(f"{'row':<12} {'pass':<14} {'ms':>8} {'MB':>9} {'GB/s':>8}")

    def line(row, name, ms, nbytes):
        rate = f"{nbytes / ms / 1e6:8.0f}" if ms > 0 else f"{'-':>8}"
        print(f"{row:<12} {name:<14} {ms:8.4f} {nbytes / 1e6:9.2f} {rate}")
    if weak:
        base_i = median_ms(lambda: prepare_images_crop(raw, resized, offset, H, W), torch)
        base_l = 0.0
    else:
        base_i = median_ms(lambda: prepare_images(raw, H, W), torch)
        base_l = median_ms(lambda: prepare_labels(lab, H, W, L2C), torch)
    line("all off", "images", base_i, n * (raw_px * 3 + H * W * 12))
    if not weak:
        line("all off", "labels", base_l, n * (raw_px + H * W * 4))
    line("all off", "total", base_i + base_l, n * (raw_px * 3 + H * W * 12) + (0 if weak else n * (raw_px + H * W * 4)))
    kw = dict(resized=resized, offset=offset) if weak else {}
    for kind in (("colour", "flip", "all") if weak else ("colour", "flip", "up", "down", "all")):
        p = records(kind, n, H, W)
        if weak:
            p["scale_mode"] = 0      # the weak streams get colour + flip only
        pb, lb = pass_bytes(p, raw_px, H, W)
        check(LIB.seg_augment_profile(1, None))
        per = []
        for _ in range(WARM + REPS):
            augment_images(raw, p, H, W, **kw)
            ms = (ctypes.c_float * 4)()
            check(LIB.seg_augment_profile(1, ms))
            per.append(list(ms))
        check(LIB.seg_augment_profile(0, None))
        per = np.median(np.asarray(per[WARM:]), 0)
        name = {"all": "all on", "up": "scale up", "down": "scale down"}.get(kind, kind + " only")
        for k in range(4):
            if pb[k]:
                line(name, PASSES[k], float(per[k]), pb[k])
        tot_i = median_ms(lambda: augment_images(raw, p, H, W, **kw), torch)
        line(name, "images (call)", tot_i, sum(pb))
        tot_l = 0.0
        if not weak:
            tot_l = median_ms(lambda: augment_labels(lab, p, H, W, L2C), torch)
            line(name, "labels", tot_l, lb)
        added = tot_i + tot_l - base_i - base_l
        line(name, "total", tot_i + tot_l, sum(pb) + (0 if weak else lb))
        print(f"{name:<12} added over all off: {added:+.4f} ms = {100 * added / STEP_MS:+.2f} % of the "
              f"{STEP_MS} ms C2 step; x{(tot_i + tot_l) / (base_i + base_l):.2f} the baseline row")
    print()


def blur_table(n, H, W, torch, dev):
    """The blur pass alone per (filter, k), then all four stages on."""
    from input_pipelines.augment import augment_images, augment_labels, blur_draw_range
    from seg_hip import LIB, check
    g = torch.Generator().manual_seed(1)
    raw = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 34, (n, H, W), dtype=torch.uint8, generator=g).to(dev)
    sigma = blur_draw_range(H, W)[1]
    nbytes = n * H * W * 24
    floor = nbytes / (COPY_TBS * 1e9)     # ms
    print(f"== blur pass, C2 per-pixel batch: n = {n}, {H}x{W}, sigma = {sigma:g}; compulsory "
          f"{nbytes / 1e6:.2f} MB (12 B read + 12 B written per pixel) = {floor:.4f} ms at "
          f"{COPY_TBS} TB/s")
    print(f"{'filter':<10} {'k':>2} {'blur ms':>9} {'x floor':>8} {'GB/s':>7} {'% step':>7} "
          f"{'images (call) ms':>17}")

    def blur_ms(p):
        check(LIB.seg_augment_profile(1, None))
        per = []
        for _ in range(WARM + REPS):
            augment_images(raw, p, H, W)
            ms = ctypes.c_float(0)
            check(LIB.seg_augment_profile_blur(ctypes.byref(ms)))
            per.append(ms.value)
        check(LIB.seg_augment_profile(0, None))
        return float(np.median(per[WARM:]))
    for mode, name in ((1, "median"), (2, "bilateral")):
        for k in (3, 5, 7, 9):
            p = records("off", n, H, W)
            p["blur"]["mode"], p["blur"]["ksize"], p["blur"]["sigma"] = mode, k, sigma if mode == 2 else 0
            ms = blur_ms(p)
            call = median_ms(lambda: augment_images(raw, p, H, W), torch)
            print(f"{name:<10} {k:>2} {ms:9.4f} {ms / floor:8.2f} {nbytes / ms / 1e6:7.0f} "
                  f"{100 * ms / BLUR_STEP_MS:7.2f} {call:17.4f}")
    print()
    print(f"== all four stages on (colour, blur, flip, half the images scaled up, half down), "
          f"images + labels; share of the {BLUR_STEP_MS} ms C2 step")
    print(f"{'blur':<14} {'blur ms':>9} {'images ms':>10} {'labels ms':>10} {'total ms':>9} {'% step':>7}")
    for mode, name, k in ((0, "none", 0), (1, "median", 3), (1, "median", 9), (2, "bilateral", 3),
                          (2, "bilateral", 9)):
        p = records("all", n, H, W)
        p["blur"]["mode"], p["blur"]["ksize"], p["blur"]["sigma"] = mode, k, sigma if mode == 2 else 0
        ms = blur_ms(p)
        ti = median_ms(lambda: augment_images(raw, p, H, W), torch)
        tl = median_ms(lambda: augment_labels(lab, p, H, W, L2C), torch)
        print(f"{(name + (f' k={k}' if k else '')):<14} {ms:9.4f} {ti:10.4f} {tl:10.4f} {ti + tl:9.4f} "
              f"{100 * (ti + tl) / BLUR_STEP_MS:7.2f}")


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("aug_table.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    if "--blur" in sys.argv[1:]:
        print(f"# {torch.cuda.get_device_name(0)}; medians of {REPS} calls after {WARM} warm-up "
              "calls; 'blur ms' is device events around the blur kernel, the call columns include "
              "the wrapper (parameter upload, workspace and output allocation)")
        blur_table(4, 1024, 2048, torch, dev)
        return
    print(f"# {torch.cuda.get_device_name(0)}; medians of {REPS} calls after {WARM} warm-up calls; "
          "'images (call)' and 'labels' include the wrapper (parameter upload, workspace and "
          "output allocation), the pass rows are device events around the kernels")
    table("C2 per-pixel batch", 4, (1024, 2048), 1024, 2048, None, (0, 0), False, torch, dev)
    table("C1 weak-stream image", 1, (768, 1024), 512, 1024, (768, 1024), (128, 0), True, torch, dev)


if __name__ == "__main__":
    main()
