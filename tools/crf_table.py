"""Cost table of the mean-field CRF refinement (csrc/crf.hip, estimator/crf.py), on the GPU.

Kernel table (default): seg_crf_decisions at 1024 x 2048, N = 1, Cityscapes and Vistas widths, on
seeded random probabilities and an image on the 256 levels, (r, d) = (3, 1) and (2, 3), with
T = 0 (the decision kernel alone), T = 1 and T = 5. Device events, alternating rounds in one
process, medians and minima of REPS rounds after WARM warm-up rounds (the protocol of
tools/window_table.py). One mean-field iteration is (T = 5 minus T = 1) / 4. Beside it the least
traffic an iteration can have -- read Q^t, P and I, write Q^{t+1}: (3 * CT + 3) * 4 bytes per
pixel -- the bytes/s that traffic would mean at the measured time, and their share of the 8.0 TB/s
HBM peak (the kernel stages neighbours through LDS, so this is the share of the memory roofline,
not a utilisation).

--pass: the whole EVAL pass per image, R50 + PSP, Nb = 1 at 1024 x 2048: forward + seg_predict
against forward + seg_full_predictions' probabilities + seg_crf_decisions with T = 5 at the
default parameters.

    python tools/crf_table.py > profiles/crf_table.txt
    python tools/crf_table.py --pass [--dtype bf16] >> profiles/crf_table.txt"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")]

WARM, REPS = 3, 15
H, W = 1024, 2048
WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}
GEOMETRY = [(3, 1), (2, 3)]
HBM_PEAK = 8.0e12


def kernel_table(torch, dev):
    from seg_hip import CrfParams, SegContext, crf_workspace_bytes
    print(f"# {torch.cuda.get_device_name(0)}; seg_crf_decisions at {H} x {W}, N = 1; device events, "
          f"alternating rounds, medians of {REPS} after {WARM} warm-up rounds; one iteration = (T5 - T1) / 4; "
          f"least traffic = (3 CT + 3) * 4 bytes per pixel")
    print(f"{'case':<26} {'T=0 ms':>8} {'T=1 ms':>8} {'T=5 ms':>8} {'T=5 min':>8} {'ms/iter':>8} "
          f"{'least MB':>9} {'GB/s':>8} {'of HBM':>7}")
    for dataset in ("cityscapes", "vistas"):
        ct = sum(WIDTHS[dataset])
        cid_map = list(range(66 if dataset == "vistas" else 20))
        # a small context: the entry takes its size from its arguments
        ctx = SegContext(pyramid="none", height=64, width=128, nb_pp=1, dtype="bf16", dataset=dataset)
        g = torch.Generator().manual_seed(11)
        logits = 2.0 * torch.randn((1, H, W, ct), generator=g)
        lo, parts = 0, []
        for c in WIDTHS[dataset]:
            parts.append(torch.softmax(logits[..., lo:lo + c], dim=-1))
            lo += c
        probs = torch.cat(parts, dim=-1).contiguous().to(dev)
        images = (torch.randint(0, 256, (1, H, W, 3), generator=g).float() * (2.0 / 255.0) - 1.0).to(dev)
        del logits, parts
        ws = torch.empty(crf_workspace_bytes(1, H, W, ct), dtype=torch.uint8, device=dev)
        out = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        cases = {}
        for r, d in GEOMETRY:
            for T in (0, 1, 5):
                p = CrfParams(T, r, d, 4.0, 3.0, 67.0, 3.0, 3.0)
                cases[(r, d, T)] = lambda p=p: ctx.crf_decisions(probs, images, p, cid_map, out, workspace=ws)
        ts = {k: [] for k in cases}
        for rnd in range(WARM + REPS):
            for name, fn in cases.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rnd >= WARM:
                    ts[name].append(a.elapsed_time(b))
        least = (3 * ct + 3) * 4 * H * W
        for r, d in GEOMETRY:
            t0, t1, t5 = (np.asarray(ts[(r, d, T)]) for T in (0, 1, 5))
            it = (np.median(t5) - np.median(t1)) / 4.0
            rate = least / (it * 1e-3)
            print(f"{dataset + f' r {r} d {d}':<26} {np.median(t0):8.4f} {np.median(t1):8.4f} "
                  f"{np.median(t5):8.4f} {t5.min():8.4f} {it:8.4f} {least / 1e6:9.1f} {rate / 1e9:8.1f} "
                  f"{rate / HBM_PEAK:7.1%}")
        ctx.close()
        del probs, images, ws, cases
        torch.cuda.empty_cache()


def pass_table(torch, dev, dtype):
    import time
    from estimator.crf import CRFDriver, CRFSettings
    from estimator.mode_keys import ModeKeys
    from models.resnet50_extended_model_hierarchical import get_context, release_contexts
    print(f"# whole EVAL pass per image, R50 + PSP, {dtype}, Nb = 1 at {H} x {W}; host clock around {REPS} "
          f"passes ending in a device synchronise, after {WARM} warm-up passes")
    s = argparse.Namespace(Nb=1, height_feature_extractor=H, width_feature_extractor=W,
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
    x = torch.rand((1, H, W, 3), device=dev) * 2 - 1
    out = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    cid_map = list(range(19)) + [-1]
    ctx = get_context(None, s, mode=ModeKeys.EVAL)
    ctx.set_bn_inference(True)
    drv = CRFDriver(ctx, CRFSettings(5, 3, 1, 4.0, 3.0, 67.0, 3.0, 3.0))
    probs = torch.empty((1, H, W, 24), device=dev)

    def plain():
        ctx.forward(x)
        ctx.predict(cid_map, out)

    def refined():
        ctx.forward(x)
        ctx.full_predictions(probs=probs)
        drv.decisions(probs, x, cid_map, out)
    a = timed(plain)
    b = timed(refined)
    print(f"forward + seg_predict:                                   {a:9.2f} ms / image")
    print(f"forward + probabilities + seg_crf_decisions (T = 5):     {b:9.2f} ms / image  (+{b - a:.2f} ms)")
    release_contexts()


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("crf_table.py measures on the GPU; none is visible")
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
