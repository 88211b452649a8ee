"""Cost table of the box-label kernels (csrc/boxlabel.hip), on the GPU.

seg_box_constrain, seg_box_decisions and seg_box_finalize at 1024 x 2048, N = 1, Cityscapes and
Vistas widths, on seeded random probabilities, with 16 and 516 (the reference's MAX_N_BBOXES)
seeded boxes per image from a 1200 x 1600 source. Device events, alternating rounds in one process,
medians and minima of REPS rounds after WARM warm-up rounds (the protocol of tools/crf_table.py).
Beside each time the bytes the kernel has to move per pixel -- constrain: read and write CT floats
plus the 2-byte mask; decide: read CT floats, write the label and the confidence; finalize: read
and write one label -- and the bytes/s they mean at the measured time. The box loop (a pixel walks
every box of its image in LDS) is work the byte count does not see.

    python tools/boxlabel_table.py > profiles/boxlabel_table.txt"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")]

WARM, REPS = 3, 15
H, W = 1024, 2048
SRC = (1200, 1600)
WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}
BOXES = (16, 516)


def box_item(rng, k):
    lo = rng.random((k, 2)).astype(np.float32)
    hi = np.minimum(lo + (rng.random((k, 2)) * 0.3).astype(np.float32), np.float32(1.0))
    coords = np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]], 1).astype(np.float32)
    return rng.integers(0, 14, size=k), coords, SRC, (H, W), (0, 0)


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("boxlabel_table.py measures on the GPU; none is visible")
    from seg_hip import SegContext
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; box-label entries at {H} x {W}, N = 1, boxes from a "
          f"{SRC[0]} x {SRC[1]} source; device events, alternating rounds, medians of {REPS} after {WARM} "
          f"warm-up rounds")
    print(f"{'case':<34} {'ms':>8} {'min ms':>8} {'B/pixel':>8} {'MB':>8} {'GB/s':>8}")
    for dataset in ("cityscapes", "vistas"):
        ct = sum(WIDTHS[dataset])
        # a small context: the entries take their size from their arguments
        ctx = SegContext(pyramid="none", height=64, width=128, nb_pp=1, dtype="bf16", dataset=dataset)
        g = torch.Generator().manual_seed(11)
        logits = 2.0 * torch.randn((1, H, W, ct), generator=g)
        lo, parts = 0, []
        for c in WIDTHS[dataset]:
            parts.append(torch.softmax(logits[..., lo:lo + c], dim=-1))
            lo += c
        probs = torch.cat(parts, dim=-1).contiguous().to(dev)
        del logits, parts
        q = torch.empty_like(probs)
        mask = torch.empty((1, H, W), dtype=torch.int16, device=dev)
        labels = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        conf = torch.empty((1, H, W), device=dev)
        out = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        cases, bytes_px = {}, {}
        for k in BOXES:
            b = ctx.upload_boxes([box_item(np.random.default_rng(3), k)], (H, W))
            counts = torch.empty((k, 2), dtype=torch.int32, device=dev)
            reject = torch.zeros(k, dtype=torch.int32, device=dev)
            reject[::2] = 1
            cases[("constrain", k)] = lambda b=b: ctx.box_constrain(probs, b, q, mask_out=mask)
            cases[("decide", k)] = lambda b=b, counts=counts: ctx.box_decisions(q, b, 0.3, labels, counts, conf_out=conf)
            cases[("finalize", k)] = lambda b=b, reject=reject: ctx.box_finalize(labels, b, reject, out)
            bytes_px.update({("constrain", k): 8 * ct + 2, ("decide", k): 4 * ct + 8, ("finalize", k): 8})
        ts = {name: [] for name in cases}
        for rnd in range(WARM + REPS):
            for name, fn in cases.items():      # constrain before decide before finalize: real inputs
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                e.record()
                e.synchronize()
                if rnd >= WARM:
                    ts[name].append(a.elapsed_time(e))
        for name in cases:
            t = np.asarray(ts[name])
            total = bytes_px[name] * H * W
            print(f"{dataset + ' ' + name[0] + f', {name[1]} boxes':<34} {np.median(t):8.4f} {t.min():8.4f} "
                  f"{bytes_px[name]:8d} {total / 1e6:8.1f} {total / (np.median(t) * 1e-3) / 1e9:8.1f}")
        ctx.close()
        del probs, q, cases
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
