"""Cost of the boundary-band confusion (csrc/boundary.hip) beside seg_confusion, on the GPU.

seg_band_confusion at the workload's label size, 4 x 1024 x 2048 with nc = 20 and ignore = 19, for
the widths 1 2 4 8 and 1 2 4 8 16 32 64, and seg_confusion on the same tensors. The labels are
seeded 32 x 32 patches (input_pipelines/synthetic.pixel_labels), the decisions the labels with 30 %
of the pixels replaced by a random class. Device events, alternating rounds in one process, medians
and minima of REPS rounds after WARM warm-up rounds (the protocol of tools/crf_table.py). Beside
each time the share of the pixels in the widest band: only those read their label and decision
again and add a count.

    python tools/boundary_band.py > profiles/boundary_band.txt"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")]

WARM, REPS = 5, 30
N, H, W, NC = 4, 1024, 2048, 20
WIDTH_SETS = ([1, 2, 4, 8], [1, 2, 4, 8, 16, 32, 64])


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("boundary_band.py measures on the GPU; none is visible")
    from input_pipelines.synthetic import pixel_labels
    from seg_hip import SegContext
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    lab = pixel_labels(rng, N, H, W, n_classes=NC)
    dec = np.where(rng.random(lab.shape) < 0.3, rng.integers(0, NC, lab.shape), lab).astype(np.int32)
    labels, decisions = torch.from_numpy(lab).to(dev), torch.from_numpy(dec).to(dev)
    # a small context: the entries take their size from their arguments
    ctx = SegContext(pyramid="none", height=64, width=128, nb_pp=1, dtype="bf16")
    print(f"# {torch.cuda.get_device_name(0)}; seg_band_confusion and seg_confusion at {N} x {H} x {W}, nc = {NC}, "
          f"ignore = {NC - 1}; device events, alternating rounds, medians of {REPS} after {WARM} warm-up rounds")
    print(f"{'case':<46} {'ms':>8} {'min ms':>8} {'in widest band':>15}")
    whole = torch.empty((NC, NC), dtype=torch.int32, device=dev)
    cases = {"seg_confusion": lambda: ctx.confusion(labels, decisions, NC, whole)}
    outs, share = {}, {"seg_confusion": float("nan")}
    for widths in WIDTH_SETS:
        name = "seg_band_confusion, widths " + " ".join(str(w) for w in widths)
        outs[name] = torch.empty((len(widths), NC, NC), dtype=torch.int32, device=dev)
        cases[name] = lambda widths=widths, name=name: ctx.band_confusion(labels, decisions, NC, NC - 1, widths, outs[name])
    ts = {name: [] for name in cases}
    for rnd in range(WARM + REPS):
        for name, fn in cases.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            e.synchronize()
            if rnd >= WARM:
                ts[name].append(a.elapsed_time(e))
    total = int(whole.sum())
    for name, out in outs.items():
        cm = out.cpu().numpy().astype(np.int64)
        assert (np.diff(cm, axis=0) >= 0).all() and (cm[-1] <= whole.cpu().numpy()).all()
        share[name] = cm[-1].sum() / total
    for name in cases:
        t = np.asarray(ts[name])
        print(f"{name:<46} {np.median(t):8.4f} {t.min():8.4f} {share[name]:15.4f}")
    ctx.close()


if __name__ == "__main__":
    main()
