"""Reference margins of the blur chain test (tests/test_gpu_blur.py::test_chain), on the CPU.

For each chain case of tests/blur_ref.py (colour + blur + flip + scaling up and down) the colour
stage is only toleranced, and the quantisations after it (the median's trunc(x * 255), the flip
stage's uint8 round trip) turn a rounding-level difference into a whole uint8 level now and
then. The table gives, per case, the colour bound (4 x the float32 restatement's error against
float64, centred units) and the share of elements by which the float32 chain restatement itself
is further than that bound from the float64 chain. The GPU test caps the kernels' share at 4 x
this figure, so the seeds in blur_ref.CHAIN_SEEDS are chosen for a non-zero but small share.

    python tools/aug_blur_margins.py > profiles/augment_blur_margins.txt
    python tools/aug_blur_margins.py --scan 8     # shares of seeds 0..7, to choose from"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"),
                os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")]


def main():
    import blur_ref
    scan = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--scan" else 0
    print("# chain cases of tests/blur_ref.py: float32 restatement against float64")
    print("# mode shape seed colour_bound share_over_bound")
    for mode in blur_ref.CHAIN_MODES:
        for H, W in blur_ref.CHAIN_SHAPES:
            for seed in (range(scan) if scan else [blur_ref.CHAIN_SEEDS[(mode, H)]]):
                _, _, bound, _, share = blur_ref.chain_reference(mode, H, W, seed)
                print(f"{mode} {H}x{W} {seed} {bound:.6e} {share:.6e}")


if __name__ == "__main__":
    main()
