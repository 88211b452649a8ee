"""CPU tests of test-time augmentation: the size rule, the flags of evaluate.py / predict.py, and
the precondition of the GPU decision tests (tests/test_gpu_tta.py): on the synthetic logits those
tests use, the reference at float32 and at float64 disagree on at most 5e-4 of the pixels, so a
kernel that misses the 1e-3 cap against float64 cannot blame the number format."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import tta_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")
PROBLEM = os.path.join(PKG, "problem_definitions", "cityscapes", "problem01.json")


def _script(name):
    spec = importlib.util.spec_from_file_location(f"seg_{name}_tta_host", os.path.join(PKG, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_module_imports_without_gpu_or_library():
    """estimator/tta.py pulls in neither torch nor seg_hip at import."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import estimator.tta as t; "
            "assert 'seg_hip' not in sys.modules and 'torch' not in sys.modules; "
            "print(t.tta_sizes(64, 128, [1.0]))" % PKG)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "[(64, 128)]"


def test_sizes_scale_one_is_the_network_size():
    from estimator.tta import tta_sizes
    assert tta_sizes(64, 128, [1.0]) == [(64, 128)]
    assert tta_sizes(101, 103, [1.0]) == [(101, 103)]        # not rounded to a multiple of 8
    assert tta_sizes(1024, 2048, [1]) == [(1024, 2048)]


def test_sizes_rule():
    from estimator.tta import tta_sizes
    assert tta_sizes(64, 128, [0.75, 1.25]) == [(48, 96), (80, 160)]
    assert tta_sizes(64, 128, [0.75, 1.0, 1.25]) == [(48, 96), (64, 128), (80, 160)]
    # 8 * floor(s * n / 8 + 0.5): 1.3 * 101 / 8 = 16.41 -> 16 -> 128; 1.3 * 103 / 8 = 16.74 -> 17 -> 136
    assert tta_sizes(101, 103, [1.3]) == [(128, 136)]
    assert tta_sizes(1024, 2048, [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]) == [
        (512, 1024), (768, 1536), (1024, 2048), (1280, 2560), (1536, 3072), (1792, 3584), (2048, 4096)]


def test_sizes_floor_of_32():
    from estimator.tta import tta_sizes
    assert tta_sizes(64, 128, [0.25]) == [(32, 32)]
    assert tta_sizes(64, 128, [0.1]) == [(32, 32)]
    assert tta_sizes(48, 512, [0.5]) == [(32, 256)]


def test_sizes_reject_duplicates_naming_both_scales():
    from estimator.tta import tta_sizes
    with pytest.raises(ValueError) as e:
        tta_sizes(64, 128, [0.75, 1.0, 0.76])
    assert "0.75" in str(e.value) and "0.76" in str(e.value)
    with pytest.raises(ValueError) as e:      # 1.01 rounds to the network size, which 1.0 is
        tta_sizes(64, 128, [1.0, 1.01])
    assert "1.01" in str(e.value) and "and" in str(e.value)
    with pytest.raises(ValueError):
        tta_sizes(64, 128, [0.1, 0.25])       # both at the floor
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            tta_sizes(64, 128, [bad])


def test_settings_off_by_default():
    import argparse
    from estimator.tta import tta_settings
    assert tta_settings(argparse.Namespace()) is None
    assert tta_settings(argparse.Namespace(tta_scales=None, tta_flip=False)) is None
    assert tta_settings(argparse.Namespace(tta_scales=None, tta_flip=True)) == ((1.0,), True)
    assert tta_settings(argparse.Namespace(tta_scales=[0.5, 1], tta_flip=False)) == ((0.5, 1.0), False)


def test_evaluate_flags():
    ev = _script("evaluate")
    base = ["/tmp/log", "4", PROBLEM, "cityscapes"]
    a = ev.build_arguments().parse_args(base)
    assert a.tta_scales is None and a.tta_flip is False
    a = ev.build_arguments().parse_args(base + ["--tta_scales", "0.75", "1.0", "1.25", "--tta_flip",
                                                 "--eval_all_ckpts"])
    assert a.tta_scales == [0.75, 1.0, 1.25] and a.tta_flip is True and a.eval_all_ckpts
    a = ev.build_arguments().parse_args(["--tta_scales", "0.5", "--Nb", "2"] + base)
    assert a.tta_scales == [0.5] and a.Nb == 2
    with pytest.raises(SystemExit):
        ev.build_arguments().parse_args(base + ["--tta_scales"])


def test_predict_flags():
    pr = _script("predict")
    base = ["/tmp/log", PROBLEM, "/tmp/in", "cityscapes"]
    a = pr.build_arguments().parse_args(base)
    assert a.tta_scales is None and a.tta_flip is False
    a = pr.build_arguments().parse_args(base + ["--tta_flip", "--replace_voids"])
    assert a.tta_scales is None and a.tta_flip and a.replace_voids
    # a list flag in front of the positionals ends at the next flag, as for every nargs flag
    a = pr.build_arguments().parse_args(["--tta_scales", "1.0", "1.5", "--Nb", "1"] + base)
    assert a.tta_scales == [1.0, 1.5]
    # the replace_voids flag says which order test-time augmentation uses
    text = pr.build_arguments().argparser.format_help()
    assert "--tta_scales" in text and "averaged l1" in " ".join(text.split())


def test_image_reference_identities():
    """Equal sizes: the reference itself is a copy / a mirror (lerp weights exactly 0)."""
    x = np.random.default_rng(3).random((2, 9, 11, 3), dtype=np.float32) * 2 - 1
    np.testing.assert_array_equal(tta_ref.resize_images_ref(x, 9, 11, False, np.float32), x)
    np.testing.assert_array_equal(tta_ref.resize_images_ref(x, 9, 11, True, np.float32), x[:, :, ::-1])


@pytest.mark.parametrize("amplitude", [1.0, 3.0])
def test_reference_precondition_fp32_vs_fp64(amplitude):
    """10 entries, low sizes (4,8) (6,12) (8,16) (10,20) (13,13), each with and without flip, to
    64 x 128, N = 2, Cityscapes widths: float32 and float64 references agree on all but <= 5e-4
    of the pixels (measured: 0), in every decision mode the GPU test uses, and both l2 branches
    carry a real share of the pixels, so the fusion is exercised."""
    for rv in (False, True):
        for out_hw in ((64, 128), (45, 77)):
            p64, d64, stats = tta_ref.synthetic_reference("cityscapes", amplitude, (), out_hw, rv,
                                                          torch.float64)
            p32, d32, _ = tta_ref.synthetic_reference("cityscapes", amplitude, (), out_hw, rv,
                                                      torch.float32)
            share = float(np.mean(d64 != d32))
            rel = float(np.linalg.norm(p32.astype(np.float64) - p64) / np.linalg.norm(p64))
            print(f"amplitude {amplitude} rv {rv} out {out_hw}: decisions differ on {share:.2e}, "
                  f"probabilities {rel:.2e} norm-relative, branches {stats}")
            assert d64.shape == (tta_ref.BATCH,) + out_hw
            assert share <= 5e-4
            assert rel <= 1e-6
            assert stats["vehicle"] >= 0.02 and stats["human"] >= 0.02
            np.testing.assert_allclose(p64[..., :14].sum(-1), 1.0, atol=1e-12)
