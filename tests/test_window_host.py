"""CPU tests of sliding-window inference: the geometry rule, the flags of evaluate.py /
predict.py, and the precondition of the GPU decision tests (tests/test_gpu_window.py): on the
synthetic entries those tests use, the reference at float32 and at float64 disagree on at most
5e-4 of the pixels (the cap of tests/test_tta_host.py), so a kernel that misses the 1e-3 cap
against float64 cannot blame the number format."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

import window_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")
PROBLEM = os.path.join(PKG, "problem_definitions", "cityscapes", "problem01.json")


def _script(name):
    spec = importlib.util.spec_from_file_location(f"seg_{name}_window_host", os.path.join(PKG, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_module_imports_without_gpu_or_library():
    """estimator/windows.py pulls in neither torch nor seg_hip at import."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import estimator.windows as w; "
            "assert 'seg_hip' not in sys.modules and 'torch' not in sys.modules; "
            "print(w.window_origins(100, 64, 24))" % PKG)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "[0, 24, 36]"


def test_origins_known_answers():
    from estimator.windows import window_origins
    assert window_origins(100, 64, 24) == [0, 24, 36]
    assert window_origins(200, 128, 40) == [0, 40, 72]
    for s in (1, 17, 64):
        assert window_origins(64, 64, s) == [0]
    assert window_origins(1024, 512, 342) == [0, 342, 512]
    assert window_origins(2048, 1024, 683) == [0, 683, 1024]
    assert window_origins(128, 64, 64) == [0, 64]
    assert window_origins(65, 64, 64) == [0, 1]
    assert window_origins(70, 64, 1) == [0, 1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("C,n,s", [(100, 64, 24), (200, 128, 40), (64, 64, 5), (1024, 512, 342),
                                   (128, 64, 64), (129, 64, 64), (101, 37, 36), (53, 53, 53)])
def test_origins_rule_and_coverage(C, n, s):
    """The rule as the reference module writes it out, and what the library relies on: strictly
    increasing from 0, no gap, the last window flush with the edge."""
    from estimator.windows import window_origins
    o = window_origins(C, n, s)
    assert o == window_ref.origins(C, n, s)
    assert o[0] == 0 and o[-1] + n == C
    assert all(b > a and b <= a + n for a, b in zip(o, o[1:]))


def test_origins_reject_bad_arguments():
    from estimator.windows import window_origins
    with pytest.raises(ValueError):
        window_origins(63, 64, 24)       # the canvas is below the window
    with pytest.raises(ValueError):
        window_origins(100, 64, 0)       # no stride
    with pytest.raises(ValueError, match="gap"):
        window_origins(200, 64, 65)      # a stride above the window leaves a gap


def test_grid_entry_cap_names_count_canvas_and_stride():
    from estimator.windows import MAX_ENTRIES, window_grid
    assert MAX_ENTRIES == 64
    assert window_grid((100, 200), (64, 128), (24, 40), True) == ([0, 24, 36], [0, 40, 72])
    # 8 x 8 windows are 64 entries: allowed; with flip 128: refused
    ys, xs = window_grid((64 + 7 * 8, 128 + 7 * 8), (64, 128), (8, 8), False)
    assert len(ys) == len(xs) == 8
    with pytest.raises(ValueError) as e:
        window_grid((64 + 7 * 8, 128 + 7 * 8), (64, 128), (8, 8), True)
    msg = str(e.value)
    assert "128 entries" in msg and "120 x 184" in msg and "8 x 8" in msg and "64" in msg
    with pytest.raises(ValueError, match="65 entries"):
        window_grid((64 + 64, 128), (64, 128), (1, 1), False)


def test_settings_off_by_default_and_default_stride():
    from estimator.windows import default_stride, input_size, window_settings
    assert window_settings(argparse.Namespace()) is None
    base = dict(height_feature_extractor=512, width_feature_extractor=1024)
    assert window_settings(argparse.Namespace(window_canvas=None, window_stride=None, **base)) is None
    assert input_size(argparse.Namespace(**base)) == (512, 1024)
    assert default_stride(512, 1024) == (342, 683) == ((2 * 512 + 2) // 3, (2 * 1024 + 2) // 3)
    assert default_stride(64, 128) == (43, 86)
    s = argparse.Namespace(window_canvas=[1024, 2048], window_stride=None, **base)
    assert window_settings(s) == ((1024, 2048), (342, 683), False)
    assert input_size(s) == (1024, 2048)
    s = argparse.Namespace(window_canvas=[1024, 2048], window_stride=[256, 512], tta_flip=True, **base)
    assert window_settings(s) == ((1024, 2048), (256, 512), True)
    with pytest.raises(ValueError) as e:
        window_settings(argparse.Namespace(window_canvas=[1024, 2048], tta_scales=[0.5, 1.0], **base))
    assert "--tta_scales" in str(e.value) and "--window_canvas" in str(e.value)
    with pytest.raises(ValueError, match="--window_canvas"):
        window_settings(argparse.Namespace(window_canvas=None, window_stride=[8, 8], **base))


def test_evaluate_flags():
    ev = _script("evaluate")
    base = ["/tmp/log", "4", PROBLEM, "cityscapes"]
    a = ev.build_arguments().parse_args(base)
    assert a.window_canvas is None and a.window_stride is None
    a = ev.build_arguments().parse_args(base + ["--window_canvas", "1024", "2048", "--tta_flip"])
    assert a.window_canvas == [1024, 2048] and a.window_stride is None and a.tta_flip is True
    a = ev.build_arguments().parse_args(["--window_canvas", "72", "100", "--window_stride", "24", "36"] + base)
    assert a.window_canvas == [72, 100] and a.window_stride == [24, 36]
    with pytest.raises(SystemExit):
        ev.build_arguments().parse_args(base + ["--window_canvas", "1024"])
    with pytest.raises(ValueError) as e:     # refused at settings time, before anything is built
        ev.main(base + ["--window_canvas", "1024", "2048", "--tta_scales", "0.5", "1.0"])
    assert "--tta_scales" in str(e.value) and "--window_canvas" in str(e.value)


def test_predict_flags():
    pr = _script("predict")
    base = ["/tmp/log", PROBLEM, "/tmp/in", "cityscapes"]
    a = pr.build_arguments().parse_args(base)
    assert a.window_canvas is None and a.window_stride is None
    a = pr.build_arguments().parse_args(base + ["--window_canvas", "72", "100", "--window_stride", "24",
                                                 "36", "--tta_flip", "--replace_voids"])
    assert a.window_canvas == [72, 100] and a.window_stride == [24, 36] and a.tta_flip
    text = " ".join(pr.build_arguments().argparser.format_help().split())
    assert "--window_canvas HC WC" in text and "--window_stride SY SX" in text
    with pytest.raises(ValueError) as e:
        pr.main(base + ["--window_canvas", "72", "100", "--tta_scales", "1.0"])
    assert "--tta_scales" in str(e.value) and "--window_canvas" in str(e.value)


def test_synthetic_case_geometry():
    ys, xs = window_ref.synthetic_grid()
    assert (ys, xs) == ([0, 24, 36], [0, 40, 72])
    ents = window_ref.synthetic_entries("cityscapes", 1.0)
    assert len(ents) == 18 and ents[0].shape == (2, 8, 16, 24) and ents[0].dtype == np.float32
    assert window_ref.synthetic_entries("vistas", 3.0)[17].shape == (2, 8, 16, 70)
    _, _, count, _ = window_ref.synthetic_reference("cityscapes", 1.0, (100, 200), False, torch.float64)
    assert count.shape == (100, 200) and count.min() == 2 and count.max() == 18
    assert count[0, 0] == 2 and count[50, 100] == 18 and count[99, 199] == 2


@pytest.mark.parametrize("dataset", ["cityscapes", "vistas"])
@pytest.mark.parametrize("amplitude", [1.0, 3.0])
def test_reference_precondition_fp32_vs_fp64(dataset, amplitude):
    """Network 64 x 128, canvas 100 x 200, stride (24, 40), flip: 18 entries of 8 x 16 logits,
    N = 2. The float32 and float64 references agree on all but <= 5e-4 of the pixels in every
    decision mode the GPU test uses."""
    ct = sum(window_ref.WIDTHS[dataset])
    c1 = window_ref.WIDTHS[dataset][0]
    for rv in (False, True):
        for out_hw in ((100, 200), (45, 77)):
            p64, d64, _, stats = window_ref.synthetic_reference(dataset, amplitude, out_hw, rv, torch.float64)
            p32, d32, _, _ = window_ref.synthetic_reference(dataset, amplitude, out_hw, rv, torch.float32)
            share = float(np.mean(d64 != d32))
            rel = float(np.linalg.norm(p32.astype(np.float64) - p64) / np.linalg.norm(p64))
            print(f"{dataset} amplitude {amplitude} rv {rv} out {out_hw}: decisions differ on "
                  f"{share:.2e}, probabilities {rel:.2e} norm-relative, branches {stats}")
            assert d64.shape == (window_ref.BATCH,) + out_hw and p64.shape == (2, 100, 200, ct)
            assert share <= 5e-4
            assert rel <= 1e-6
            np.testing.assert_allclose(p64[..., :c1].sum(-1), 1.0, atol=1e-12)
            np.testing.assert_allclose(p64[..., c1:].sum(-1), 2.0, atol=1e-12)
