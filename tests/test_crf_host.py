"""CPU tests of the mean-field CRF refinement: the flags of evaluate.py / predict.py, the
neighbourhood order and the host tables against the header's text, properties of the reference
(tests/crf_ref.py), and the precondition of the GPU parity test (tests/test_gpu_crf.py): on the
inputs and cases that test uses, the reference at float32 and at float64 disagree on at most 1e-3
of the per-head decisions (the project's near-tie cap; measured 0) and by at most 1e-5
norm-relative on Q^T (measured <= 4.9e-7), so a kernel that misses its bounds against float64
cannot blame the number format."""
import argparse
import importlib.util
import math
import os

import numpy as np
import pytest

import crf_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")
PROBLEM = os.path.join(PKG, "problem_definitions", "cityscapes", "problem01.json")

DATASETS = ["cityscapes", "vistas"]
ALL_CASES = [("synthetic", c) for c in crf_ref.CASES] + [("tiny", crf_ref.TINY_CASE)]


def _script(name):
    spec = importlib.util.spec_from_file_location(f"seg_{name}_crf_host", os.path.join(PKG, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_module_imports_without_gpu_or_library():
    """estimator/crf.py pulls in neither torch nor seg_hip at import."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import estimator.crf as c; "
            "assert 'seg_hip' not in sys.modules and 'torch' not in sys.modules; "
            "print(len(c.offsets(3, 1)))" % PKG)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "48"


# ---- the flags --------------------------------------------------------------------------------

def _ns(**kw):
    return argparse.Namespace(**kw)


def test_settings_defaults_and_off():
    from estimator.crf import CRFSettings, crf_settings
    assert crf_settings(_ns()) is None                       # no flag at all
    assert crf_settings(_ns(crf_iterations=0, crf_radius=2)) is None
    assert crf_settings(_ns(crf_iterations=5)) == CRFSettings(5, 3, 1, 4.0, 3.0, 67.0, 3.0, 3.0)
    st = crf_settings(_ns(crf_iterations=2, crf_radius=5, crf_dilation=4, crf_weights=[0, 1.5],
                          crf_thetas=[10, 2.5, 1]))
    assert st == CRFSettings(2, 5, 4, 0.0, 1.5, 10.0, 2.5, 1.0)


@pytest.mark.parametrize("kw,flag", [
    (dict(crf_iterations=-1), "--crf_iterations"),
    (dict(crf_iterations=33), "--crf_iterations"),
    (dict(crf_iterations=1.5), "--crf_iterations"),
    (dict(crf_iterations=2, crf_radius=0), "--crf_radius"),
    (dict(crf_iterations=2, crf_radius=6), "--crf_radius"),
    (dict(crf_iterations=2, crf_dilation=0), "--crf_dilation"),
    (dict(crf_iterations=2, crf_dilation=5), "--crf_dilation"),
    (dict(crf_iterations=2, crf_weights=[-0.1, 3]), "--crf_weights"),
    (dict(crf_iterations=2, crf_weights=[4, float("nan")]), "--crf_weights"),
    (dict(crf_iterations=2, crf_weights=[4]), "--crf_weights"),
    (dict(crf_iterations=2, crf_thetas=[67, 0, 3]), "--crf_thetas"),
    (dict(crf_iterations=2, crf_thetas=[67, 3, -1]), "--crf_thetas"),
    (dict(crf_iterations=2, crf_thetas=[float("inf"), 3, 3]), "--crf_thetas"),
    (dict(crf_iterations=2, crf_thetas=[67, 3]), "--crf_thetas"),
    # a bad value is refused even while the refinement is off
    (dict(crf_iterations=0, crf_radius=9), "--crf_radius"),
])
def test_settings_refusals_name_the_flag(kw, flag):
    from estimator.crf import crf_settings
    with pytest.raises(ValueError) as e:
        crf_settings(_ns(**kw))
    assert flag in str(e.value)


@pytest.mark.parametrize("script", ["evaluate", "predict"])
def test_scripts_take_the_flags(script, tmp_path):
    from estimator.crf import CRFSettings, crf_settings
    mod = _script(script)
    pos = ([str(tmp_path), "2", PROBLEM, "cityscapes"] if script == "evaluate"
           else [str(tmp_path), PROBLEM, str(tmp_path), "cityscapes"])
    parser = mod.build_arguments().argparser
    a = parser.parse_args(pos)
    assert a.crf_iterations == 0 and crf_settings(a) is None
    assert (a.crf_radius, a.crf_dilation, a.crf_weights, a.crf_thetas) == (3, 1, [4.0, 3.0], [67.0, 3.0, 3.0])
    a = parser.parse_args(pos + ["--crf_iterations", "5", "--crf_radius", "2", "--crf_dilation", "3",
                                 "--crf_weights", "1", "2", "--crf_thetas", "30", "4", "5"])
    assert crf_settings(a) == CRFSettings(5, 2, 3, 1.0, 2.0, 30.0, 4.0, 5.0)


@pytest.mark.parametrize("script", ["evaluate", "predict"])
def test_scripts_refuse_a_bad_value_before_anything_is_built(script, tmp_path):
    mod = _script(script)
    pos = ([str(tmp_path), "2", PROBLEM, "cityscapes"] if script == "evaluate"
           else [str(tmp_path), PROBLEM, str(tmp_path), "cityscapes"])
    with pytest.raises(ValueError, match="--crf_radius"):
        mod.main(pos + ["--crf_iterations", "2", "--crf_radius", "7"])


# ---- the neighbourhood and the tables against the header's text ------------------------------

@pytest.mark.parametrize("r,d", [(1, 1), (3, 1), (2, 3), (5, 4)])
def test_offset_order_and_tables(r, d):
    from estimator.crf import offsets
    offs = offsets(r, d)
    assert offs == crf_ref.offsets(r, d)
    assert len(offs) == (2 * r + 1) ** 2 - 1 and (0, 0) not in offs
    assert offs[0] == (-r * d, -r * d) and offs[1] == (-r * d, (-r + 1) * d) and offs[-1] == (r * d, r * d)
    assert offs == sorted(offs)                                    # row-major (dy, dx)
    assert all(oy % d == 0 and ox % d == 0 for oy, ox in offs)
    ga, gs, inv2b = crf_ref.tables(r, d)
    assert ga.dtype == gs.dtype == np.float32 and ga.shape == gs.shape == (len(offs),)
    for o, (oy, ox) in enumerate(offs):                            # the header's formulas, one by one
        o2 = float(oy * oy + ox * ox)
        assert ga[o] == np.float32(4.0 * math.exp(-o2 / (2.0 * 67.0 ** 2)))
        assert gs[o] == np.float32(3.0 * math.exp(-o2 / (2.0 * 3.0 ** 2)))
    assert inv2b == np.float32(1.0 / (2.0 * (3.0 * 2.0 / 255.0) ** 2))
    # one grey level is 2 / 255 in the prepared image: a difference of theta_beta levels in one
    # channel gives exp(-1/2)
    step = 3.0 * 2.0 / 255.0
    assert abs(math.exp(-(step * step) * float(inv2b)) - math.exp(-0.5)) < 1e-6


def test_synthetic_inputs_are_what_the_tests_expect():
    for ds in DATASETS:
        P, I = crf_ref.synthetic_inputs(ds)
        ct = sum(crf_ref.WIDTHS[ds])
        assert P.shape == (2, 37, 45, ct) and I.shape == (2, 37, 45, 3)
        assert P.dtype == I.dtype == np.float32
        assert I.min() >= -1.0 and I.max() <= 1.0   # level 255 is 1.0
        levels = (I.astype(np.float64) + 1.0) * 127.5
        assert np.abs(levels - np.round(levels)).max() < 1e-4      # on the 256 levels
        lo = 0
        for c in crf_ref.WIDTHS[ds]:
            np.testing.assert_allclose(P[..., lo:lo + c].sum(-1), 1.0, atol=1e-5)
            lo += c
        Pt, It = crf_ref.tiny_inputs(ds)
        assert Pt.shape == (1, 5, 3, ct) and It.shape == (1, 5, 3, 3)
        P2, _ = crf_ref.two_seed_inputs(ds)
        assert P2.shape == (2, 64, 128, ct) and not np.array_equal(P2[0], P2[1])


# ---- properties of the reference, and the GPU test's precondition ----------------------------

@pytest.mark.parametrize("dataset", DATASETS)
@pytest.mark.parametrize("which,case", ALL_CASES)
def test_float32_share_and_properties(dataset, which, case):
    widths = crf_ref.WIDTHS[dataset]
    P = (crf_ref.synthetic_inputs if which == "synthetic" else crf_ref.tiny_inputs)(dataset)[0]
    q64 = crf_ref.reference(dataset, case, np.float64, which)
    q32 = crf_ref.reference(dataset, case, np.float32, which)
    assert q64.dtype == np.float64 and q32.dtype == np.float32
    rel = crf_ref.rel(q32, q64)
    a64, a32 = crf_ref.head_argmax(q64, widths), crf_ref.head_argmax(q32, widths)
    share = float(np.mean(a64 != a32))
    moved = float(np.mean(a64[..., 0] != crf_ref.head_argmax(P, widths)[..., 0]))
    print(f"{dataset} {which} (r, d, T) = {case}: float32 vs float64 Q^T {rel:.2e} norm-relative, "
          f"per-head decisions differ on {share:.2e}; the l1 argmax of Q^T differs from P's on {moved:.3f}")
    assert rel <= 1e-5
    assert share <= 1e-3
    if which == "synthetic":
        assert moved > 0.01          # the refinement changes decisions: the comparison has content
    # Q^T is a distribution per head
    assert q64.min() >= 0.0 and q64.max() <= 1.0
    lo = 0
    for c in widths:
        np.testing.assert_allclose(q64[..., lo:lo + c].sum(-1), 1.0, atol=1e-5)
        lo += c


@pytest.mark.parametrize("dataset", DATASETS)
def test_zero_weights_keep_the_argmax(dataset):
    """w_a = w_s = 0: the message is 0, v = P, Q = P / sum P: the per-head argmax is P's."""
    widths = crf_ref.WIDTHS[dataset]
    P, I = crf_ref.synthetic_inputs(dataset)
    for dtype in (np.float64, np.float32):
        q = crf_ref.mean_field(P, I, 3, 1, 3, weights=(0.0, 0.0), widths=widths, dtype=dtype)
        np.testing.assert_array_equal(crf_ref.head_argmax(q, widths), crf_ref.head_argmax(P, widths))
        np.testing.assert_allclose(q, P, rtol=0, atol=1e-6)


def test_iterations_zero_is_the_input():
    P, I = crf_ref.synthetic_inputs("cityscapes")
    np.testing.assert_array_equal(crf_ref.mean_field(P, I, 3, 1, 0, dtype=np.float32), P)


def test_outside_neighbours_contribute_nothing():
    """One pixel: every neighbour is outside, the message is 0 and Q = P / sum P. A 1 x 2 image
    at r = 1: exactly one neighbour each, k known in closed form."""
    P = np.array([[[[0.2, 0.8] + [1.0] + [1.0]]]], dtype=np.float32)
    I = np.zeros((1, 1, 1, 3), dtype=np.float32)
    q = crf_ref.mean_field(P, I, 5, 4, 2, widths=(2, 1, 1))
    np.testing.assert_allclose(q, P.astype(np.float64), atol=1e-12)
    P = np.array([[[[0.5, 0.5, 1.0, 1.0], [0.9, 0.1, 1.0, 1.0]]]], dtype=np.float32)
    I = np.zeros((1, 1, 2, 3), dtype=np.float32)
    q = crf_ref.mean_field(P, I, 1, 1, 1, widths=(2, 1, 1))
    ga, gs, _ = crf_ref.tables(1, 1)
    k = float(ga[3]) + float(gs[3])                   # offset (0, -1) is index 3, (0, 1) index 4
    assert crf_ref.offsets(1, 1)[3] == (0, -1) and ga[3] == ga[4]
    m = k * P[0, 0, 1, :2].astype(np.float64)         # pixel 0 hears pixel 1
    v = 0.5 * np.exp(m - m.max())
    np.testing.assert_allclose(q[0, 0, 0, :2], v / v.sum(), rtol=1e-12)
