"""Host side of the blur stage of the training augmentation (input_pipelines/augment.py): the
draws of random_blur, their independence from the other stages' draws, the record layout, the
train.py flag, and self-checks of the numpy restatement the GPU tests compare with
(tests/blur_ref.py)."""
import os
import re

import numpy as np
import pytest

import blur_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _draw(seed, n, H, W, **kw):
    from input_pipelines.augment import draw_params
    return draw_params(np.random.default_rng(seed), n, H, W, blur=True,
                       blur_rng=np.random.default_rng([seed, 1]), **kw)


@pytest.mark.parametrize("H,W,ks,sigma", [(512, 1024, {3, 5}, 38.0), (1024, 2048, {3, 5, 7, 9}, 77.0)])
def test_blur_draw_distribution(H, W, ks, sigma):
    from input_pipelines.augment import draw_params
    rng, brng = np.random.default_rng(0), np.random.default_rng(1)
    modes, seen = [], set()
    for _ in range(200):
        p = draw_params(rng, 6, H, W, blur=True, blur_rng=brng)
        assert len(set(p["blur"]["mode"])) == 1          # one selector per batch
        mode = int(p["blur"]["mode"][0])
        modes.append(mode)
        if mode == 0:   # all-zero words: the record of a caller that knows no blur
            assert not p["blur"]["ksize"].any() and not p["blur"]["sigma"].any()
            continue
        seen |= set(int(k) for k in p["blur"]["ksize"])
        assert np.all(p["blur"]["sigma"] == (sigma if mode == 2 else 0.0))
    assert seen == ks
    share = np.bincount(modes, minlength=3) / len(modes)
    # selector ~ integers(0, 4): 0 median, 1 bilateral, 2 and 3 none; 200 draws, > 4 sigma slack
    assert abs(share[0] - 0.5) < 0.15 and abs(share[1] - 0.25) < 0.13 and abs(share[2] - 0.25) < 0.13


def test_blur_draw_limits():
    from input_pipelines.augment import blur_draw_range, draw_params, off_params
    assert blur_draw_range(512, 1024) == (2, 38.0) and blur_draw_range(1024, 2048) == (4, 77.0)
    assert blur_draw_range(1, 2214285)[0] == 4         # 1.4 * (res + 1) <= 4.5
    with pytest.raises(ValueError, match="kernel sizes"):
        blur_draw_range(1, 2214287)
    with pytest.raises(ValueError, match="kernel sizes"):
        _draw(0, 2, 1200, 2400)
    with pytest.raises(ValueError, match="blur_rng"):
        draw_params(np.random.default_rng(0), 2, 64, 128, blur=True)
    # blur off: the size is not looked at, nothing is drawn, the words stay zero
    p = draw_params(np.random.default_rng(0), 2, 1200, 2400)
    assert p.tobytes() == off_params(2, 1200, 2400).tobytes()
    assert not off_params(3, 64, 128)["blur"]["mode"].any()


def test_blur_overrides():
    p = _draw(3, 4, 64, 128, blur_mode=2, blur_ksize=[3, 5, 7, 9])
    assert list(p["blur"]["mode"]) == [2] * 4 and list(p["blur"]["ksize"]) == [3, 5, 7, 9]
    assert np.all(p["blur"]["sigma"] == 25.0)
    p = _draw(3, 4, 64, 128, blur_mode=[0, 1, 0, 1], blur_ksize=5)
    assert list(p["blur"]["ksize"]) == [0, 5, 0, 5] and not p["blur"]["sigma"].any()


def test_blur_draws_leave_the_other_draws_alone():
    """The blur draws come from their own generator: colour, flip and scale fields are those
    drawn with blur off, and the main generator is left in the same state."""
    from input_pipelines.augment import draw_params
    kw = dict(color=True, flip=True, scale_poi=[1.0, 2.0], void_cid=19)
    ra, rb = np.random.default_rng(5), np.random.default_rng(5)
    brng = np.random.default_rng(9)
    blurred = 0
    for _ in range(8):
        a = draw_params(ra, 4, 512, 1024, **kw)
        b = draw_params(rb, 4, 512, 1024, blur=True, blur_rng=brng, **kw)
        blurred += int(b["blur"]["mode"].any())
        for name in a.dtype.names:
            if name != "blur":
                assert np.array_equal(a[name], b[name]), name
    assert blurred > 0
    assert ra.integers(0, 1 << 30) == rb.integers(0, 1 << 30)


def test_blur_record_layout():
    from input_pipelines.augment import AUG_DTYPE, AUG_PARAMS_BYTES
    assert AUG_DTYPE.itemsize == AUG_PARAMS_BYTES == 64
    # the record's last field is the 12-byte blur sub-record: mode, ksize, sigma at 52, 56, 60
    blur, base = AUG_DTYPE.fields["blur"][:2]
    assert AUG_DTYPE.names[-1] == "blur" and base == 52 and blur.itemsize == 12
    assert blur.names == ("mode", "ksize", "sigma")
    assert [base + blur.fields[n][1] for n in blur.names] == [52, 56, 60]
    assert [blur.fields[n][0] for n in blur.names] == [np.dtype(np.int32), np.dtype(np.int32),
                                                       np.dtype(np.float32)]
    p = np.zeros(1, AUG_DTYPE)
    p["blur"]["mode"], p["blur"]["ksize"], p["blur"]["sigma"] = 2, 9, 77.0
    assert p.view(np.int32).reshape(16)[13:15].tolist() == [2, 9]
    assert p.view(np.float32).reshape(16)[15] == 77.0 and not p.view(np.int32).reshape(16)[:13].any()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "seg_hip.h")).read()
    sub = re.search(r"typedef struct seg_aug_blur \{(.*?)\} seg_aug_blur;", hdr, re.S).group(1)
    assert re.search(r"int32_t mode, ksize;\s*float sigma;\s*$", re.sub(r"/\*.*?\*/", "", sub, flags=re.S))
    body = re.search(r"typedef struct seg_aug_params \{(.*?)\} seg_aug_params;", hdr, re.S).group(1)
    assert re.search(r"int32_t void_cid;\s*seg_aug_blur blur;\s*$", body)


def test_blur_flag_parses_and_defaults_off():
    import train
    from estimator.mode_keys import ModeKeys
    from utils.utils import SemanticSegmentationArguments
    a = SemanticSegmentationArguments(mode=ModeKeys.TRAIN)
    train.add_train_input_pipeline_arguments(a.argparser)
    assert a.parse_args(["logs", "cityscapes"]).augment_blur is False
    s = a.parse_args(["logs", "cityscapes", "--augment_color", "--augment_blur", "--augment_flip",
                      "--augment_scale", "1.0", "2.0"])
    assert s.augment_blur is True and s.augment_color is True and s.augment_flip is True


def test_blur_generators_leave_the_existing_streams_alone():
    """default_rng([seed, s, rank, 3]) is a stream of its own: drawing from it changes nothing
    that [seed, s, rank, 2] gives."""
    from input_pipelines.augment import draw_params
    kw = dict(color=True, flip=True, scale_poi=[1.0, 2.0])
    seed, rank = 3, 0
    for s in range(3):
        a = np.random.default_rng([seed, s, rank, 2])
        b = np.random.default_rng([seed, s, rank, 2])
        br = np.random.default_rng([seed, s, rank, 3])
        for _ in range(4):
            x = draw_params(a, 2, 64, 128, **kw)
            y = draw_params(b, 2, 64, 128, blur=True, blur_rng=br, **kw)
            y["blur"]["mode"] = y["blur"]["ksize"] = 0
            y["blur"]["sigma"] = 0
            assert x.tobytes() == y.tobytes()


# ---- the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_median_restatement_is_scipy_median_filter(k):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(k)
    for shape in [(5, 7), (37, 53)]:
        q = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        q[: shape[0] // 2] = q[: shape[0] // 2] // 64 * 64          # ties
        x = (q.astype(np.float64) + 0.5) / 255.0                    # trunc(x * 255) = q
        got = blur_ref.median(x, k, np.float64)
        ref = ndimage.median_filter(q, size=(k, k, 1), mode="nearest")
        np.testing.assert_array_equal(got, ref.astype(np.float64) / 255.0)
        got32 = blur_ref.median(x.astype(np.float32), k, np.float32)
        np.testing.assert_array_equal(got32, ref.astype(np.float32) / np.float32(255))


def test_median_truncates_at_255():
    """q = trunc(x * 255), not the flip stage's 255.5: 0.999 is 254."""
    x = np.full((3, 3, 3), 0.999, np.float32)
    assert np.all(blur_ref.median(x, 3) == np.float32(254) / np.float32(255))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bilateral_constant_image(dtype):
    x = np.full((6, 9, 3), 0.37, dtype) * np.asarray([1.0, 0.5, 2.0], dtype)
    for k in (3, 9):
        for sigma in (38.0, 0.1):
            out = blur_ref.bilateral(x, k, np.float32(sigma), dtype)
            assert out.dtype == dtype
            np.testing.assert_allclose(out, x, atol=1e-6, rtol=0)


def test_bilateral_one_hot_spreads_to_the_disc():
    """k = 3: r = 1, the taps are the centre and its 4-neighbours. A one-hot pixel of height h
    therefore reaches exactly those 5 pixels: at a neighbour the tap on the hot pixel weighs
    s * c with s = exp(-1 / (2 sigma^2)), c = exp(-h^2 / (2 sigma^2)) (L1 distance h: one channel
    differs), and the four other taps see zeros."""
    sigma, h = 0.5, 0.8
    x = np.zeros((7, 7, 3))
    x[3, 3, 1] = h
    out = blur_ref.bilateral(x, 3, sigma, np.float64)
    s, c = np.exp(-1.0 / (2 * sigma ** 2)), np.exp(-h * h / (2 * sigma ** 2))
    expect = np.zeros_like(x)
    expect[3, 3, 1] = h / (1.0 + 4 * s * c)                 # centre: itself + four zero taps
    for y, xx in [(2, 3), (4, 3), (3, 2), (3, 4)]:
        expect[y, xx, 1] = h * s * c / (1.0 + 3 * s + s * c)   # own tap 1, three zero neighbours s
    np.testing.assert_allclose(out, expect, atol=1e-12, rtol=0)
    assert np.count_nonzero(out) == 5 and out[2, 2, 1] == 0.0   # the diagonal is off the disc


def test_bilateral_reflect101_corner():
    """k = 3 at pixel (0, 0): the taps (-1, 0) and (0, -1) read rows / columns 1 (reflect-101:
    -1 -> 1, not 0), so the corner sees a = x[0, 0] once and b = x[1, 0], c = x[0, 1] twice."""
    sigma = 0.3
    x = np.zeros((4, 5, 3))
    a, b, c = 0.2, 0.5, 0.9
    x[0, 0], x[1, 0], x[0, 1] = a, b, c
    out = blur_ref.bilateral(x, 3, sigma, np.float64)
    s = np.exp(-1.0 / (2 * sigma ** 2))
    wb = s * np.exp(-(3 * (b - a)) ** 2 / (2 * sigma ** 2))   # L1 over three equal channels
    wc = s * np.exp(-(3 * (c - a)) ** 2 / (2 * sigma ** 2))
    expect = (a + 2 * wb * b + 2 * wc * c) / (1 + 2 * wb + 2 * wc)
    np.testing.assert_allclose(out[0, 0], expect, atol=1e-12, rtol=0)
    # the far corner (3, 4): index n maps to n - 2
    x = np.zeros((4, 5, 3))
    x[3, 4], x[2, 4], x[3, 3] = a, b, c
    out = blur_ref.bilateral(x, 3, sigma, np.float64)
    np.testing.assert_allclose(out[3, 4], expect, atol=1e-12, rtol=0)


def test_chain_reference_shares_are_those_on_file():
    """profiles/augment_blur_margins.txt is what tools/aug_blur_margins.py writes for the chain
    cases of blur_ref: non-zero but small shares for the seeds in use."""
    path = os.path.join(os.path.dirname(HERE), "profiles", "augment_blur_margins.txt")
    rows = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    assert len(rows) == len(blur_ref.CHAIN_MODES) * len(blur_ref.CHAIN_SHAPES)
    for mode, shape, seed, bound, share in rows:
        H, W = (int(v) for v in shape.split("x"))
        assert int(seed) == blur_ref.CHAIN_SEEDS[(mode, H)]
        assert 0.0 < float(share) < 5e-3
    # one case recomputed: the smallest, a median (no exp, whose last bit may depend on the host's
    # vector units); a share is a count of elements, so a host that rounds alike gives the
    # figure on file
    mode, shape, seed, bound, share = rows[0]
    H, W = (int(v) for v in shape.split("x"))
    got = blur_ref.chain_reference(mode, H, W)
    assert mode == "median"
    assert got[4] == pytest.approx(float(share), rel=1e-5)
    assert got[2] == pytest.approx(float(bound), rel=1e-5)
