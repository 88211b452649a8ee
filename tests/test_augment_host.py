"""Host side of the training augmentation (input_pipelines/augment.py): the parameter draws,
the train.py flags, the independence of the augmentation generators from the existing shuffle /
crop-offset streams, and self-checks of the numpy restatement the GPU tests compare with
(tests/aug_ref.py)."""
import os
import re

import numpy as np
import pytest

import aug_ref

HERE = os.path.dirname(os.path.abspath(__file__))
L2C = [-1] * 7 + list(range(19)) + [-1] * 8


def test_params_struct_matches_the_c_record():
    from input_pipelines.augment import AUG_DTYPE, AUG_PARAMS_BYTES
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "seg_hip.h")).read()
    assert int(re.search(r"#define SEG_AUG_PARAMS_BYTES (\d+)", hdr).group(1)) == AUG_PARAMS_BYTES
    assert AUG_DTYPE.itemsize == AUG_PARAMS_BYTES == 64
    body = re.search(r"typedef struct seg_aug_params \{(.*?)\} seg_aug_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == list(AUG_DTYPE.names)
    # every field is 4 bytes, in declaration order, no holes
    assert [AUG_DTYPE.fields[n][1] for n in AUG_DTYPE.names] == [4 * i for i in range(13)] + [52]


@pytest.mark.parametrize("H,W", [(37, 53), (64, 128), (512, 1024)])
def test_draw_params_ranges_and_crops(H, W):
    from input_pipelines.augment import draw_params
    rng = np.random.default_rng(11)
    orders, modes, flips = set(), set(), set()
    f32 = np.float32
    for _ in range(60):
        p = draw_params(rng, 5, H, W, color=True, flip=True, scale_poi=[1.0, 2.0], void_cid=19)
        assert len(set(p["color_order"])) == 1 and -1 <= p["color_order"][0] <= 3
        orders.add(int(p["color_order"][0]))
        assert np.all(np.abs(p["brightness_delta"]) <= f32(32.0 / 255.0))
        assert np.all(np.abs(p["hue_delta"]) <= f32(0.1))
        for k in ("saturation_factor", "contrast_factor"):
            assert np.all((p[k] >= f32(0.7)) & (p[k] <= f32(1.3)))
        assert np.all(p["quantize"] == 1) and set(p["flip"]) <= {0, 1}
        flips |= set(int(v) for v in p["flip"])
        assert set(p["scale_mode"]) <= {1, 2} and np.all(p["void_cid"] == 19)
        modes |= set(int(v) for v in p["scale_mode"])
        # f in [1/2, 1]: sizes floor(f * H), crops inside the image
        assert np.all((p["sh"] >= H // 2) & (p["sh"] <= H) & (p["sw"] >= W // 2) & (p["sw"] <= W))
        up = p["scale_mode"] == 1
        assert np.all((p["oy"] >= 0) & (p["oy"] + p["sh"] <= H) & (p["ox"] >= 0) & (p["ox"] + p["sw"] <= W))
        assert np.all(p["oy"][~up] == 0) and np.all(p["ox"][~up] == 0)
    assert orders == {-1, 0, 1, 2, 3} and modes == {1, 2} and flips == {0, 1}


def test_draw_params_off_and_seeded():
    from input_pipelines.augment import draw_params, off_params
    p = draw_params(np.random.default_rng(0), 3, 64, 128, color=False, flip=False,
                    scale_poi=[1.0, 1.0], void_cid=19)
    assert p.tobytes() == off_params(3, 64, 128, 19).tobytes()
    assert np.all(p["scale_mode"] == 0) and np.all(p["color_order"] == -1)
    assert np.all(p["quantize"] == 0) and np.all(p["flip"] == 0)
    p = draw_params(np.random.default_rng(0), 3, 64, 128, color=True, flip=True, scale_poi=[1.0, 1.0])
    assert np.all(p["scale_mode"] == 0)
    kw = dict(color=True, flip=True, scale_poi=[1.0, 2.0], void_cid=19)
    a = draw_params(np.random.default_rng(5), 4, 64, 128, **kw)
    b = draw_params(np.random.default_rng(5), 4, 64, 128, **kw)
    c = draw_params(np.random.default_rng(6), 4, 64, 128, **kw)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()


def test_augment_flags_parse_and_default_off():
    import train
    from estimator.mode_keys import ModeKeys
    from utils.utils import SemanticSegmentationArguments
    a = SemanticSegmentationArguments(mode=ModeKeys.TRAIN)
    train.add_train_input_pipeline_arguments(a.argparser)
    s = a.parse_args(["logs", "cityscapes"])
    assert s.augment_color is False and s.augment_flip is False and s.augment_scale is None
    s = a.parse_args(["logs", "cityscapes", "--augment_color", "--augment_flip",
                      "--augment_scale", "1.0", "2.0"])
    assert s.augment_color is True and s.augment_flip is True and s.augment_scale == [1.0, 2.0]


def test_augmentation_generators_leave_the_existing_streams_alone():
    """The augmentation draws use default_rng([seed, s, rank, 2]): the shuffle ([seed, s, rank])
    and crop-offset ([seed, s, rank, 1]) generators give what they give without them."""
    from input_pipelines.augment import draw_params
    from input_pipelines.train_inputs import _weak_geometry, shuffled
    seed, rank = 3, 0

    def draws(with_aug):
        rngs = [np.random.default_rng([seed, s, rank]) for s in range(3)]
        geom = [np.random.default_rng([seed, s, rank, 1]) for s in range(3)]
        out = []
        if with_aug:
            aug = [np.random.default_rng([seed, s, rank, 2]) for s in range(3)]
        for k in range(6):
            if with_aug:
                for s in range(3):
                    draw_params(aug[s], 2, 64, 128, color=True, flip=True, scale_poi=[1.0, 2.0])
            out.append([_weak_geometry((300 + 7 * k, 400), 64, 128, geom[s]) for s in (1, 2)])
        its = [shuffled(list(range(50)), r, buffer=8) for r in rngs]
        out.append([[next(it) for _ in range(20)] for it in its])
        return out
    assert draws(False) == draws(True)


@pytest.mark.parametrize("src,dst", [((45, 70), (37, 53)), ((100, 200), (48, 64))])
def test_reference_identity_is_the_oracle_prepare(src, dst):
    from input_pipelines.augment import off_params
    from oracle.tfseg import prepare_images_np, prepare_labels_np
    rng = np.random.default_rng(sum(src))
    raw = rng.integers(0, 256, (2,) + src + (3,), dtype=np.uint8)
    lab = rng.integers(0, 34, (2,) + src, dtype=np.uint8)
    p = off_params(2, *dst, void_cid=19)
    out, fill = aug_ref.augment_images(raw, p, *dst, dtype=np.float32)
    assert out.dtype == np.float32 and not fill.any()
    np.testing.assert_array_equal(out, prepare_images_np(raw, *dst))
    np.testing.assert_array_equal(aug_ref.augment_labels(lab, p, *dst, L2C),
                                  prepare_labels_np(lab, *dst, L2C))
    rs, off = (dst[0] + 3, dst[1] + 7), (2, 5)      # a window of a larger resize
    out, _ = aug_ref.augment_images(raw, p, *dst, resized=rs, offset=off)
    np.testing.assert_array_equal(out, prepare_images_np(raw, *dst, resized=rs, offset=off))


def test_reference_hsv_round_trip():
    rng = np.random.default_rng(1)
    c = rng.random((64, 96, 3))
    c[:8] = np.round(c[:8] * 3) / 3          # ties between channels, zero range
    c[8:10] = 0.0                            # v = 0
    h, s, v = aug_ref.rgb_to_hsv(c, np.float64)
    assert h.min() >= 0.0 and h.max() < 1.0 and s.min() >= 0.0 and s.max() <= 1.0
    np.testing.assert_allclose(aug_ref.hsv_to_rgb(h, s, v, np.float64), c, atol=1e-6, rtol=0)


def test_reference_geometry_properties():
    """flip twice = identity; up-scaling the whole image of an already quantised image and
    down-scaling to the full size are the identity; the down-scale pad is the mean / void."""
    from input_pipelines.augment import off_params
    H, W = 37, 53
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)   # same size: values k / 255
    lab = rng.integers(0, 34, (1, H, W), dtype=np.uint8)
    base, _ = aug_ref.augment_images(raw, off_params(1, H, W), H, W)
    p = off_params(1, H, W, void_cid=19)
    p["flip"] = 1
    f, _ = aug_ref.augment_images(raw, p, H, W)
    np.testing.assert_array_equal(f, base[:, :, ::-1])
    np.testing.assert_array_equal(aug_ref.augment_labels(lab, p, H, W, L2C),
                                  aug_ref.augment_labels(lab, off_params(1, H, W), H, W, L2C)[:, :, ::-1])
    for mode in (1, 2):
        p = off_params(1, H, W, void_cid=19)
        p["scale_mode"] = mode
        o, fill = aug_ref.augment_images(raw, p, H, W)
        np.testing.assert_array_equal(o, base)
        assert not fill.any()
    p = off_params(1, H, W, void_cid=19)
    p["scale_mode"], p["sh"], p["sw"] = 2, 18, 26
    o, fill = aug_ref.augment_images(raw, p, H, W, dtype=np.float64)
    la = aug_ref.augment_labels(lab, p, H, W, L2C)
    assert fill[0, :9].all() and fill[0, 28:].all() and fill[0, :, :13].all() and fill[0, :, 40:].all()
    assert not fill[0, 9:27, 13:39].any() and np.all(la[0][fill[0]] == 19)
    inner = o[0, 9:27, 13:39]
    np.testing.assert_allclose(o[0][fill[0]], inner.mean(), atol=1e-12)
