"""The blur stage of the device-side training augmentation (csrc/augment.hip pass 2b through
seg_augment_images, input_pipelines/augment.py) against the numpy restatement tests/blur_ref.py:
the median bitwise, the bilateral filter against float64 within a bound measured from the
float32 restatement, the chain colour -> blur -> flip -> scaling, mixed batches, the rejected
records, determinism, and the train input / train.py wiring.

Shapes: 5 x 7 (the smallest at which the k = 9 reflect-101 border is defined), 37 x 53 (odd,
narrower than one 64-wide tile), 70 x 131 (three tile rows and columns with ragged edges)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import aug_ref
import blur_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "tiny_train")
VOID = 19
SHAPES = [(5, 7), (37, 53), (70, 131)]
KSIZES = [3, 5, 7, 9]


def _gpu(cuda, raw, p, H, W, **kw):
    from input_pipelines.augment import augment_images
    return augment_images(torch.from_numpy(raw).to(cuda), p, H, W, **kw).cpu().numpy()


def _prepare(cuda, raw, H, W):
    from input_pipelines.tfrecords import prepare_images
    return prepare_images(torch.from_numpy(raw).to(cuda), H, W).cpu().numpy()


def _blur_params(n, H, W, mode, k, sigma=0.0):
    from input_pipelines.augment import off_params
    p = off_params(n, H, W, void_cid=VOID)
    p["blur"]["mode"], p["blur"]["ksize"], p["blur"]["sigma"] = mode, k, sigma
    return p


# ---- 1. median, bitwise --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def median_inputs():
    """Per shape: uniform noise, a 4-level posterised image (many ties), a constant."""
    out = {}
    for H, W in SHAPES:
        noise = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
        out[(H, W)] = np.stack([noise, noise // 64 * 64, np.full((H, W, 3), 93, np.uint8)])
    return out


@pytest.mark.parametrize("k", KSIZES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_median_bitwise(cuda, median_inputs, H, W, k):
    raw = median_inputs[(H, W)]
    p = _blur_params(3, H, W, 1, k)
    got = _gpu(cuda, raw, p, H, W)
    ref, _ = blur_ref.augment_images_blur(raw, p, H, W, dtype=np.float32)
    assert np.array_equal(got, ref)
    if (H, W) != (5, 7):    # a window that covers all of 5 x 7 gives one value per channel
        assert not np.array_equal(got[0], _prepare(cuda, raw[:1], H, W)[0])
    assert np.array_equal(got[2], ref[2]) and np.all(got[2] == got[2].flat[0])


def test_median_bitwise_after_a_resize_and_with_the_flip_stage(cuda):
    """Values that are no multiple of 1 / 255 enter the median (a 45 x 70 raw image resized to
    37 x 53), a different k per image, and the flip stage's round trip follows."""
    H, W = 37, 53
    raw = np.random.default_rng(8).integers(0, 256, (4, 45, 70, 3), dtype=np.uint8)
    p = _blur_params(4, H, W, 1, KSIZES)
    p["quantize"], p["flip"] = 1, [0, 1, 0, 1]
    ref, _ = blur_ref.augment_images_blur(raw, p, H, W, dtype=np.float32)
    assert np.array_equal(_gpu(cuda, raw, p, H, W), ref)


# ---- 2. bilateral, toleranced --------------------------------------------------------------------
@pytest.fixture(scope="module")
def bilateral_inputs():
    """Per shape: noise and a step edge, each once per sigma (38 and 0.1)."""
    out = {}
    for H, W in SHAPES:
        noise = np.random.default_rng(100 + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
        step = np.empty((H, W, 3), np.uint8)
        step[:, : W // 2], step[:, W // 2:] = (40, 60, 80), (200, 180, 90)
        out[(H, W)] = np.stack([noise, noise, step, step])
    return out


@pytest.mark.parametrize("k", KSIZES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_bilateral_within_the_float32_bound(cuda, bilateral_inputs, H, W, k):
    """Colour and the flip stage off. Per element |gpu - ref64| <= 4 x the largest error of the
    float32 restatement against the float64 one over the case."""
    raw = bilateral_inputs[(H, W)]
    p = _blur_params(4, H, W, 2, k, [38.0, 0.1, 38.0, 0.1])
    r32, _ = blur_ref.augment_images_blur(raw, p, H, W, dtype=np.float32)
    r64, _ = blur_ref.augment_images_blur(raw, p, H, W, dtype=np.float64)
    bound = 4.0 * float(np.abs(r32 - r64).max())
    got = _gpu(cuda, raw, p, H, W)
    err = np.abs(got - r64).reshape(4, -1).max(1)
    print("bilateral", (H, W), "k", k, "bound", bound, "err per image", err)
    assert bound > 0.0
    assert np.all(err <= bound), (err, bound)
    plain = _prepare(cuda, raw, H, W)
    # sigma 38 on values in [0, 1] weighs every tap alike: the noise is smoothed, the step edge
    # bleeds; sigma 0.1 keeps the two sides of the edge apart (the colour term discriminates)
    assert np.abs(got[0] - plain[0]).max() > 0.1
    assert np.abs(got[3] - plain[3]).max() < 1e-3 < np.abs(got[2] - plain[2]).max()


# ---- 3. the chain --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_references():
    return {(mode, H): blur_ref.chain_reference(mode, H, W)
            for mode in blur_ref.CHAIN_MODES for H, W in blur_ref.CHAIN_SHAPES}


@pytest.mark.parametrize("mode", list(blur_ref.CHAIN_MODES))
@pytest.mark.parametrize("H,W", blur_ref.CHAIN_SHAPES)
def test_chain(cuda, chain_references, H, W, mode):
    """Colour on, blur, flip stage, scaling up (image 0) and down (image 1). The colour stage is
    only toleranced (bound: 4 x its float32 restatement's error, centred units), the median is
    1-Lipschitz in the sup norm and the quantisations move a value by at most one uint8 level,
    which is 2 / 255 of the centred output: every element is within one level plus the colour
    bound of the float64 chain, and the share of elements further than the colour bound from it
    is at most 4 x the share of the float32 chain restatement on the same inputs
    (profiles/augment_blur_margins.txt)."""
    raw, p, bound, r64, share32 = chain_references[(mode, H)]
    assert 0.0 < share32 < 5e-3
    d = np.abs(_gpu(cuda, raw, p, H, W) - r64)
    share = float((d > bound).mean())
    print("chain", mode, (H, W), "bound", bound, "share32", share32, "share", share, "max", float(d.max()))
    assert float(d.max()) <= 2.0 / 255.0 + bound
    assert share <= 4.0 * share32


# ---- 4. all-off and mixed batches ----------------------------------------------------------------
def test_mixed_batch_leaves_the_other_images_alone(cuda):
    from input_pipelines.augment import off_params
    H, W = 37, 53
    raw = np.random.default_rng(4).integers(0, 256, (3, 45, 70, 3), dtype=np.uint8)
    plain = _prepare(cuda, raw, H, W)
    assert np.array_equal(_gpu(cuda, raw, off_params(3, H, W, void_cid=VOID), H, W), plain)
    for mode, sigma in [(1, 0.0), (2, 38.0)]:
        p = _blur_params(3, H, W, [0, mode, 0], [0, 5, 0], [0.0, sigma, 0.0])
        got = _gpu(cuda, raw, p, H, W)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[2], plain[2])
        assert np.abs(got[1] - plain[1]).max() > 0.1
        if mode == 1:
            assert np.array_equal(got[1], blur_ref.augment_image_blur(raw[1], p[1], H, W)[0])
    # a blurred image beside one that only goes through the geometry pass: the two use the stage
    # and the output in opposite roles
    p = _blur_params(3, H, W, [1, 0, 1], [3, 0, 7])
    p["quantize"], p["flip"] = 1, [1, 1, 0]
    ref, _ = blur_ref.augment_images_blur(raw, p, H, W, dtype=np.float32)
    assert np.array_equal(_gpu(cuda, raw, p, H, W), ref)


def test_blur_in_the_second_chunk(cuda):
    """n = 33 exceeds AUG_MAX_CHUNK = 32: the blur of image 32 alone launches with the second
    chunk."""
    H, W = 37, 53
    raw = np.random.default_rng(5).integers(0, 256, (33, H, W, 3), dtype=np.uint8)
    p = _blur_params(33, H, W, [0] * 32 + [1], [0] * 32 + [5])
    got = _gpu(cuda, raw, p, H, W)
    assert np.array_equal(got[:32], _prepare(cuda, raw[:32], H, W))
    assert np.array_equal(got[32], blur_ref.augment_image_blur(raw[32], p[32], H, W)[0])
    assert not np.array_equal(got[32], _prepare(cuda, raw[32:], H, W)[0])


# ---- 5. rejected records -------------------------------------------------------------------------
def test_rejected_blur_records_launch_nothing(cuda):
    from input_pipelines.augment import augment_images, augment_labels
    from seg_hip import LIB
    s = torch.cuda.current_stream().cuda_stream

    def raw_call(H, W, p):
        """seg_augment_images on 2 images with the output pre-filled; (status, message, out)."""
        traw = torch.zeros((2, H, W, 3), dtype=torch.uint8, device=cuda)
        dev = torch.from_numpy(p.view(np.uint8).copy()).to(cuda)
        need = ctypes.c_int64(0)
        assert LIB.seg_augment_workspace(2, H, W, ctypes.byref(need)) == 0
        ws = torch.empty(need.value, dtype=torch.uint8, device=cuda)
        out = torch.full((2, H, W, 3), 7.0, dtype=torch.float32, device=cuda)
        rc = LIB.seg_augment_images(traw.data_ptr(), 2, H, W, H, W, 0, 0, H, W, p.ctypes.data,
                                    dev.data_ptr(), out.data_ptr(), ws.data_ptr(), need.value, s)
        msg = LIB.seg_last_error(None).decode() if rc else ""
        torch.cuda.synchronize()
        return rc, msg, out

    cases = [((37, 53), dict(mode=3, ksize=3), "blur.mode"),
             ((37, 53), dict(mode=-1, ksize=3), "blur.mode"),
             ((37, 53), dict(mode=1, ksize=4), "blur.ksize"),
             ((37, 53), dict(mode=1, ksize=11), "blur.ksize"),
             ((37, 53), dict(mode=2, ksize=1, sigma=38.0), "blur.ksize"),
             ((37, 53), dict(mode=2, ksize=5, sigma=0.0), "blur.sigma"),
             ((37, 53), dict(mode=2, ksize=5, sigma=-1.0), "blur.sigma"),
             ((37, 53), dict(mode=2, ksize=5, sigma=np.nan), "blur.sigma"),
             ((37, 53), dict(mode=2, ksize=5, sigma=np.inf), "blur.sigma"),
             ((4, 9), dict(mode=2, ksize=9, sigma=38.0), "min"),
             ((9, 4), dict(mode=2, ksize=9, sigma=38.0), "min")]
    for (H, W), fields, word in cases:
        p = _blur_params(2, H, W, 0, 0)
        for name, v in fields.items():
            p["blur"][name][1] = v            # image 0 is fine, image 1 is the bad record
        rc, msg, out = raw_call(H, W, p)
        assert rc == -22 and "image 1" in msg and word in msg, (fields, rc, msg)
        assert bool((out == 7.0).all()), fields
        with pytest.raises(RuntimeError, match="image 1.*" + word):
            augment_images(torch.zeros((2, H, W, 3), dtype=torch.uint8, device=cuda), p, H, W)
        with pytest.raises(RuntimeError, match="image 1.*" + word):
            augment_labels(torch.zeros((2, H, W), dtype=torch.uint8, device=cuda), p, H, W,
                           [-1] * 7 + list(range(19)) + [-1] * 8)
    # the neighbouring good records: median k = 9 needs no minimum size, bilateral k = 9 runs at 5 x 7
    for (H, W), fields in [((4, 9), dict(mode=1, ksize=9)),
                           ((5, 7), dict(mode=2, ksize=9, sigma=38.0))]:
        p = _blur_params(2, H, W, 0, 0)
        for name, v in fields.items():
            p["blur"][name][1] = v
        rc, msg, out = raw_call(H, W, p)
        assert rc == 0, msg
        assert bool((out != 7.0).all())


# ---- 6. determinism ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sigma", [(1, 0.0), (2, 38.0)])
def test_blur_is_deterministic(cuda, mode, sigma):
    from input_pipelines.augment import augment_images
    H, W = 70, 131
    raw = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (4, H, W, 3), dtype=np.uint8)).to(cuda)
    p = _blur_params(4, H, W, mode, KSIZES, sigma)
    p["color_order"], p["brightness_delta"], p["contrast_factor"] = [0, 1, 2, 3], 0.04, 0.8
    p["quantize"], p["flip"] = 1, [0, 1, 0, 1]
    p["scale_mode"], p["sh"], p["sw"] = [0, 0, 2, 1], [H, H, 50, 60], [W, W, 100, 90]
    a = augment_images(raw, p, H, W)
    b = augment_images(raw, p, H, W)
    assert torch.equal(a, b)
    assert bool(torch.isfinite(a).all()) and float(a.min()) >= -1.0 and float(a.max()) <= 1.0


# ---- 7. pipeline ---------------------------------------------------------------------------------
H8, W8 = 64, 128


class _Cfg:
    class train_distribute:
        num_towers = 1


def _pipeline_params(**kw):
    import json
    pkg = os.path.join(os.path.dirname(HERE), "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")
    pd = json.load(open(os.path.join(pkg, "problem_definitions", "cityscapes", "problem01.json")))
    return SimpleNamespace(height_feature_extractor=H8, width_feature_extractor=W8, Nb_per_pixel=2,
                           Nb_per_bbox=2, Nb_per_image=2, input_seed=3, input_workers=2,
                           input_prefetch=2, training_problem_def=pd,
                           tfrecords_path_per_pixel=[os.path.join(TINY, "cityscapes.tfrecord")],
                           bboxes_index_path=os.path.join(TINY, "bboxes.json"),
                           bboxes_images_dir=os.path.join(TINY, "images"),
                           image_labels_index_path=os.path.join(TINY, "tags.json"),
                           image_labels_images_dir=os.path.join(TINY, "images"), **kw)


def _take(params, k):
    from input_pipelines.train_inputs import heterogeneous_train_input
    gen = heterogeneous_train_input(_Cfg, params)
    out = []
    try:
        for _ in range(k):
            f, l = next(gen)
            out.append((f["proimages"].cpu().numpy(), l["prolabels_per_pixel"].cpu().numpy(),
                        list(l["prolabels_per_bbox"]), list(l["prolabels_per_image"])))
    finally:
        gen.close()
    return out


def _same_items(a, b):
    return len(a) == len(b) and all(
        len(x) == len(y) and all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(x, y))
        for x, y in zip(a, b))


@pytest.fixture(scope="module")
def plain_batches(cuda):
    return _take(_pipeline_params(), 3)


def test_pipeline_blur_off_draws_nothing(cuda, plain_batches, monkeypatch):
    """--augment_blur off: no blur generator exists, draw_params is never asked for a blur, and
    the batches with the other three flags on are those drawn without the blur arguments."""
    from input_pipelines import augment
    assert _same_items([b[:2] for b in plain_batches],
                       [b[:2] for b in _take(_pipeline_params(augment_blur=False), 3)])
    on = dict(augment_color=True, augment_flip=True, augment_scale=[1.0, 2.0])
    calls = []
    orig = augment.draw_params

    def no_blur(rng, n, H, W, **kw):
        calls.append((kw.pop("blur", False), kw.pop("blur_rng", None)))
        return orig(rng, n, H, W, **kw)       # the parent's signature
    monkeypatch.setattr(augment, "draw_params", no_blur)
    a = _take(_pipeline_params(augment_blur=False, **on), 2)
    monkeypatch.undo()
    assert calls and all(c == (False, None) for c in calls)
    b = _take(_pipeline_params(**on), 2)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        assert _same_items(x[2], y[2]) and x[3] == y[3]


def test_pipeline_blur_on_matches_the_restatement(cuda, plain_batches):
    """--augment_blur alone, fixed seed: every stream's images are the restatement's for the
    draws of default_rng([seed, s, rank, 3]) (median batches bitwise, bilateral ones within the
    float32 restatement's bound); labels, boxes and tags are those of the plain batches."""
    from input_pipelines import train_inputs as ti
    from input_pipelines.augment import draw_params
    params = _pipeline_params(augment_blur=True)
    got = _take(params, 3)
    seed = params.input_seed
    void_cid = max(params.training_problem_def["lids2cids"]) + 1
    rngs = [np.random.default_rng([seed, s, 0]) for s in range(3)]
    geom = [np.random.default_rng([seed, s, 0, 1]) for s in range(3)]
    aug = [np.random.default_rng([seed, s, 0, 2]) for s in range(3)]
    brng = [np.random.default_rng([seed, s, 0, 3]) for s in range(3)]
    pp = ti.PerPixelStream(params.tfrecords_path_per_pixel, rngs[0])
    pb = ti.OpenImagesStream(params.bboxes_index_path, params.bboxes_images_dir, rngs[1])
    pi = ti.OpenImagesStream(params.image_labels_index_path, params.image_labels_images_dir, rngs[2])
    modes = set()

    def draw(s):
        p = draw_params(aug[s], 2, H8, W8, void_cid=void_cid, blur=True, blur_rng=brng[s])
        modes.add(int(p["blur"]["mode"][0]))
        return p

    def check(image, raw, rec, **kw):
        r32, _ = blur_ref.augment_image_blur(raw, rec, H8, W8, dtype=np.float32, **kw)
        if rec["blur"]["mode"] != 2:
            assert np.array_equal(image, r32)
            return
        r64, _ = blur_ref.augment_image_blur(raw, rec, H8, W8, dtype=np.float64, **kw)
        assert np.abs(image - r64).max() <= 4.0 * np.abs(r32 - r64).max()
    for k in range(3):
        ims = got[k][0]
        assert ims.shape == (6, H8, W8, 3)
        p = draw(0)
        for i, e in enumerate(pp.take(2)):
            check(ims[i], e[0], p[i])
        p = draw(1)
        for i, (iid, im, ann) in enumerate(pb.take(2)):
            item = ti.box_item(ann, im.shape[:2], H8, W8, geom[1])
            check(ims[2 + i], im, p[i], resized=item[3], offset=item[4])
        p = draw(2)
        for i, (iid, im, ann) in enumerate(pi.take(2)):
            rs, off = ti._weak_geometry(im.shape[:2], H8, W8, geom[2])
            check(ims[4 + i], im, p[i], resized=rs, offset=off)
        # labels and box maps are untouched
        assert np.array_equal(got[k][1], plain_batches[k][1])
        assert _same_items(got[k][2], plain_batches[k][2]) and got[k][3] == plain_batches[k][3]
    assert modes == {0, 1, 2}
    assert not all(np.array_equal(x[0], z[0]) for x, z in zip(got, plain_batches))


# ---- 8. train step -------------------------------------------------------------------------------
def test_train_step_with_all_four_stages(cuda, tmp_path, monkeypatch):
    """One train.py step through the facade with colour, blur, flip and scaling on."""
    import train
    from estimator.define_estimator_hierarchical import get_or_create_global_step
    from models import resnet50_extended_model_hierarchical as mh
    import system_factory as sf
    mh.release_contexts()
    get_or_create_global_step().value = 0
    logged = []
    orig = sf.define_estimator

    def wrapped(mode, features, labels, model_fn, config, params):
        spec = orig(mode, features, labels, model_fn, config, params)
        if spec.train_op is None:
            return spec

        def train_op():
            L = spec.train_op()
            logged.append([float(L[n]) for n in ("total", "l1_segmentation", "l2_vehicle_segmentation",
                                                 "l2_human_segmentation")])
            return L
        return spec._replace(train_op=train_op)
    monkeypatch.setattr(sf, "define_estimator", wrapped)
    argv = [str(tmp_path / "logs"), "cityscapes", "--max_steps", "1", "--compute_dtype", "fp32",
            "--height_feature_extractor", str(H8), "--width_feature_extractor", str(W8),
            "--Nb_per_pixel", "2", "--Nb_per_bbox", "2", "--Nb_per_image", "2",
            "--learning_rate_initial", "1e-5", "--save_summaries_steps", "1",
            "--save_checkpoints_steps", "100",
            "--tfrecords_path_per_pixel", os.path.join(TINY, "cityscapes.tfrecord"),
            "--bboxes_index_path", os.path.join(TINY, "bboxes.json"),
            "--bboxes_images_dir", os.path.join(TINY, "images"),
            "--image_labels_index_path", os.path.join(TINY, "tags.json"),
            "--image_labels_images_dir", os.path.join(TINY, "images"),
            "--input_workers", "2", "--input_seed", "3",
            "--augment_color", "--augment_blur", "--augment_flip", "--augment_scale", "1.0", "2.0"]
    try:
        assert train.main(argv) == 1
    finally:
        mh.release_contexts()
    assert len(logged) == 1 and np.isfinite(logged[0]).all() and logged[0][0] > 0
