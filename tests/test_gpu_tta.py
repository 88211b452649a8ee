"""Test-time augmentation on the GPU (include/seg_hip.h at seg_tta_decisions): the image pyramid
kernel, the multi-entry decision head, the host driver and the evaluate.py / predict.py flags.

* seg_resize_images against the float64 reference: max abs error <= 1e-6 on data in [-1, 1) (six
  fp32 roundings of <= 2^-24 each are 3.6e-7); equal sizes copy / mirror bit for bit.
* one unflipped entry holding a context's own logits: decisions bitwise seg_predict's (modes 0
  and 1), mean probabilities bitwise seg_full_predictions'.
* many entries on synthetic logits: mean probabilities <= 1e-5 norm-relative against float64
  (the bound test_model_predictions_full_resolution holds the same arithmetic to), decisions
  differing on <= 1e-3 of the pixels (the project's near-tie cap; tests/test_tta_host.py shows
  the reference's own float32-vs-float64 share is 0 on these inputs).
* the driver: every scale context computes what a stand-alone context of that size with the same
  parameters computes, bit for bit; the decisions equal the reference on those native logits.
* evaluate.py / predict.py end to end, including the re-synchronisation of the scale contexts
  after every checkpoint restore of --eval_all_ckpts.
"""
import argparse
import ctypes
import errno

import numpy as np
import pytest
import torch

import tta_ref
from inference_common import (MAPS, PROBLEM, _realistic_moving_stats, _rel, _script,  # noqa: F401
                              city_ctx, vistas_ctx)

pytestmark = pytest.mark.gpu


# ---- seg_resize_images ---------------------------------------------------------------------

def _images(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, h, w, 3), dtype=np.float32) * 2 - 1).astype(np.float32)


@pytest.mark.parametrize("hw", [(64, 128), (101, 103), (8, 8)])
def test_resize_same_size_is_copy_or_mirror(cuda, hw):
    from seg_hip import resize_images
    x = _images(2, hw[0], hw[1], 1)
    xd = torch.from_numpy(x).to(cuda)
    np.testing.assert_array_equal(resize_images(xd, hw[0], hw[1], False).cpu().numpy(), x)
    np.testing.assert_array_equal(resize_images(xd, hw[0], hw[1], True).cpu().numpy(), x[:, :, ::-1])


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("src,dst", [((64, 128), (48, 96)), ((64, 128), (80, 160)),
                                     ((101, 103), (32, 40)), ((8, 8), (33, 17))])
def test_resize_against_float64(cuda, src, dst, flip):
    from seg_hip import resize_images
    x = _images(2, src[0], src[1], 2)
    got = resize_images(torch.from_numpy(x).to(cuda), dst[0], dst[1], flip).cpu().numpy()
    ref = tta_ref.resize_images_ref(x, dst[0], dst[1], flip, np.float64)
    assert got.shape == ref.shape == (2,) + dst + (3,) and got.dtype == np.float32
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"resize {src} -> {dst} flip {flip}: max abs error {err:.3e}")
    assert err <= 1e-6


def test_resize_rejects_bad_arguments(cuda):
    from seg_hip import LIB, resize_images
    x = torch.zeros((1, 8, 8, 3), device=cuda)
    out = torch.full((1, 8, 8, 3), 7.0, device=cuda)
    for args in ((x.data_ptr(), 1, 8, 8, 0, 8, 0, out.data_ptr(), None),
                 (x.data_ptr(), 1, 8, 8, 8, 8, 2, out.data_ptr(), None),
                 (None, 1, 8, 8, 8, 8, 0, out.data_ptr(), None),
                 (x.data_ptr(), -1, 8, 8, 8, 8, 0, out.data_ptr(), None)):
        assert LIB.seg_resize_images(*args) == -errno.EINVAL
        assert b"seg_resize_images" in LIB.seg_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError):
        resize_images(torch.zeros((1, 8, 8, 4), device=cuda), 8, 8)


# ---- one entry: the bits of seg_predict / seg_full_predictions ---------------------------

@pytest.mark.parametrize("replace_voids", [False, True])
@pytest.mark.parametrize("out_hw", [(64, 128), (32, 64), (45, 77), (128, 256)])
@pytest.mark.parametrize("mapname", sorted(MAPS))
def test_single_entry_is_predict_bitwise(cuda, city_ctx, mapname, out_hw, replace_voids):
    ctx = city_ctx
    lg = ctx.outputs()[2]
    assert float(lg.std()) > 1e-3 and bool(torch.isfinite(lg).all())
    want = torch.full((2,) + out_hw, -7, dtype=torch.int32, device=cuda)
    ctx.predict(MAPS[mapname], want, replace_voids=replace_voids)
    got = torch.full((2,) + out_hw, -9, dtype=torch.int32, device=cuda)
    ctx.tta_decisions([(lg, False)], MAPS[mapname], got, replace_voids=replace_voids)
    assert int(want.min()) >= 0
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_single_entry_mean_is_full_predictions_bitwise(cuda, city_ctx):
    ctx = city_ctx
    lg = ctx.outputs()[2]
    want = torch.full((2, 64, 128, 24), -1.0, device=cuda)
    ctx.full_predictions(probs=want)
    got = torch.full((2, 64, 128, 24), -2.0, device=cuda)
    decs = torch.empty((2, 64, 128), dtype=torch.int32, device=cuda)
    ctx.tta_decisions([(lg, False)], MAPS["identity"], decs, mean_probs=got)
    ne = got != want
    print(f"mean probabilities vs seg_full_predictions: {int(ne.sum())} of {ne.numel()} values differ, "
          f"max abs {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)
    # the l1 probabilities are neither uniform nor one-hot everywhere: the comparison has content
    top = float(want[..., :14].max(-1).values.mean())
    print(f"mean of the largest l1 probability: {top:.4f}")
    assert 1.0 / 14 + 1e-3 < top < 0.9999


# ---- many entries against float64 ------------------------------------------------------

EXTRA = ((1, 2),)   # the n_in = 1 branch of the align-corners scaler (scale 0)


def _device_entries(dataset, amplitude, cuda):
    """The synthetic entries on the device; every third one in a padded buffer (ld > CT) whose
    padding is NaN, so that a read past the CT channels of a pixel shows."""
    ct = sum(tta_ref.WIDTHS[dataset])
    out = []
    for i, (lg, flip) in enumerate(tta_ref.synthetic_entries(dataset, amplitude, EXTRA)):
        t = torch.from_numpy(lg).to(cuda)
        if i % 3 == 0:
            pad = torch.full(t.shape[:3] + (ct + 5 + i,), float("nan"), device=cuda)
            pad[..., :ct] = t
            t = pad
        out.append((t, flip))
    return out


@pytest.mark.parametrize("dataset,amplitude", [("cityscapes", 1.0), ("cityscapes", 3.0),
                                               ("vistas", 1.0), ("vistas", 3.0)])
def test_multi_entry_against_float64(cuda, city_ctx, vistas_ctx, dataset, amplitude):
    ctx = city_ctx if dataset == "cityscapes" else vistas_ctx
    ct = sum(tta_ref.WIDTHS[dataset])
    ents = _device_entries(dataset, amplitude, cuda)
    assert len(ents) == 12 and any(t.shape[3] > ct for t, _ in ents)
    cid_map = tta_ref.IDENTITY_MAP[dataset]
    H, W = tta_ref.NET_HW
    for rv in (False, True):
        for out_hw in ((H, W), (45, 77)):
            p64, d64, stats = tta_ref.synthetic_reference(dataset, amplitude, EXTRA, out_hw, rv,
                                                          torch.float64)
            got = torch.full((tta_ref.BATCH,) + out_hw, -9, dtype=torch.int32, device=cuda)
            probs = None
            if out_hw == (H, W):
                probs = torch.full((tta_ref.BATCH, H, W, ct), -2.0, device=cuda)
            ctx.tta_decisions(ents, cid_map, got, replace_voids=rv, mean_probs=probs)
            d = got.cpu().numpy()
            mism = float(np.mean(d != d64))
            line = f"{dataset} x{amplitude} rv {rv} out {out_hw}: decisions differ on {mism:.2e}"
            if probs is not None:
                rel = _rel(probs.cpu().numpy(), p64)
                line += f", mean probabilities {rel:.2e} norm-relative"
            print(line + f", branches {stats}")
            assert d.min() >= 0
            assert mism <= 1e-3
            if probs is not None:
                assert rel <= 1e-5


def test_flip_consistency(cuda, city_ctx):
    """[(L, no flip)] and [(L mirrored in x, flip)] describe the same image."""
    ct = 24
    decs = torch.empty((2, 64, 128), dtype=torch.int32, device=cuda)
    for lg, _ in tta_ref.synthetic_entries("cityscapes", 3.0)[::2]:
        t = torch.from_numpy(lg).to(cuda)
        a = torch.empty((2, 64, 128, ct), device=cuda)
        b = torch.empty((2, 64, 128, ct), device=cuda)
        city_ctx.tta_decisions([(t, False)], MAPS["identity"], decs, mean_probs=a)
        city_ctx.tta_decisions([(torch.flip(t, dims=(2,)).contiguous(), True)], MAPS["identity"], decs,
                               mean_probs=b)
        assert _rel(b.cpu().numpy(), a.cpu().numpy()) <= 1e-5


# ---- error paths ---------------------------------------------------------------------------

def test_decisions_reject_bad_arguments(cuda, city_ctx):
    from seg_hip import LIB, TtaEntry
    ctx = city_ctx
    lg = torch.zeros((2, 8, 16, 24), device=cuda)
    out = torch.full((2, 64, 128), -7, dtype=torch.int32, device=cuda)
    probs = torch.full((2, 64, 128, 24 + 1), -3.0, device=cuda)
    ident = MAPS["identity"]

    def call(entries=None, n_entries=None, cid_map=ident, rv=0, out_hw=(64, 128), probs_ptr=None,
             out_ptr=out.data_ptr(), null_entries=False, null_map=False):
        entries = [TtaEntry(lg.data_ptr(), 8, 16, 24, 0)] if entries is None else entries
        arr = (TtaEntry * max(len(entries), 1))(*entries)
        m = (ctypes.c_int32 * len(cid_map))(*cid_map)
        return LIB.seg_tta_decisions(ctx.h, None if null_entries else arr,
                                     len(entries) if n_entries is None else n_entries,
                                     None if null_map else m, len(cid_map), rv, out_hw[0], out_hw[1],
                                     probs_ptr, out_ptr, None)
    assert call() == 0                       # the baseline call is valid
    torch.cuda.synchronize()
    assert int(out.min()) >= 0
    out.fill_(-7)
    e = lambda **kw: TtaEntry(**{**dict(logits=lg.data_ptr(), h_low=8, w_low=16, ld=24, flip=0), **kw})
    cases = {
        "no entries": dict(entries=[], n_entries=0),
        "17 entries": dict(entries=[e()] * 17),
        "null entries": dict(null_entries=True),
        "null logits": dict(entries=[e(), e(logits=None)]),
        "null cid map": dict(null_map=True),
        "null decisions": dict(out_ptr=None),
        "h_low 0": dict(entries=[e(h_low=0)]),
        "w_low 0": dict(entries=[e(w_low=0)]),
        "ld below the channels": dict(entries=[e(ld=23)]),
        "flip 2": dict(entries=[e(flip=2)]),
        "flip -1": dict(entries=[e(flip=-1)]),
        "replace_voids 2": dict(rv=2),
        "replace_voids 3": dict(rv=3),
        "replace_voids -1": dict(rv=-1),
        "short cid map": dict(cid_map=ident[:-1]),
        "cid map entry -2": dict(cid_map=[-2] + ident[1:]),
        "out_h 0": dict(out_hw=(0, 128)),
        "out_w 0": dict(out_hw=(64, 0)),
        "misaligned mean": dict(probs_ptr=probs.data_ptr() + 4),
        "mean at another size": dict(probs_ptr=probs.data_ptr(), out_hw=(32, 64)),
    }
    for name, kw in cases.items():
        rc = call(**kw)
        msg = LIB.seg_last_error(ctx.h).decode()
        assert rc == -errno.EINVAL, (name, rc)
        assert "seg_tta_decisions" in msg, (name, msg)
        if name == "replace_voids 2":
            assert "averaged" in msg
    assert LIB.seg_tta_decisions(None, None, 1, None, 20, 0, 64, 128, None, out.data_ptr(), None) == -errno.EINVAL
    assert b"seg_tta_decisions" in LIB.seg_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((probs == -3.0).all())
    # the wrapper's own checks
    with pytest.raises(RuntimeError, match="averaged"):
        ctx.tta_decisions([(lg, False)], ident, out, replace_voids=2)
    with pytest.raises(ValueError):
        ctx.tta_decisions([(lg, False)] * 17, ident, out)
    with pytest.raises(ValueError):
        ctx.tta_decisions([(lg[:1], False)], ident, out)
    assert bool((out == -7).all())


# ---- the driver ----------------------------------------------------------------------------

SCALES = (0.75, 1.0, 1.25)


def _settings(dtype):
    return argparse.Namespace(Nb=2, height_feature_extractor=64, width_feature_extractor=128,
                              per_pixel_dataset_name="cityscapes", compute_dtype=dtype,
                              pyramid="psp", name_feature_extractor="resnet_v1_50", init_seed=3,
                              tta_scales=list(SCALES), tta_flip=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_driver_scale_contexts_and_decisions(cuda, dtype):
    """Base 64 x 128, PSP, Nb = 2, scales 0.75 1.0 1.25 with flip: each entry's logits are bitwise
    those of a stand-alone context of that size loaded with the same named parameters, and the
    driver's decisions are the reference's on those native logits (teacher-forced)."""
    from estimator.mode_keys import ModeKeys
    from estimator.tta import driver_for, tta_sizes
    from input_pipelines.synthetic import batch
    from models.resnet50_extended_model_hierarchical import get_context, release_contexts
    from seg_hip import SegContext, resize_images
    release_contexts()
    s = _settings(dtype)
    primary = get_context(None, s, mode=ModeKeys.EVAL)
    _realistic_moving_stats(primary, torch.as_tensor(batch(99, 2, 0, 0, 64, 128)["images"]).to(cuda))
    x = torch.as_tensor(batch(12, 2, 0, 0, 64, 128)["images"]).to(cuda)
    primary.forward(x)                                   # what model_fn does
    drv = driver_for(primary, None, s, ModeKeys.EVAL)
    assert drv is driver_for(primary, None, s, ModeKeys.EVAL)
    assert drv.sizes == tta_sizes(64, 128, SCALES) == [(48, 96), (64, 128), (80, 160)]
    assert drv.contexts[1] is primary
    out = torch.full((2, 45, 77), -9, dtype=torch.int32, device=cuda)
    ents = drv.decisions(x, MAPS["merge"], out, replace_voids=True)
    assert [f for _, f in ents] == [False, True] * 3
    assert [tuple(t.shape[1:3]) for t, _ in ents] == [(6, 12)] * 2 + [(8, 16)] * 2 + [(10, 20)] * 2
    named = primary.named("params")
    for i, (h, w) in enumerate(drv.sizes):
        alone = SegContext(pyramid="psp", height=h, width=w, nb_pp=2, dtype=dtype)
        alone.load_params(named)
        alone.set_bn_inference(True)
        for k, flip in enumerate((False, True)):
            alone.forward(resize_images(x, h, w, flip))
            assert torch.equal(alone.outputs()[2], ents[2 * i + k][0]), (h, w, flip)
        alone.close()
    _, ref, _ = tta_ref.tta_reference([(t.cpu().numpy(), f) for t, f in ents], (64, 128), "cityscapes",
                                      MAPS["merge"], (45, 77), True, torch.float64)
    mism = float(np.mean(out.cpu().numpy() != ref))
    print(f"driver {dtype}: decisions differ from the reference on {mism:.2e}")
    assert mism <= 1e-3
    # the lazy predictions under test-time augmentation
    from models.resnet50_extended_model_hierarchical import Predictions
    pred = Predictions(primary, "cityscapes")
    drv.attach(pred, ents)
    p1 = pred["l1_probabilities"]
    assert tuple(p1.shape) == (2, 64, 128, 14)
    np.testing.assert_allclose(p1.sum(-1).cpu().numpy(), 1.0, atol=1e-5)
    assert torch.equal(pred["l1_decisions"].long(), torch.argmax(p1, dim=-1))
    assert tuple(pred["l2_human_probabilities"].shape) == (2, 64, 128, 3)
    with pytest.raises(KeyError, match="test-time augmentation"):
        pred["l1_logits"]
    # the primary's last forward was the mirrored image: the eager low-resolution entries still
    # describe the batch itself (the clone of its unflipped logits)
    assert torch.equal(pred["l1_logits_lowres"], ents[2][0][..., :14])
    assert torch.equal(pred["l2_human_logits_lowres"], ents[2][0][..., 21:24])
    assert torch.equal(primary.outputs()[2], ents[3][0]) and not torch.equal(ents[2][0], ents[3][0])
    # a reload of the primary's parameters reaches the scale contexts at the next batch
    from models.initializers import init_params
    primary.load_params(init_params(primary.param_info, seed=4))
    assert not torch.equal(drv.contexts[0].params, primary.params)
    primary.forward(x)
    again = drv.entries(x)
    for c in (drv.contexts[0], drv.contexts[2]):
        assert torch.equal(c.params, primary.params) and torch.equal(c.moving, primary.moving)
    assert not torch.equal(again[0][0], ents[0][0])
    assert "l1_logits" not in set(pred) and "l1_probabilities" in set(pred)
    release_contexts()


def test_driver_names_the_scale_of_a_refused_size(cuda):
    """A PSP map too small for the 6 x 6 grid: seg_create's error, with the scale named."""
    from estimator.mode_keys import ModeKeys
    from estimator.tta import TTADriver
    from models.resnet50_extended_model_hierarchical import get_context, release_contexts
    release_contexts()
    s = _settings("fp32")
    primary = get_context(None, s, mode=ModeKeys.EVAL)
    with pytest.raises(RuntimeError, match=r"tta scale 0\.25 \(32 x 32\)"):
        TTADriver(primary, None, s, ModeKeys.EVAL, (1.0, 0.25), False)
    with pytest.raises(ValueError, match="entries"):
        TTADriver(primary, None, s, ModeKeys.EVAL, tuple(1.0 + 0.125 * i for i in range(9)), True)
    release_contexts()


# ---- evaluate.py / predict.py --------------------------------------------------------------

EVAL_ARGS = ["--Nb", "1", "--height_feature_extractor", "48", "--width_feature_extractor", "64",
             "--compute_dtype", "fp32"]
TTA_ARGS = ["--tta_scales", "0.75", "1.0", "1.25", "--tta_flip"]


def test_evaluate_scale_one_alone_changes_nothing(cuda, tmp_path, init_ckpt):
    from models.resnet50_extended_model_hierarchical import release_contexts
    ev = _script("evaluate")
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=1, dtype="fp32")
    base = [str(tmp_path), "2", PROBLEM, "cityscapes"] + EVAL_ARGS
    plain = ev.main(base + ["--eval_res_dir", str(tmp_path / "a")])
    one = ev.main(base + ["--eval_res_dir", str(tmp_path / "b"), "--tta_scales", "1.0"])
    assert len(plain) == len(one) == 1
    assert int(plain[0]["confusion_matrix"].sum()) > 0
    np.testing.assert_array_equal(one[0]["confusion_matrix"], plain[0]["confusion_matrix"])
    release_contexts()


def test_evaluate_all_ckpts_resynchronises(cuda, tmp_path, init_ckpt):
    """Two checkpoints of different seeds under --eval_all_ckpts with scales and flip: each
    confusion matrix is the one of evaluating that checkpoint alone."""
    from models.resnet50_extended_model_hierarchical import release_contexts
    ev = _script("evaluate")
    kw = dict(pyramid="none", height=48, width=64, nb_pp=1, dtype="fp32")
    init_ckpt(tmp_path, step=0, seed=0, **kw)
    init_ckpt(tmp_path, step=1, seed=1, **kw)
    base = [str(tmp_path), "2", PROBLEM, "cityscapes"] + EVAL_ARGS + TTA_ARGS
    # contexts and drivers are cached per process: every run below starts from none, so that an
    # alone run's scale contexts never held another checkpoint (fresh ones hold the seed-0
    # initialisation, which is checkpoint 0: a missing second copy would leave checkpoint 1's
    # scales at checkpoint 0 in the loop and be right alone)
    release_contexts()
    both = ev.main(base + ["--eval_all_ckpts", "--eval_res_dir", str(tmp_path / "all")])
    assert [m["global_step"] for m in both] == [0, 1]
    assert not np.array_equal(both[0]["confusion_matrix"], both[1]["confusion_matrix"])
    for step in (1, 0):
        release_contexts()
        alone = ev.main(base + ["--ckpt_path", str(tmp_path / f"model.ckpt-{step}.pt"),
                                "--eval_res_dir", str(tmp_path / f"one{step}")])
        np.testing.assert_array_equal(alone[0]["confusion_matrix"], both[step]["confusion_matrix"])
    release_contexts()


def test_predict_script_exports_with_tta(cuda, tmp_path, init_ckpt):
    from PIL import Image
    from models.resnet50_extended_model_hierarchical import release_contexts
    pdir, rdir = tmp_path / "in", tmp_path / "out"
    pdir.mkdir()
    rdir.mkdir()
    rng = np.random.default_rng(6)
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (50, 90, 3), dtype=np.uint8)).save(pdir / f"img{i}.png")
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=2, dtype="fp32")
    pr = _script("predict")
    n = pr.main([str(tmp_path), PROBLEM, str(pdir), "cityscapes", "--Nb", "2",
                 "--height_feature_extractor", "48", "--width_feature_extractor", "64",
                 "--compute_dtype", "fp32", "--results_dir", str(rdir), "--export_lids_images",
                 "--export_color_decisions", "--replace_voids"] + TTA_ARGS)
    assert n == 3
    for i in range(3):
        lids = np.asarray(Image.open(rdir / f"img{i}_result_lids.png"))
        col = np.asarray(Image.open(rdir / f"img{i}_result_color.png"))
        assert lids.shape == (50, 90) and col.shape == (50, 90, 3)
    release_contexts()
