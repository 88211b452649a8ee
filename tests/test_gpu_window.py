"""Sliding-window inference on the GPU (include/seg_hip.h at seg_window_decisions): the window
extraction kernel, the decision head over a grid of windows, the host driver and the
evaluate.py / predict.py flags.

* seg_window_images is a copy: bitwise numpy slicing and mirroring.
* canvas = network size: one window holding a context's own logits gives seg_predict's decisions
  (modes 0 and 1) and seg_full_predictions' probabilities bit for bit; [unflipped, mirrored] gives
  seg_tta_decisions' bits on the same two entries (pins r_k and the order of the sum).
* windows that do not overlap: every quadrant is bitwise seg_tta_decisions on that window's
  logits alone (pins the origin arithmetic).
* overlapping windows on synthetic logits against float64: mean probabilities <= 1e-5
  norm-relative (the bound tests/test_gpu_tta.py holds the same arithmetic to), decisions
  differing on <= 1e-3 of the pixels (tests/test_window_host.py shows the reference's own
  float32-vs-float64 share is 0 on these inputs).
* the driver: every entry is what the context computes on that window alone, bit for bit; the
  decisions equal the reference on those native logits.
* evaluate.py / predict.py end to end.
"""
import argparse
import ctypes
import errno

import numpy as np
import pytest
import torch

import tta_ref
import window_ref
from inference_common import (MAPS, PROBLEM, _realistic_moving_stats, _rel, _script,  # noqa: F401
                              city_ctx, vistas_ctx)

pytestmark = pytest.mark.gpu

H, W = window_ref.NET_HW


# ---- seg_window_images ---------------------------------------------------------------------

def _canvas(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, h, w, 3), dtype=np.float32) * 2 - 1).astype(np.float32)


@pytest.mark.parametrize("hw,places", [
    ((64, 128), [(0, 0), (36, 72), (0, 72), (36, 0), (17, 23)]),        # the four corners + inside
    ((37, 53), [(0, 0), (63, 147), (0, 147), (63, 0), (11, 101)]),
    ((100, 200), [(0, 0)]),                                             # window = canvas
])
def test_window_images_is_a_copy(cuda, hw, places):
    from seg_hip import window_images
    x = _canvas(2, 100, 200, 1)
    xd = torch.from_numpy(x).to(cuda)
    h, w = hw
    for y0, x0 in places:
        want = x[:, y0:y0 + h, x0:x0 + w]
        got = window_images(xd, y0, x0, h, w, False).cpu().numpy()
        assert got.shape == (2, h, w, 3) and got.dtype == np.float32
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(window_images(xd, y0, x0, h, w, True).cpu().numpy(), want[:, :, ::-1])


def test_window_images_rejects_bad_arguments(cuda):
    from seg_hip import LIB, window_images
    x = torch.zeros((1, 16, 24, 3), device=cuda)
    out = torch.full((1, 8, 8, 3), 7.0, device=cuda)
    xp, op = x.data_ptr(), out.data_ptr()
    #        in  n  Hc  Wc  y0 x0 H  W  flip out
    cases = {
        "null in": (None, 1, 16, 24, 0, 0, 8, 8, 0, op),
        "null out": (xp, 1, 16, 24, 0, 0, 8, 8, 0, None),
        "n -1": (xp, -1, 16, 24, 0, 0, 8, 8, 0, op),
        "Hc 0": (xp, 1, 0, 24, 0, 0, 8, 8, 0, op),
        "Wc 0": (xp, 1, 16, 0, 0, 0, 8, 8, 0, op),
        "H 0": (xp, 1, 16, 24, 0, 0, 0, 8, 0, op),
        "W 0": (xp, 1, 16, 24, 0, 0, 8, 0, 0, op),
        "y0 -1": (xp, 1, 16, 24, -1, 0, 8, 8, 0, op),
        "x0 -1": (xp, 1, 16, 24, 0, -1, 8, 8, 0, op),
        "below the canvas": (xp, 1, 16, 24, 9, 0, 8, 8, 0, op),
        "right of the canvas": (xp, 1, 16, 24, 0, 17, 8, 8, 0, op),
        "flip 2": (xp, 1, 16, 24, 0, 0, 8, 8, 2, op),
        "flip -1": (xp, 1, 16, 24, 0, 0, 8, 8, -1, op),
    }
    for name, args in cases.items():
        assert LIB.seg_window_images(*args, None) == -errno.EINVAL, name
        assert b"seg_window_images" in LIB.seg_last_error(None), name
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert LIB.seg_window_images(xp, 1, 16, 24, 8, 16, 8, 8, 1, op, None) == 0   # the last valid origin
    with pytest.raises(ValueError):
        window_images(torch.zeros((1, 8, 8, 4), device=cuda), 0, 0, 8, 8)
    with pytest.raises(RuntimeError, match="seg_window_images"):
        window_images(x, 9, 0, 8, 8)


# ---- canvas = network size: the bits of seg_predict / seg_full_predictions / seg_tta_decisions

@pytest.mark.parametrize("replace_voids", [False, True])
@pytest.mark.parametrize("out_hw", [(64, 128), (45, 77), (128, 256)])
@pytest.mark.parametrize("mapname", sorted(MAPS))
def test_one_window_is_predict_bitwise(cuda, city_ctx, mapname, out_hw, replace_voids):
    ctx = city_ctx
    lg = ctx.outputs()[2]
    assert float(lg.std()) > 1e-3 and bool(torch.isfinite(lg).all())
    want = torch.full((2,) + out_hw, -7, dtype=torch.int32, device=cuda)
    ctx.predict(MAPS[mapname], want, replace_voids=replace_voids)
    got = torch.full((2,) + out_hw, -9, dtype=torch.int32, device=cuda)
    ctx.window_decisions([lg], [0], [0], False, (64, 128), MAPS[mapname], got,
                         replace_voids=replace_voids)
    assert int(want.min()) >= 0
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_one_window_mean_is_full_predictions_bitwise(cuda, city_ctx):
    ctx = city_ctx
    lg = ctx.outputs()[2]
    want = torch.full((2, 64, 128, 24), -1.0, device=cuda)
    ctx.full_predictions(probs=want)
    got = torch.full((2, 64, 128, 24), -2.0, device=cuda)
    decs = torch.empty((2, 64, 128), dtype=torch.int32, device=cuda)
    ctx.window_decisions([lg], [0], [0], False, (64, 128), MAPS["identity"], decs, mean_probs=got)
    ne = got != want
    print(f"mean probabilities vs seg_full_predictions: {int(ne.sum())} of {ne.numel()} values differ, "
          f"max abs {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)


def _synthetic_device(dataset, amplitude, cuda, canvas_hw=window_ref.CANVAS_HW):
    return [torch.from_numpy(e).to(cuda) for e in window_ref.synthetic_entries(dataset, amplitude, canvas_hw)]


@pytest.mark.parametrize("dataset", ["cityscapes", "vistas"])
@pytest.mark.parametrize("replace_voids", [False, True])
def test_unflipped_and_mirrored_is_tta_bitwise(cuda, city_ctx, vistas_ctx, dataset, replace_voids):
    """Canvas = network size, entries [unflipped, mirrored]: k = 2 everywhere."""
    ctx = city_ctx if dataset == "cityscapes" else vistas_ctx
    ct = sum(window_ref.WIDTHS[dataset])
    a, b = _synthetic_device(dataset, 3.0, cuda)[:2]
    cid_map = window_ref.IDENTITY_MAP[dataset]
    for out_hw in ((64, 128), (45, 77)):
        probs = out_hw == (64, 128)
        want = torch.full((2,) + out_hw, -7, dtype=torch.int32, device=cuda)
        want_p = torch.full((2, 64, 128, ct), -1.0, device=cuda) if probs else None
        ctx.tta_decisions([(a, False), (b, True)], cid_map, want, replace_voids=replace_voids,
                          mean_probs=want_p)
        got = torch.full((2,) + out_hw, -9, dtype=torch.int32, device=cuda)
        got_p = torch.full((2, 64, 128, ct), -2.0, device=cuda) if probs else None
        ctx.window_decisions([a, b], [0], [0], True, (64, 128), cid_map, got,
                             replace_voids=replace_voids, mean_probs=got_p)
        assert int(want.min()) >= 0
        assert torch.equal(got, want)
        if probs:
            assert torch.equal(got_p, want_p)


@pytest.mark.parametrize("dataset", ["cityscapes", "vistas"])
def test_disjoint_windows_are_tta_per_quadrant_bitwise(cuda, city_ctx, vistas_ctx, dataset):
    """Canvas 128 x 256, stride (64, 128): 4 windows that do not overlap, k = 1 everywhere."""
    ctx = city_ctx if dataset == "cityscapes" else vistas_ctx
    ct = sum(window_ref.WIDTHS[dataset])
    ents = _synthetic_device(dataset, 3.0, cuda)[:4]
    cid_map = window_ref.IDENTITY_MAP[dataset]
    ys, xs = window_ref.origins(128, 64, 64), window_ref.origins(256, 128, 128)
    assert (ys, xs) == ([0, 64], [0, 128])
    for rv in (False, True):
        got = torch.full((2, 128, 256), -9, dtype=torch.int32, device=cuda)
        got_p = torch.full((2, 128, 256, ct), -2.0, device=cuda)
        ctx.window_decisions(ents, ys, xs, False, (128, 256), cid_map, got, replace_voids=rv,
                             mean_probs=got_p)
        for e, (y0, x0, _) in zip(ents, window_ref.placements(ys, xs, False)):
            want = torch.full((2, 64, 128), -7, dtype=torch.int32, device=cuda)
            want_p = torch.full((2, 64, 128, ct), -1.0, device=cuda)
            ctx.tta_decisions([(e, False)], cid_map, want, replace_voids=rv, mean_probs=want_p)
            assert int(want.min()) >= 0
            assert torch.equal(got[:, y0:y0 + 64, x0:x0 + 128], want), (y0, x0, rv)
            assert torch.equal(got_p[:, y0:y0 + 64, x0:x0 + 128], want_p), (y0, x0, rv)


# ---- overlapping windows against float64 ------------------------------------------------

def _padded(ents, ct, cuda):
    """The entries in padded buffers (ld > CT) whose padding is NaN, so that a read past the CT
    channels of a pixel shows. The entries of one launch share one ld, so padding every third
    entry pads them all."""
    ld = ct + 5
    out = []
    for t in ents:
        pad = torch.full(t.shape[:3] + (ld,), float("nan"), device=cuda)
        pad[..., :ct] = t
        out.append(pad)
    return out


def _against_float64(ctx, dataset, amplitude, canvas_hw, outs, cuda):
    ct = sum(window_ref.WIDTHS[dataset])
    ents = _padded(_synthetic_device(dataset, amplitude, cuda, canvas_hw), ct, cuda)
    ys, xs = window_ref.synthetic_grid(canvas_hw)
    assert len(ents) == 2 * len(ys) * len(xs) and ents[0].shape[3] > ct
    cid_map = window_ref.IDENTITY_MAP[dataset]
    for rv in (False, True):
        for out_hw in outs:
            p64, d64, count, stats = window_ref.synthetic_reference(dataset, amplitude, out_hw, rv,
                                                                    torch.float64, canvas_hw)
            got = torch.full((window_ref.BATCH,) + out_hw, -9, dtype=torch.int32, device=cuda)
            probs = None
            if out_hw == canvas_hw:
                probs = torch.full((window_ref.BATCH,) + canvas_hw + (ct,), -2.0, device=cuda)
            ctx.window_decisions(ents, ys, xs, True, canvas_hw, cid_map, got, replace_voids=rv,
                                 mean_probs=probs)
            d = got.cpu().numpy()
            mism = float(np.mean(d != d64))
            line = (f"{dataset} x{amplitude} canvas {canvas_hw} rv {rv} out {out_hw}: coverage "
                    f"{count.min()}..{count.max()}, decisions differ on {mism:.2e}")
            if probs is not None:
                rel = _rel(probs.cpu().numpy(), p64)
                line += f", mean probabilities {rel:.2e} norm-relative"
            print(line + f", branches {stats}")
            assert d.min() >= 0
            assert mism <= 1e-3
            if probs is not None:
                assert rel <= 1e-5


@pytest.mark.parametrize("dataset,amplitude", [("cityscapes", 1.0), ("cityscapes", 3.0),
                                               ("vistas", 1.0), ("vistas", 3.0)])
def test_overlapping_windows_against_float64(cuda, city_ctx, vistas_ctx, dataset, amplitude):
    """Network 64 x 128, canvas 100 x 200, stride (24, 40), flip: 18 entries, coverage 2..18."""
    ctx = city_ctx if dataset == "cityscapes" else vistas_ctx
    _against_float64(ctx, dataset, amplitude, (100, 200), ((100, 200), (45, 77)), cuda)


@pytest.mark.parametrize("canvas_hw", [(64, 200), (100, 128)])
@pytest.mark.parametrize("dataset", ["cityscapes", "vistas"])
def test_one_axis_against_float64(cuda, city_ctx, vistas_ctx, dataset, canvas_hw):
    """ny = 1 (canvas 64 x 200) and nx = 1 (canvas 100 x 128)."""
    ctx = city_ctx if dataset == "cityscapes" else vistas_ctx
    ys, xs = window_ref.synthetic_grid(canvas_hw)
    assert (len(ys), len(xs)) == ((1, 3) if canvas_hw == (64, 200) else (3, 1))
    _against_float64(ctx, dataset, 3.0, canvas_hw, (canvas_hw, (45, 77)), cuda)


# ---- error paths ---------------------------------------------------------------------------

def test_decisions_reject_bad_arguments(cuda, city_ctx):
    from seg_hip import LIB
    ctx = city_ctx
    lg = torch.zeros((2, 8, 16, 24), device=cuda)
    out = torch.full((2, 100, 200), -7, dtype=torch.int32, device=cuda)
    probs = torch.full((2, 100, 200, 24 + 1), -3.0, device=cuda)
    ident = MAPS["identity"]
    VP, INT = ctypes.c_void_p, ctypes.c_int

    def call(ptrs=None, low=(8, 16, 24), ys=(0, 36), xs=(0, 72), ny=None, nx=None, flip=0,
             canvas=(100, 200), cid_map=ident, rv=0, out_hw=(100, 200), probs_ptr=None,
             out_ptr=out.data_ptr(), null=()):
        n = max(len(ys), 1) * max(len(xs), 1) * (2 if flip == 1 else 1)
        ptrs = [lg.data_ptr()] * n if ptrs is None else ptrs
        arr = (VP * max(len(ptrs), 1))(*ptrs)
        ya, xa = (INT * max(len(ys), 1))(*ys), (INT * max(len(xs), 1))(*xs)
        m = (ctypes.c_int32 * len(cid_map))(*cid_map)
        return LIB.seg_window_decisions(
            ctx.h, None if "logits" in null else arr, low[0], low[1], low[2],
            None if "ys" in null else ya, len(ys) if ny is None else ny,
            None if "xs" in null else xa, len(xs) if nx is None else nx, flip,
            canvas[0], canvas[1], None if "map" in null else m, len(cid_map), rv,
            out_hw[0], out_hw[1], probs_ptr, out_ptr, None)
    assert call() == 0                       # the baseline call is valid
    assert call(flip=1) == 0
    torch.cuda.synchronize()
    assert int(out.min()) >= 0
    out.fill_(-7)
    p = lg.data_ptr()
    cases = {
        "null logits array": dict(null=("logits",)),
        "null logits entry": dict(ptrs=[p, p, None, p]),
        "null ys": dict(null=("ys",)),
        "null xs": dict(null=("xs",)),
        "null cid map": dict(null=("map",)),
        "null decisions": dict(out_ptr=None),
        "ny 0": dict(ny=0),
        "nx 0": dict(nx=0),
        "ny -1": dict(ny=-1),
        "65 entries": dict(ys=tuple(range(65)), xs=(0,), canvas=(128, 128), ptrs=[p] * 65),
        "33 x 1 windows with flip": dict(ys=tuple(range(33)), xs=(0,), canvas=(96, 128), flip=1,
                                         ptrs=[p] * 66),
        "h_low 0": dict(low=(0, 16, 24)),
        "w_low 0": dict(low=(8, 0, 24)),
        "ld below the channels": dict(low=(8, 16, 23)),
        "flip 2": dict(flip=2),
        "flip -1": dict(flip=-1),
        "replace_voids 2": dict(rv=2),
        "replace_voids 3": dict(rv=3),
        "replace_voids -1": dict(rv=-1),
        "canvas below the network height": dict(ys=(0,), canvas=(63, 200)),
        "canvas below the network width": dict(xs=(0,), canvas=(100, 127)),
        "ys not increasing": dict(ys=(0, 36, 36), canvas=(100, 200)),
        "ys decreasing": dict(ys=(0, 40, 36)),
        "ys[0] not 0": dict(ys=(1, 36)),
        "ys gap": dict(ys=(0, 65), canvas=(129, 200)),
        "ys last not flush": dict(ys=(0, 35)),
        "ys last past the canvas": dict(ys=(0, 37)),
        "xs not increasing": dict(xs=(0, 0, 72)),
        "xs[0] not 0": dict(xs=(2, 72)),
        "xs gap": dict(xs=(0, 129), canvas=(100, 257)),
        "xs last not flush": dict(xs=(0, 71)),
        "short cid map": dict(cid_map=ident[:-1]),
        "cid map entry -2": dict(cid_map=[-2] + ident[1:]),
        "out_h 0": dict(out_hw=(0, 200)),
        "out_w 0": dict(out_hw=(100, 0)),
        "misaligned mean": dict(probs_ptr=probs.data_ptr() + 4),
        "mean at another size": dict(probs_ptr=probs.data_ptr(), out_hw=(64, 128)),
    }
    for name, kw in cases.items():
        rc = call(**kw)
        msg = LIB.seg_last_error(ctx.h).decode()
        assert rc == -errno.EINVAL, (name, rc)
        assert "seg_window_decisions" in msg, (name, msg)
        if name == "replace_voids 2":
            assert "PREDICT order" in msg and "averaged" in msg
    arr = (VP * 1)(p)
    one = (INT * 1)(0)
    m = (ctypes.c_int32 * 20)(*ident)
    assert LIB.seg_window_decisions(None, arr, 8, 16, 24, one, 1, one, 1, 0, 64, 128, m, 20, 0, 64, 128,
                                    None, out.data_ptr(), None) == -errno.EINVAL
    assert b"seg_window_decisions" in LIB.seg_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((probs == -3.0).all())
    # the wrapper's own checks
    ys, xs = [0, 36], [0, 72]
    with pytest.raises(RuntimeError, match="averaged"):
        ctx.window_decisions([lg] * 4, ys, xs, False, (100, 200), ident, out, replace_voids=2)
    with pytest.raises(RuntimeError, match="seg_window_decisions"):
        ctx.window_decisions([lg] * 4, [0, 35], xs, False, (100, 200), ident, out)
    with pytest.raises(ValueError):
        ctx.window_decisions([lg] * 3, ys, xs, False, (100, 200), ident, out)           # count
    with pytest.raises(ValueError):
        ctx.window_decisions([lg] * 4, ys, xs, True, (100, 200), ident, out)            # count with flip
    with pytest.raises(ValueError):
        ctx.window_decisions([lg] * 65, list(range(65)), [0], False, (128, 128), ident, out)
    with pytest.raises(ValueError):
        ctx.window_decisions([lg, lg, lg, lg[:1]], ys, xs, False, (100, 200), ident, out)   # batch
    with pytest.raises(ValueError):
        ctx.window_decisions([lg, lg, lg, lg[:, :4].contiguous()], ys, xs, False, (100, 200), ident, out)
    with pytest.raises(ValueError):
        ctx.window_decisions([lg.double()] * 4, ys, xs, False, (100, 200), ident, out)
    with pytest.raises(ValueError):
        ctx.window_decisions([lg] * 4, ys, xs, False, (100, 200), ident, out.long())
    with pytest.raises(ValueError):
        ctx.window_decisions([lg] * 4, ys, xs, False, (100, 200), ident, out,
                             mean_probs=probs[..., :24])                                # not contiguous
    assert bool((out == -7).all())


# ---- the driver ----------------------------------------------------------------------------

def _settings(dtype):
    return argparse.Namespace(Nb=2, height_feature_extractor=64, width_feature_extractor=128,
                              per_pixel_dataset_name="cityscapes", compute_dtype=dtype,
                              pyramid="psp", name_feature_extractor="resnet_v1_50", init_seed=3,
                              window_canvas=[100, 200], window_stride=[24, 40], tta_flip=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_driver_entries_and_decisions(cuda, dtype):
    """Base 64 x 128, PSP, Nb = 2, canvas 100 x 200, stride (24, 40), flip: each entry's logits
    are bitwise those of the context's forward on that window alone, and the driver's decisions
    are the reference's on those native logits (teacher-forced)."""
    from estimator.mode_keys import ModeKeys
    from estimator.windows import driver_for_windows
    from input_pipelines.synthetic import batch
    from models.resnet50_extended_model_hierarchical import (Predictions, get_context, model,
                                                            release_contexts)
    from seg_hip import window_images
    release_contexts()
    s = _settings(dtype)
    primary = get_context(None, s, mode=ModeKeys.EVAL)
    _realistic_moving_stats(primary, torch.as_tensor(batch(99, 2, 0, 0, 64, 128)["images"]).to(cuda))
    x = torch.as_tensor(batch(12, 2, 0, 0, 100, 200)["images"]).to(cuda)
    before = primary.forward_count
    _, _, pred = model(ModeKeys.EVAL, x, None, None, s)          # runs no forward of its own
    assert primary.forward_count == before and isinstance(pred, Predictions)
    assert tuple(pred["decisions"].shape) == (2, 100, 200)
    drv = driver_for_windows(primary, None, s, ModeKeys.EVAL)
    assert drv is driver_for_windows(primary, None, s, ModeKeys.EVAL)
    assert (drv.ys, drv.xs, drv.flip) == ([0, 24, 36], [0, 40, 72], True)
    out = torch.full((2, 45, 77), -9, dtype=torch.int32, device=cuda)
    ents = drv.decisions(x, MAPS["merge"], out, replace_voids=True)
    assert primary.forward_count == before + 18
    assert len(ents) == 18 and all(tuple(t.shape) == (2, 8, 16, ents[0].shape[3]) for t in ents)
    place = window_ref.placements(drv.ys, drv.xs, True)
    assert drv.placements() == place
    for t, (y0, x0, flip) in zip(ents, place):
        primary.forward(window_images(x, y0, x0, 64, 128, flip))
        assert torch.equal(primary.outputs()[2], t), (y0, x0, flip)
    assert not torch.equal(ents[0], ents[1]) and not torch.equal(ents[0], ents[2])
    _, ref, _, _ = window_ref.window_reference([t.cpu().numpy() for t in ents], drv.ys, drv.xs, True,
                                               (64, 128), (100, 200), "cityscapes", MAPS["merge"],
                                               (45, 77), True, torch.float64)
    mism = float(np.mean(out.cpu().numpy() != ref))
    print(f"driver {dtype}: decisions differ from the reference on {mism:.2e}")
    assert mism <= 1e-3
    # the lazy predictions under sliding windows
    with pytest.raises(KeyError, match="sliding windows"):
        pred["l1_probabilities"]                       # nothing attached yet
    drv.attach(pred, ents)
    lo = 0
    for head, c in zip(("l1", "l2_vehicle", "l2_human"), (14, 7, 3)):
        p = pred[f"{head}_probabilities"]
        assert tuple(p.shape) == (2, 100, 200, c)
        np.testing.assert_allclose(p.sum(-1).cpu().numpy(), 1.0, atol=1e-5)
        assert torch.equal(pred[f"{head}_decisions"].long(), torch.argmax(p, dim=-1))
        for k in (f"{head}_logits", f"{head}_logits_lowres"):
            with pytest.raises(KeyError, match="sliding windows"):
                pred[k]
        lo += c
    assert "l1_logits" not in set(pred) and "l1_probabilities" in set(pred)
    # no other context was created
    from models import resnet50_extended_model_hierarchical as mm
    assert list(mm._CONTEXTS.values()) == [primary]
    release_contexts()


# ---- evaluate.py / predict.py --------------------------------------------------------------

EVAL_ARGS = ["--height_feature_extractor", "48", "--width_feature_extractor", "64",
             "--compute_dtype", "fp32"]
WIN_ARGS = ["--window_canvas", "72", "100", "--window_stride", "24", "36", "--tta_flip", "--replace_voids"]


def test_evaluate_one_window_changes_nothing(cuda, tmp_path, init_ckpt):
    """--window_canvas of the network size is one window: the plain run's confusion matrix."""
    from models.resnet50_extended_model_hierarchical import release_contexts
    ev = _script("evaluate")
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=1, dtype="fp32")
    base = [str(tmp_path), "2", PROBLEM, "cityscapes", "--Nb", "1"] + EVAL_ARGS
    plain = ev.main(base + ["--eval_res_dir", str(tmp_path / "a")])
    one = ev.main(base + ["--eval_res_dir", str(tmp_path / "b"), "--window_canvas", "48", "64"])
    assert len(plain) == len(one) == 1
    assert int(plain[0]["confusion_matrix"].sum()) > 0
    np.testing.assert_array_equal(one[0]["confusion_matrix"], plain[0]["confusion_matrix"])
    release_contexts()


def test_evaluate_with_windows_counts_every_labelled_pixel(cuda, tmp_path, init_ckpt):
    from input_pipelines.synthetic import images, pixel_labels
    from models.resnet50_extended_model_hierarchical import release_contexts
    ev = _script("evaluate")
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=2, dtype="fp32")
    release_contexts()
    res = ev.main([str(tmp_path), "2", PROBLEM, "cityscapes", "--Nb", "2"] + EVAL_ARGS + WIN_ARGS
                  + ["--eval_res_dir", str(tmp_path / "w")])
    # the one batch evaluate_input draws (seed 1234): images first, then the labels at the canvas
    rng = np.random.default_rng(1234)
    images(rng, 2, 72, 100)
    labels = pixel_labels(rng, 2, 72, 100)
    voids = int((labels == 19).sum())
    assert 0 < voids < labels.size
    cm = res[0]["confusion_matrix"]
    assert cm.shape == (19, 19)
    assert int(cm.sum()) == 2 * 72 * 100 - voids
    np.testing.assert_array_equal(cm.sum(1), np.bincount(labels.ravel(), minlength=20)[:19])
    release_contexts()


def test_predict_script_exports_with_windows(cuda, tmp_path, init_ckpt):
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
    n = pr.main([str(tmp_path), PROBLEM, str(pdir), "cityscapes", "--Nb", "2"] + EVAL_ARGS
                + ["--results_dir", str(rdir), "--export_lids_images", "--export_color_decisions"]
                + WIN_ARGS)
    assert n == 3
    for i in range(3):
        lids = np.asarray(Image.open(rdir / f"img{i}_result_lids.png"))
        col = np.asarray(Image.open(rdir / f"img{i}_result_color.png"))
        assert lids.shape == (50, 90) and col.shape == (50, 90, 3)
    release_contexts()
