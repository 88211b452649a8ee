"""Box-constrained pseudo-labels on the GPU (include/seg_hip.h at seg_box_constrain): the three
kernels against tests/boxlabel_ref.py, the composition with the CRF, the refusals of the entries,
estimator.pseudo.label_batch and pseudo_label.py.

The probabilities are 37 x 45 (1665 pixels: a ragged last block) in a 64 x 128 context, n = 2 and
n = 3 (the middle image without a box), sources 50 x 70 and 111 x 95, one image with 1024 boxes.

* cover: mask_out against seg_bbox_labels on the same box lists, exactly.
* constrain: copied channels bitwise, zeroed channels +0.0f, kept channels within 2e-6 relative of
  float64 (at most c2 - 2 additions, one reciprocal and one multiply, each rounding <= 2^-24, give
  < 1e-6, doubled), constrained heads summing to 1 within the same bound.
* decide, finalize: exact against the float32 reference on the device's own P'; twice the same.
"""
import errno
import json

import numpy as np
import pytest
import torch

import boxlabel_ref as R
import crf_ref
from inference_common import PROBLEM, _script, city_ctx, vistas_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

BOUND = 2e-6


def _ctx_of(dataset, city_ctx, vistas_ctx):
    return city_ctx if dataset == "cityscapes" else vistas_ctx


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


def _constrain(ctx, dataset, case, cuda, want_mask=True):
    """(P' numpy, mask uint16 numpy or None, uploaded boxes) of the case on the device."""
    P = R.probabilities(dataset, case)
    boxes = ctx.upload_boxes(R.box_lists(case), R.HW)
    out = torch.full(P.shape, -2.0, device=cuda)
    mask = torch.full(P.shape[:3], -1, dtype=torch.int16, device=cuda) if want_mask else None
    ctx.box_constrain(_dev(P, cuda), boxes, out, mask_out=mask)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (mask.cpu().numpy().view(np.uint16) if want_mask else None), boxes


def _decide(ctx, q, boxes, tau, cuda, conf=True):
    n, H, W, _ = q.shape
    labels = torch.full((n, H, W), -9, dtype=torch.int32, device=cuda)
    cf = torch.full((n, H, W), -1.0, device=cuda) if conf else None
    counts = torch.full((max(boxes.total, 1), 2), -5, dtype=torch.int32, device=cuda)   # the entry zeroes it
    ctx.box_decisions(_dev(q, cuda), boxes, tau, labels, counts, conf_out=cf)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), (cf.cpu().numpy() if conf else None), counts.cpu().numpy()[:boxes.total]


# ---- 1. cover ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["n2", "n3"])
def test_mask_is_the_cover_of_seg_bbox_labels(cuda, city_ctx, case):
    from input_pipelines.weak_labels import BboxLabelsGPU
    _, mask, _ = _constrain(city_ctx, "cityscapes", case, cuda)
    soft = BboxLabelsGPU(R.HW[0], R.HW[1], cuda).bbox(R.box_lists(case)).cpu().numpy()
    for k in range(14):
        np.testing.assert_array_equal((mask >> np.uint16(k)) & np.uint16(1) > 0, soft[..., k] > 0, str(k))
    assert not (mask >> np.uint16(14)).any()
    np.testing.assert_array_equal(mask, R.case_cover(case)[1])
    assert mask.any() and not mask.all()
    if case == "n3":
        assert not mask[1].any()


@pytest.mark.parametrize("dataset", ["cityscapes", "vistas"])
def test_box_kinds_are_the_reference_tables(cuda, city_ctx, vistas_ctx, dataset):
    from seg_hip import LIB
    ctx = _ctx_of(dataset, city_ctx, vistas_ctx)
    assert ctx.box_kinds() == R.box_kinds(dataset)
    assert LIB.seg_box_kinds(ctx.h, None) == -errno.EINVAL and b"kinds" in LIB.seg_last_error(ctx.h)
    assert LIB.seg_box_kinds(None, None) == -errno.EINVAL and b"seg_box_kinds" in LIB.seg_last_error(None)


# ---- 2. constrain --------------------------------------------------------------------------------

@pytest.mark.parametrize("dataset,case", R.CASES)
def test_constrain(cuda, city_ctx, vistas_ctx, dataset, case):
    ctx = _ctx_of(dataset, city_ctx, vistas_ctx)
    c1, c2, c3 = crf_ref.WIDTHS[dataset]
    P = R.probabilities(dataset, case)
    got, mask, _ = _constrain(ctx, dataset, case, cuda)
    np.testing.assert_array_equal(mask, R.case_cover(case)[1])
    ref = R.reference(dataset, case, np.float64)["constrained"]
    av, ah = R.allowed(mask, dataset)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    np.testing.assert_array_equal(bits(got[..., :c1]), bits(P[..., :c1]))           # l1: bit for bit
    for lo, c, a in ((c1, c2, av), (c1 + c2, c3, ah)):
        g, p, r = got[..., lo:lo + c], P[..., lo:lo + c], ref[..., lo:lo + c]
        free = ~a.any(-1)
        assert free.any() and (~free).any()
        np.testing.assert_array_equal(bits(g[free]), bits(p[free]))                 # unconstrained: bit for bit
        zeroed = ~a & ~free[..., None]
        assert zeroed.any() and not bits(g[zeroed]).any()                           # exactly +0.0f
        kept = a & ~free[..., None]
        err = np.abs(g[kept].astype(np.float64) - r[kept]) / r[kept]
        sums = g[~free].astype(np.float64).sum(-1)
        print(f"{dataset} {case} head at {lo}: kept channels within {err.max():.3e} relative of float64, "
              f"sums within {np.abs(sums - 1).max():.3e} of 1")
        assert err.max() <= BOUND
        assert np.abs(sums - 1).max() <= BOUND


# ---- 3. decide -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dataset,case", R.CASES)
def test_decide_is_the_float32_reference_on_the_device_probabilities(cuda, city_ctx, vistas_ctx, dataset, case):
    ctx = _ctx_of(dataset, city_ctx, vistas_ctx)
    q, mask, boxes = _constrain(ctx, dataset, case, cuda)
    items = R.box_lists(case)
    cv, _ = R.case_cover(case)
    for tau in (R.TAU, 0.0):
        labels, conf, counts = _decide(ctx, q, boxes, tau, cuda)
        rl, rc, rn = R.decide(q, items, cv, mask, dataset, tau, np.float32)
        np.testing.assert_array_equal(labels, rl)
        np.testing.assert_array_equal(conf.view(np.uint32), rc.view(np.uint32))
        np.testing.assert_array_equal(counts, rn)
        again = _decide(ctx, q, boxes, tau, cuda, conf=False)
        np.testing.assert_array_equal(again[0], labels)
        np.testing.assert_array_equal(again[2], counts)
    ignore = crf_ref.N_PP[dataset] - 1
    assert (labels == ignore).any() and (labels != ignore).any() and counts[:, 1].any()
    # the labels of the whole float32 chain are the reference's too
    np.testing.assert_array_equal(_decide(ctx, q, boxes, R.TAU, cuda, conf=False)[0],
                                  R.reference(dataset, case, np.float64)["labels"])


# ---- 4. finalize ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dataset,case", R.CASES)
def test_finalize(cuda, city_ctx, vistas_ctx, dataset, case):
    ctx = _ctx_of(dataset, city_ctx, vistas_ctx)
    ref = R.reference(dataset, case, np.float32)
    cv, _ = R.case_cover(case)
    boxes = ctx.upload_boxes(R.box_lists(case), R.HW)
    labels = _dev(ref["labels"], cuda)
    ignore = crf_ref.N_PP[dataset] - 1
    for name, rj in (("hand-made", R.hand_reject(case)), ("min_fill", ref["reject"]),
                     ("none", np.zeros_like(ref["reject"]))):
        rj = np.asarray(rj, np.int32)
        rd = torch.zeros(max(boxes.total, 1), dtype=torch.int32, device=cuda)
        rd[:len(rj)] = _dev(rj, cuda)
        for hw in R.OUT_SIZES:
            out = torch.full((len(cv),) + hw, -9, dtype=torch.int32, device=cuda)
            ctx.box_finalize(labels, boxes, rd, out)
            want = R.finalize(ref["labels"], cv, rj, hw, dataset)
            np.testing.assert_array_equal(out.cpu().numpy(), want, f"{name} {hw}")
            if name == "min_fill":
                np.testing.assert_array_equal(want, ref["final"][hw])
        if name != "none":
            assert ((want == ignore) & (R.finalize(ref["labels"], cv, 0 * rj, hw, dataset) != ignore)).any()


# ---- 5. composition with the CRF -----------------------------------------------------------------

@pytest.mark.parametrize("dataset", ["cityscapes", "vistas"])
@pytest.mark.parametrize("rdt", [(1, 1, 1), (3, 1, 3)])
def test_crf_keeps_the_zeros_of_the_constraint(cuda, city_ctx, vistas_ctx, dataset, rdt):
    from seg_hip import CrfParams, crf_workspace_bytes
    ctx = _ctx_of(dataset, city_ctx, vistas_ctx)
    case = "n2"
    r, d, T = rdt
    q0, mask, boxes = _constrain(ctx, dataset, case, cuda)
    n, H, W, ct = q0.shape
    I = crf_ref.synthetic_inputs(dataset, n, R.HW)[1]
    qt = torch.full(q0.shape, -2.0, device=cuda)
    scratch = torch.empty((n, H, W), dtype=torch.int32, device=cuda)
    ws = torch.empty(crf_workspace_bytes(n, H, W, ct), dtype=torch.uint8, device=cuda)
    ctx.crf_decisions(_dev(q0, cuda), _dev(I, cuda),
                      CrfParams(T, r, d, *crf_ref.DEFAULT_WEIGHTS, *crf_ref.DEFAULT_THETAS),
                      crf_ref.IDENTITY_MAP[dataset], scratch, workspace=ws, probs_out=qt)
    torch.cuda.synchronize()
    qt = qt.cpu().numpy()
    zero = q0 == 0
    assert zero.any() and not qt[zero].view(np.uint32).any()          # exactly zero after T steps
    assert crf_ref.rel(qt, q0) > 1e-3                                  # the refinement moved something
    labels, _, counts = _decide(ctx, qt, boxes, R.TAU, cuda)
    rl, _, rn = R.decide(qt, R.box_lists(case), R.case_cover(case)[0], mask, dataset, R.TAU, np.float32)
    np.testing.assert_array_equal(labels, rl)
    np.testing.assert_array_equal(counts, rn)


# ---- 6. refusals ---------------------------------------------------------------------------------

def test_entries_reject_bad_arguments(cuda, city_ctx):
    from seg_hip import LIB
    ctx = city_ctx
    n, H, W, ct = 2, 20, 24, 24
    b = ctx.upload_boxes(R.box_lists("n3")[:2], R.HW)     # the device arrays; sizes are the call's own
    probs = torch.full((n, H, W, ct + 1), 1.0 / 14, device=cuda)      # room for a misaligned view
    pout = torch.full((n, H, W, ct + 1), -3.0, device=cuda)
    mask = torch.full((n, H, W), -3, dtype=torch.int16, device=cuda)
    labels = torch.full((n, H, W), -7, dtype=torch.int32, device=cuda)
    conf = torch.full((n, H, W), -3.0, device=cuda)
    counts = torch.full((b.total, 2), -7, dtype=torch.int32, device=cuda)
    reject = torch.zeros(b.total, dtype=torch.int32, device=cuda)
    fin = torch.full((n, 30, 40), -7, dtype=torch.int32, device=cuda)
    lists = dict(boxes=b.boxes.data_ptr(), cids=b.cids.data_ptr(), box_off=b.box_off.data_ptr(),
                 geom=b.geom.data_ptr(), max_boxes=b.max_boxes)

    def constrain(ctx_h=ctx.h, probs_ptr=probs.data_ptr(), nhw=(n, H, W), pout_ptr=pout.data_ptr(), **kw):
        a = dict(lists, **kw)
        return LIB.seg_box_constrain(ctx_h, probs_ptr, *nhw, a["boxes"], a["cids"], a["box_off"], a["geom"],
                                     a["max_boxes"], pout_ptr, mask.data_ptr(), None)

    def decide(ctx_h=ctx.h, q_ptr=probs.data_ptr(), nhw=(n, H, W), tau=0.5, labels_ptr=labels.data_ptr(),
               counts_ptr=counts.data_ptr(), **kw):
        a = dict(lists, **kw)
        return LIB.seg_box_decisions(ctx_h, q_ptr, *nhw, a["boxes"], a["cids"], a["box_off"], a["geom"],
                                     a["max_boxes"], tau, labels_ptr, conf.data_ptr(), counts_ptr, None)

    def finalize(ctx_h=ctx.h, labels_ptr=labels.data_ptr(), nhw=(n, H, W), reject_ptr=reject.data_ptr(),
                 out_hw=(30, 40), out_ptr=fin.data_ptr(), **kw):
        a = dict(lists, **kw)
        return LIB.seg_box_finalize(ctx_h, labels_ptr, *nhw, a["boxes"], a["cids"], a["box_off"], a["geom"],
                                    a["max_boxes"], reject_ptr, *out_hw, out_ptr, None)

    assert constrain() == 0 and decide() == 0 and finalize() == 0      # the baseline calls are valid
    torch.cuda.synchronize()
    assert int(labels.min()) >= 0 and int(counts.min()) >= 0 and int(fin.min()) >= 0
    for t, v in ((pout, -3.0), (mask, -3), (labels, -7), (conf, -3.0), (counts, -7), (fin, -7)):
        t.fill_(v)
    shared = {
        "null boxes": (dict(boxes=None), "boxes"), "null cids": (dict(cids=None), "cids"),
        "null box_off": (dict(box_off=None), "box_off"), "null geom": (dict(geom=None), "geom"),
        "n 0": (dict(nhw=(0, H, W)), "n ="), "H 0": (dict(nhw=(n, 0, W)), "H ="),
        "W -1": (dict(nhw=(n, H, -1)), "W ="),
        "max_boxes 1025": (dict(max_boxes=1025), "max_boxes"), "max_boxes -1": (dict(max_boxes=-1), "max_boxes"),
    }
    nan, inf = float("nan"), float("inf")
    own = {
        "seg_box_constrain": (constrain, {
            "null probs": (dict(probs_ptr=None), "probs"), "null probs_out": (dict(pout_ptr=None), "probs_out"),
            "misaligned probs": (dict(probs_ptr=probs.data_ptr() + 4), "probs"),
            "misaligned probs_out": (dict(pout_ptr=pout.data_ptr() + 4), "probs_out"),
            "probs_out is probs": (dict(pout_ptr=probs.data_ptr()), "probs_out")}),
        "seg_box_decisions": (decide, {
            "null q": (dict(q_ptr=None), "q"), "null labels_out": (dict(labels_ptr=None), "labels_out"),
            "null counts_out": (dict(counts_ptr=None), "counts_out"),
            "misaligned q": (dict(q_ptr=probs.data_ptr() + 4), "q"),
            "tau nan": (dict(tau=nan), "tau"), "tau inf": (dict(tau=inf), "tau"),
            "tau < 0": (dict(tau=-0.01), "tau"), "tau > 1": (dict(tau=1.01), "tau")}),
        "seg_box_finalize": (finalize, {
            "null labels": (dict(labels_ptr=None), "labels"), "null reject": (dict(reject_ptr=None), "reject"),
            "null out": (dict(out_ptr=None), "out"),
            "out_h 0": (dict(out_hw=(0, 40)), "out_h"), "out_w 0": (dict(out_hw=(30, 0)), "out_w")}),
    }
    for fn, (call, cases) in own.items():
        for name, (kw, word) in dict(shared, **cases).items():
            rc = call(**kw)
            msg = LIB.seg_last_error(ctx.h).decode()
            assert rc == -errno.EINVAL, (fn, name, rc)
            assert fn in msg and word in msg, (fn, name, msg)
        assert call(ctx_h=None) == -errno.EINVAL
        assert fn.encode() in LIB.seg_last_error(None) and b"ctx" in LIB.seg_last_error(None)
    torch.cuda.synchronize()
    for t, v in ((pout, -3.0), (mask, -3), (labels, -7), (conf, -3.0), (counts, -7), (fin, -7)):
        assert bool((t == v).all())
    # the wrapper's own checks
    p4 = probs[..., :ct].contiguous()
    with pytest.raises(ValueError, match="box lists of 2 images for 37x45"):
        ctx.box_constrain(p4, b, torch.empty_like(p4))                    # boxes uploaded for another size
    with pytest.raises(ValueError):
        ctx.box_constrain(probs[..., :ct], R.box_lists("n3")[:2], torch.empty_like(p4))   # not contiguous
    with pytest.raises(ValueError, match="flipped"):
        ctx.upload_boxes([R.box_lists("n3")[0] + (1,)], R.HW)
    first = R.box_lists("n3")[0]
    with pytest.raises(ValueError, match="class ids"):
        ctx.upload_boxes([(np.array([14]), first[1][:1]) + first[2:]], R.HW)
    here = ctx.upload_boxes([it[:3] + ((H, W), (0, 0)) for it in R.box_lists("n3")[:2]], (H, W))
    with pytest.raises(RuntimeError, match="tau"):
        ctx.box_decisions(p4, here, 2.0, labels, counts)
    assert bool((labels == -7).all())


# ---- 7. label_batch ------------------------------------------------------------------------------

SOURCES = {
    # extra settings, (height, width) of the prepared batch, forwards beyond model_fn's
    "single": ({}, (64, 128), 0),
    "flip": (dict(tta_flip=True), (64, 128), 1),
    "windows": (dict(window_canvas=[64, 200], window_stride=[24, 40]), (64, 200), 3),   # xs 0, 40, 72
}
E2E_TAU, E2E_MIN_FILL = 0.1, 0.02


def _e2e_boxlists():
    hand = R.box_lists("n3")
    return [(hand[0][0], hand[0][1], (111, 95)), (hand[2][0], hand[2][1], (50, 70))]


@pytest.fixture(scope="module")
def shared_contexts():
    from models.resnet50_extended_model_hierarchical import release_contexts
    release_contexts()
    yield
    release_contexts()


@pytest.mark.parametrize("crf", [0, 2])
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_label_batch_is_the_low_level_sequence_bitwise(cuda, shared_contexts, source, crf):
    import argparse
    from estimator.crf import crf_settings
    from estimator.define_estimator_hierarchical import _predict_spec
    from estimator.inference import decide_batch
    from estimator.mode_keys import ModeKeys
    from estimator.pseudo import label_batch
    from estimator.tta import driver_for
    from estimator.windows import driver_for_windows
    from inference_common import _realistic_moving_stats
    from input_pipelines.synthetic import batch
    from input_pipelines.weak_labels import BoxLists
    from models.resnet50_extended_model_hierarchical import get_context, model
    from seg_hip import CrfParams, crf_workspace_bytes, resize_images, window_images
    extra, hw, forwards = SOURCES[source]
    s = argparse.Namespace(Nb=2, height_feature_extractor=64, width_feature_extractor=128,
                           per_pixel_dataset_name="cityscapes", compute_dtype="fp32", pyramid="psp",
                           name_feature_extractor="resnet_v1_50", init_seed=3, crf_iterations=crf,
                           crf_radius=1, pseudo_tau=E2E_TAU, pseudo_min_fill=E2E_MIN_FILL,
                           output_Nclasses=20, **extra)
    mode = ModeKeys.PREDICT
    ctx = get_context(None, s, mode=mode)
    if not getattr(ctx, "_realistic", False):     # once per context: logits of a trained range
        _realistic_moving_stats(ctx, torch.as_tensor(batch(99, 2, 0, 0, 64, 128)["images"]).to(cuda))
        ctx._realistic = True
    x = torch.as_tensor(batch(12, 2, 0, 0, *hw)["images"]).to(cuda)
    tta, win = driver_for(ctx, None, s, mode), driver_for_windows(ctx, None, s, mode)
    assert (tta is not None, win is not None) == (source == "flip", source == "windows")
    contexts = {id(c): c for c in [ctx] + (tta.contexts if tta else [])}.values()
    count = lambda: sum(getattr(c, "forward_count", 0) for c in contexts)
    boxlists = _e2e_boxlists()

    _, _, pred = model(mode, x, None, None, s)
    before = count()
    got = torch.full((2, 45, 77), -9, dtype=torch.int32, device=cuda)
    out, report = label_batch(pred, x, boxlists, ctx, None, s, got)
    assert out is got and count() - before == forwards
    lazy_probs = torch.cat([pred[f"{h}_probabilities"] for h in ("l1", "l2_vehicle", "l2_human")], -1)

    # the same sequence of low-level calls
    model(mode, x, None, None, s)
    probs = torch.full((2,) + hw + (24,), -1.0, device=cuda)
    at_size = torch.empty((2,) + hw, dtype=torch.int32, device=cuda)
    if source == "single":
        ctx.full_predictions(probs=probs)
    elif source == "flip":
        ents = []
        for c in tta.contexts:
            for flip in (False, True):
                if c is not ctx or flip:
                    c.forward(resize_images(x, c.cfg.height, c.cfg.width, flip))
                ents.append((c.outputs()[2].clone(), flip))
        ctx.tta_decisions(ents, list(range(20)), at_size, mean_probs=probs)
    else:
        ents = []
        for x0 in (0, 40, 72):
            ctx.forward(window_images(x, 0, x0, 64, 128, False))
            ents.append(ctx.outputs()[2].clone())
        ctx.window_decisions(ents, [0], [0, 40, 72], False, (64, 200), list(range(20)), at_size, mean_probs=probs)
    items = BoxLists((c, xy, src, hw, (0, 0)) for c, xy, src in boxlists)
    b = ctx.upload_boxes(items, hw)
    q = torch.full_like(probs, -2.0)
    ctx.box_constrain(probs, b, q)
    if crf:
        refined = torch.full_like(probs, -3.0)
        ws = torch.empty(crf_workspace_bytes(2, hw[0], hw[1], 24), dtype=torch.uint8, device=cuda)
        ctx.crf_decisions(q, x, CrfParams(*crf_settings(s)), list(range(20)), at_size, workspace=ws,
                          probs_out=refined)
        q = refined
    labels = torch.empty((2,) + hw, dtype=torch.int32, device=cuda)
    counts = torch.empty((b.total, 2), dtype=torch.int32, device=cuda)
    ctx.box_decisions(q, b, E2E_TAU, labels, counts)
    counts = counts.cpu().numpy()
    rj = R.rejects(counts, R.all_cids(items), "cityscapes", E2E_MIN_FILL)
    want = torch.full((2, 45, 77), -7, dtype=torch.int32, device=cuda)
    ctx.box_finalize(labels, b, _dev(rj, cuda), want)
    assert torch.equal(got, want)
    assert torch.equal(lazy_probs, q)                  # the lazy probabilities are what was decided on
    w = want.cpu().numpy()
    print(f"{source} crf {crf}: labelled {float((w != 19).mean()):.3f}, rejected {int(rj.sum())} of {len(rj)} boxes")
    assert (w == 19).any() and (w != 19).any() and w.min() >= 0 and w.max() <= 19
    flat = [bx for rep in report for bx in rep["boxes"]]
    assert [(bx["class"], bx["area"], bx["hit"], int(bx["rejected"])) for bx in flat] == \
        [(int(c), int(a), int(h), int(r)) for c, (a, h), r in zip(R.all_cids(items), counts, rj)]
    assert [rep["labelled"] for rep in report] == pytest.approx([float((w[i] != 19).mean()) for i in range(2)])

    # the PREDICT spec: with 'boxlists' the decisions are label_batch's, without the key nothing changes
    _, _, pred = model(mode, x, None, None, s)
    spec = _predict_spec(pred, {"proimages": x, "boxlists": boxlists}, s, None)
    assert tuple(spec.predictions["decisions"].shape) == (2,) + hw
    plain = torch.full((2,) + hw, -7, dtype=torch.int32, device=cuda)
    ctx.box_finalize(labels, b, _dev(rj, cuda), plain)
    assert torch.equal(spec.predictions["decisions"], plain)
    assert spec.predictions["pseudo_report"][0]["boxes"] == report[0]["boxes"]
    _, _, pred = model(mode, x, None, None, s)
    spec = _predict_spec(pred, {"proimages": x}, s, None)
    _, _, pred = model(mode, x, None, None, s)
    direct = torch.full((2,) + hw, -7, dtype=torch.int32, device=cuda)
    decide_batch(pred, x, ctx, None, s, mode, list(range(20)), direct, False, order="predict")
    assert torch.equal(spec.predictions["decisions"], direct)
    assert "pseudo_report" not in spec.predictions


# ---- 8. pseudo_label.py --------------------------------------------------------------------------

EVAL_ARGS = ["--height_feature_extractor", "48", "--width_feature_extractor", "64",
             "--compute_dtype", "fp32"]


def _write_jpegs(folder, sizes, seed):
    from PIL import Image
    from oracle.tfseg import resize_bilinear_ac
    rng = np.random.default_rng(seed)
    folder.mkdir()
    for i, (h, w) in enumerate(sizes):     # smooth images: JPEG-friendly, and not one flat colour
        coarse = torch.as_tensor(rng.uniform(0, 255, (1, 3, 4, 5)))
        img = resize_bilinear_ac(coarse, h, w)[0].permute(1, 2, 0).numpy()
        Image.fromarray(img.astype(np.uint8)).save(folder / f"img{i}.jpg", quality=95)


def test_pseudo_label_script(cuda, tmp_path, init_ckpt, monkeypatch):
    import estimator.pseudo as pseudo
    import seg_hip
    from estimator.pseudo import label_id_palette
    from input_pipelines.tfrecords import parse_cityscapes_example, read_records
    from models.resnet50_extended_model_hierarchical import release_contexts
    sizes = [(48, 64), (96, 128), (96, 128)]       # a size change closes the first batch of --Nb 2
    _write_jpegs(tmp_path / "in", sizes, 8)
    hand = R.box_lists("n3")[0]
    from input_pipelines.train_inputs import MID2CID
    mids = {v: k for k, v in MID2CID.items()}
    index = {f"img{i}": [[mids[int(c)], [float(v) for v in xy]] for c, xy in zip(hand[0], hand[1])]
                        + [["/m/unknown", [0.1, 0.2, 0.1, 0.2]]] for i in range(3)}
    index["img1"] = []
    (tmp_path / "boxes.json").write_text(json.dumps(index))
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=2, dtype="fp32")
    release_contexts()

    batches, entry_counts = [], []
    real_label_batch, real_decisions = pseudo.label_batch, seg_hip.SegContext.box_decisions

    def spy_label_batch(*a, **k):
        out, report = real_label_batch(*a, **k)
        batches.append((out.cpu().numpy().copy(), report))
        return out, report

    def spy_decisions(self, q, boxes, tau, labels_out, counts_out, **k):
        b = real_decisions(self, q, boxes, tau, labels_out, counts_out, **k)
        entry_counts.append(counts_out.cpu().numpy()[:b.total].copy())
        return b
    monkeypatch.setattr(pseudo, "label_batch", spy_label_batch)
    monkeypatch.setattr(seg_hip.SegContext, "box_decisions", spy_decisions)

    pl = _script("pseudo_label")
    out_path = tmp_path / "pseudo.tfrecord"
    base = [str(tmp_path), PROBLEM, str(tmp_path / "in")]
    tail = ["cityscapes", "--Nb", "2"] + EVAL_ARGS
    n = pl.main(base + [str(tmp_path / "boxes.json"), str(out_path)] + tail
                + ["--pseudo_tau", "0.08", "--pseudo_min_fill", "0.02"])
    assert n == 3 and len(batches) == 2
    assert [b[0].shape for b in batches] == [(2, 48, 64), (2, 96, 128)]
    pal = label_id_palette(json.load(open(PROBLEM)))
    want = [batches[0][0][0], batches[1][0][0], batches[1][0][1]]       # the padded copy is dropped
    recs = list(read_records(str(out_path)))
    assert len(recs) == 3
    from PIL import Image
    for i, rec in enumerate(recs):
        im, la, ip, lp = parse_cityscapes_example(rec)
        np.testing.assert_array_equal(im, np.asarray(Image.open(tmp_path / "in" / f"img{i}.jpg").convert("RGB")))
        np.testing.assert_array_equal(la, pal[want[i]])
        assert ip.decode().endswith(f"img{i}.jpg") and lp == f"img{i}_pseudo_lids.png".encode()
    report = json.load(open(str(out_path) + ".report.json"))
    assert sorted(report) == ["img0", "img1", "img2"] and report["img1"]["boxes"] == []
    k = len(hand[0])
    got_counts = [[(bx["area"], bx["hit"]) for bx in report[f"img{i}"]["boxes"]] for i in (0, 2)]
    assert len(entry_counts) == 2 and [len(c) for c in entry_counts] == [2 * k, k]
    assert got_counts[0] == [tuple(r) for r in entry_counts[0][:k].tolist()]       # batch 1: img0 and its copy
    assert got_counts[1] == [tuple(r) for r in entry_counts[1].tolist()]           # batch 2: img1 (no box), img2
    assert any(a > 0 for a, _ in got_counts[0])
    assert 0.0 < report["img0"]["labelled"] <= 1.0

    # without boxes and with both thresholds off the labels are the model's own decisions wherever
    # they are not void: evaluate.py on the written file sees no off-diagonal mass
    release_contexts()
    (tmp_path / "none.json").write_text(json.dumps({f"img{i}": [] for i in range(3)}))
    own = tmp_path / "own.tfrecord"
    assert pl.main(base + [str(tmp_path / "none.json"), str(own)] + tail) == 3
    release_contexts()
    ev = _script("evaluate")
    res = ev.main([str(tmp_path), "3", PROBLEM, "cityscapes", "--Nb", "1"] + EVAL_ARGS
                  + ["--tfrecords_path", str(own), "--eval_res_dir", str(tmp_path / "ev")])
    cm = np.asarray(res[0]["confusion_matrix"])
    print("evaluate on the model's own pseudo-labels: diagonal", int(np.trace(cm)), "of", int(cm.sum()))
    assert cm.sum() > 0 and np.trace(cm) == cm.sum()
    release_contexts()
