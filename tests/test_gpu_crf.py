"""Mean-field CRF refinement on the GPU (include/seg_hip.h at seg_crf_decisions): the step
kernel, the decision kernel, the host driver and the evaluate.py / predict.py flags.

* T = 0 is the existing head: on mean_probs_out of seg_tta_decisions for one unflipped entry the
  decisions are bitwise seg_tta_decisions' and probs_out is a bitwise copy.
* parity with float64 (tests/crf_ref.py) on every case of crf_ref.CASES, both datasets: Q^T within
  1e-5 norm-relative (the bound tests/test_gpu_tta.py holds the decision head's __expf softmax
  arithmetic to; tests/test_crf_host.py shows the reference's own float32 share is <= 4.9e-7),
  decisions differing on <= 1e-3 of the pixels (the reference's own share is 0). The inputs are
  37 x 45 in a 64 x 128 context: the entry takes its size from its arguments.
* geometry: a 5 x 3 image at r * d = 20, and N = 2 at 64 x 128 with image 1 from another seed.
* every refusal of the C entry, with decisions_out unwritten.
* evaluate.py / predict.py with --crf_iterations alone, with --tta_flip and with --window_canvas.
* estimator.inference.decide_batch, the one path of both specs, for {one forward, TTA, windows} x
  {CRF off, on} x {EVAL, PREDICT}: decisions bitwise those of the same low-level calls made by
  hand, the same number of forwards, the lazy predictions' key sets and KeyError texts.
"""
import ctypes
import errno

import numpy as np
import pytest
import torch

import crf_ref
import tta_ref
from inference_common import (MAPS, PROBLEM, _script, city_ctx, vistas_ctx)  # noqa: F401

pytestmark = pytest.mark.gpu

DATASETS = ["cityscapes", "vistas"]
ALL_MAPS = {
    "cityscapes": MAPS,
    "vistas": {"identity": crf_ref.IDENTITY_MAP["vistas"],
               "merge": [i // 3 for i in range(65)] + [-1]},
}


def _params(T, r=3, d=1, weights=crf_ref.DEFAULT_WEIGHTS, thetas=crf_ref.DEFAULT_THETAS):
    from seg_hip import CrfParams
    return CrfParams(T, r, d, *weights, *thetas)


def _workspace(n, H, W, ct, cuda):
    from seg_hip import crf_workspace_bytes
    nbytes = crf_workspace_bytes(n, H, W, ct)
    assert nbytes >= 2 * n * H * W * ct * 4 and nbytes % 16 == 0
    return torch.empty(nbytes, dtype=torch.uint8, device=cuda)


def _ctx_of(dataset, city_ctx, vistas_ctx):
    return city_ctx if dataset == "cityscapes" else vistas_ctx


def _run(ctx, P, I, case, cid_map, out_hw, rv, cuda, want_probs=True):
    """seg_crf_decisions on host arrays; returns (decisions, Q^T or None) as numpy."""
    r, d, T = case
    n, H, W, ct = P.shape
    pd, im = torch.from_numpy(np.array(P)).to(cuda), torch.from_numpy(np.array(I)).to(cuda)
    out = torch.full((n,) + tuple(out_hw), -9, dtype=torch.int32, device=cuda)
    q = torch.full((n, H, W, ct), -2.0, device=cuda) if want_probs else None
    ctx.crf_decisions(pd, im, _params(T, r, d), cid_map, out, replace_voids=rv,
                      workspace=_workspace(n, H, W, ct, cuda), probs_out=q)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (q.cpu().numpy() if want_probs else None)


# ---- T = 0: the existing head, bit for bit -------------------------------------------------------

@pytest.mark.parametrize("dataset", DATASETS)
@pytest.mark.parametrize("mapname", ["identity", "merge"])
def test_zero_iterations_is_the_tta_head_bitwise(cuda, city_ctx, vistas_ctx, dataset, mapname):
    ctx = _ctx_of(dataset, city_ctx, vistas_ctx)
    ct = sum(crf_ref.WIDTHS[dataset])
    cid_map = ALL_MAPS[dataset][mapname]
    if dataset == "cityscapes":
        lg = ctx.outputs()[2]           # the context's own logits of its last forward
        assert float(lg.std()) > 1e-3 and bool(torch.isfinite(lg).all())
    else:                               # a context without weights: seeded synthetic logits
        lg = torch.from_numpy(tta_ref.synthetic_entries("vistas", 3.0)[4][0]).to(cuda)
    images = torch.rand((2, 64, 128, 3), device=cuda) * 2 - 1
    mean = torch.full((2, 64, 128, ct), -1.0, device=cuda)
    at_net = torch.empty((2, 64, 128), dtype=torch.int32, device=cuda)
    ctx.tta_decisions([(lg, False)], cid_map, at_net, mean_probs=mean)
    for rv in (False, True):
        for out_hw in ((64, 128), (45, 77), (128, 256)):
            want = torch.full((2,) + out_hw, -7, dtype=torch.int32, device=cuda)
            ctx.tta_decisions([(lg, False)], cid_map, want, replace_voids=rv)
            got = torch.full((2,) + out_hw, -9, dtype=torch.int32, device=cuda)
            copy = torch.full((2, 64, 128, ct), -2.0, device=cuda)
            ctx.crf_decisions(mean, images, _params(0), cid_map, got, replace_voids=rv, probs_out=copy)
            assert int(want.min()) >= 0
            assert torch.equal(got, want), (rv, out_hw)
            assert torch.equal(copy, mean)
    assert len(torch.unique(at_net)) > 1


# ---- parity with float64 -------------------------------------------------------------------------

def _parity(ctx, dataset, which, case, cuda):
    inputs = {"synthetic": crf_ref.synthetic_inputs, "tiny": crf_ref.tiny_inputs,
              "two_seed": crf_ref.two_seed_inputs}[which]
    P, I = inputs(dataset)
    H, W = P.shape[1:3]
    assert (H, W) != (ctx.cfg.height, ctx.cfg.width) or which == "two_seed"
    q64 = crf_ref.reference(dataset, case, np.float64, which)
    cid_map = crf_ref.IDENTITY_MAP[dataset]
    figures = []
    for rv in (False, True):
        for out_hw in ((H, W), (2 * H + 1, W - 1)):
            d, q = _run(ctx, P, I, case, cid_map, out_hw, rv, cuda)
            d64 = crf_ref.decisions(q64, dataset, cid_map, out_hw, rv)
            rel = crf_ref.rel(q, q64)
            mism = float(np.mean(d != d64))
            print(f"{dataset} {which} {H}x{W} (r, d, T) = {case} rv {rv} out {out_hw}: Q^T {rel:.2e} "
                  f"norm-relative, decisions differ on {mism:.2e}")
            figures.append((d, q, d64, rel, mism))
    for d, q, d64, rel, mism in figures:
        assert d.min() >= 0 and np.isfinite(q).all()
        assert rel <= 1e-5
        assert mism <= 1e-3
    return figures


@pytest.mark.parametrize("dataset", DATASETS)
@pytest.mark.parametrize("case", crf_ref.CASES)
def test_parity_with_float64(cuda, city_ctx, vistas_ctx, dataset, case):
    """N = 2, 37 x 45 (odd, ragged against the tile, below twice the largest halo) in a 64 x 128
    context."""
    _parity(_ctx_of(dataset, city_ctx, vistas_ctx), dataset, "synthetic", case, cuda)


# ---- geometry ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dataset", DATASETS)
def test_tiny_image_under_a_large_halo(cuda, city_ctx, vistas_ctx, dataset):
    """1 x 5 x 3 at r = 5, d = 4: almost every neighbour is outside the image."""
    _parity(_ctx_of(dataset, city_ctx, vistas_ctx), dataset, "tiny", crf_ref.TINY_CASE, cuda)


@pytest.mark.parametrize("dataset", DATASETS)
def test_batch_stride(cuda, city_ctx, vistas_ctx, dataset):
    """N = 2 at 64 x 128, image 1 drawn from another seed than image 0: image 1 alone against
    the reference, and against image 0's result."""
    for case in ((3, 1, 2), (2, 3, 2)):
        figs = _parity(_ctx_of(dataset, city_ctx, vistas_ctx), dataset, "two_seed", case, cuda)
        d, q, d64, _, _ = figs[0]
        q64 = crf_ref.reference(dataset, case, np.float64, "two_seed")
        assert crf_ref.rel(q[1], q64[1]) <= 1e-5
        assert float(np.mean(d[1] != d64[1])) <= 1e-3
        assert crf_ref.rel(q[1], q64[0]) > 1e-2     # image 1 is not image 0


def test_zero_weights_keep_the_argmax_on_the_device(cuda, city_ctx):
    P, I = crf_ref.synthetic_inputs("cityscapes")
    n, H, W, ct = P.shape
    pd, im = torch.from_numpy(np.array(P)).to(cuda), torch.from_numpy(np.array(I)).to(cuda)
    out = torch.empty((n, H, W), dtype=torch.int32, device=cuda)
    q = torch.empty((n, H, W, ct), device=cuda)
    city_ctx.crf_decisions(pd, im, _params(3, weights=(0.0, 0.0)), MAPS["identity"], out,
                           workspace=_workspace(n, H, W, ct, cuda), probs_out=q)
    w = crf_ref.WIDTHS["cityscapes"]
    np.testing.assert_array_equal(crf_ref.head_argmax(q.cpu().numpy(), w), crf_ref.head_argmax(P, w))


# ---- refusals ------------------------------------------------------------------------------------

def test_entry_rejects_bad_arguments(cuda, city_ctx):
    from seg_hip import LIB, CrfParams, crf_workspace_bytes
    ctx = city_ctx
    n, H, W, ct = 2, 20, 24, 24
    probs = torch.full((n, H, W, ct + 1), 1.0 / 14, device=cuda)    # room for a misaligned view
    images = torch.zeros((n, H, W, 3), device=cuda)
    out = torch.full((n, H, W), -7, dtype=torch.int32, device=cuda)
    pout = torch.full((n, H, W, ct + 1), -3.0, device=cuda)
    need = crf_workspace_bytes(n, H, W, ct)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=cuda)
    ident = MAPS["identity"]
    good = dict(iterations=2, radius=3, dilation=1, w_appearance=4.0, w_smoothness=3.0,
                theta_alpha=67.0, theta_beta=3.0, theta_gamma=3.0)

    def call(ctx_h=ctx.h, probs_ptr=probs.data_ptr(), images_ptr=images.data_ptr(), nhw=(n, H, W),
             par=None, null_par=False, ws_ptr=ws.data_ptr(), ws_bytes=need, cid_map=ident,
             null_map=False, rv=0, out_hw=(H, W), pout_ptr=None, out_ptr=out.data_ptr()):
        p = CrfParams(**dict(good, **(par or {})))
        m = (ctypes.c_int32 * len(cid_map))(*cid_map)
        return LIB.seg_crf_decisions(ctx_h, probs_ptr, images_ptr, nhw[0], nhw[1], nhw[2],
                                     None if null_par else ctypes.byref(p), ws_ptr, ws_bytes,
                                     None if null_map else m, len(cid_map), rv, out_hw[0], out_hw[1],
                                     pout_ptr, out_ptr, None)
    assert call() == 0                                # the baseline call is valid
    assert call(par=dict(iterations=0), ws_ptr=None, ws_bytes=0) == 0   # T = 0 needs no workspace
    torch.cuda.synchronize()
    assert int(out.min()) >= 0
    out.fill_(-7)
    nan, inf = float("nan"), float("inf")
    cases = {
        "iterations -1": (dict(par=dict(iterations=-1)), "iterations"),
        "iterations 33": (dict(par=dict(iterations=33)), "iterations"),
        "radius 0": (dict(par=dict(radius=0)), "radius"),
        "radius 6": (dict(par=dict(radius=6)), "radius"),
        "dilation 0": (dict(par=dict(dilation=0)), "dilation"),
        "dilation 5": (dict(par=dict(dilation=5)), "dilation"),
        "w_appearance < 0": (dict(par=dict(w_appearance=-0.5)), "w_appearance"),
        "w_smoothness < 0": (dict(par=dict(w_smoothness=-1.0)), "w_smoothness"),
        "theta_alpha 0": (dict(par=dict(theta_alpha=0.0)), "theta_alpha"),
        "theta_beta < 0": (dict(par=dict(theta_beta=-3.0)), "theta_beta"),
        "theta_gamma 0": (dict(par=dict(theta_gamma=0.0)), "theta_gamma"),
        "w_appearance nan": (dict(par=dict(w_appearance=nan)), "w_appearance"),
        "w_smoothness inf": (dict(par=dict(w_smoothness=inf)), "w_smoothness"),
        "theta_alpha inf": (dict(par=dict(theta_alpha=inf)), "theta_alpha"),
        "theta_beta nan": (dict(par=dict(theta_beta=nan)), "theta_beta"),
        "theta_gamma nan": (dict(par=dict(theta_gamma=nan)), "theta_gamma"),
        "null probs": (dict(probs_ptr=None), "probs"),
        "null images": (dict(images_ptr=None), "images"),
        "null params": (dict(null_par=True), "params"),
        "null cid map": (dict(null_map=True), "cid_map"),
        "null decisions": (dict(out_ptr=None), "decisions_out"),
        "null workspace": (dict(ws_ptr=None), "workspace"),
        "small workspace": (dict(ws_bytes=need - 1), "workspace"),
        "misaligned workspace": (dict(ws_ptr=ws.data_ptr() + 8, ws_bytes=need + 8), "workspace"),
        "misaligned probs": (dict(probs_ptr=probs.data_ptr() + 4), "probs"),
        "misaligned probs_out": (dict(pout_ptr=pout.data_ptr() + 4), "probs_out"),
        "n 0": (dict(nhw=(0, H, W)), "n ="),
        "H 0": (dict(nhw=(n, 0, W)), "H ="),
        "W -1": (dict(nhw=(n, H, -1)), "W ="),
        "out_h 0": (dict(out_hw=(0, W)), "out_h"),
        "out_w 0": (dict(out_hw=(H, 0)), "out_w"),
        "replace_voids 2": (dict(rv=2), "replace_voids"),
        "replace_voids 3": (dict(rv=3), "replace_voids"),
        "replace_voids -1": (dict(rv=-1), "replace_voids"),
        "short cid map": (dict(cid_map=ident[:-1]), "cid_map"),
        "cid map entry -2": (dict(cid_map=[-2] + ident[1:]), "cid_map"),
    }
    for name, (kw, word) in cases.items():
        rc = call(**kw)
        msg = LIB.seg_last_error(ctx.h).decode()
        assert rc == -errno.EINVAL, (name, rc)
        assert "seg_crf_decisions" in msg and word in msg, (name, msg)
    assert call(ctx_h=None) == -errno.EINVAL
    assert b"seg_crf_decisions" in LIB.seg_last_error(None) and b"ctx" in LIB.seg_last_error(None)
    b = ctypes.c_int64(-1)
    for args in ((0, H, W, ct), (n, 0, W, ct), (n, H, 0, ct), (n, H, W, 0)):
        assert LIB.seg_crf_workspace(*args, ctypes.byref(b)) == -errno.EINVAL
        assert b"seg_crf_workspace" in LIB.seg_last_error(None)
    assert LIB.seg_crf_workspace(n, H, W, ct, None) == -errno.EINVAL and b.value == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((pout == -3.0).all())
    # the wrapper's own checks
    p4 = probs[..., :ct].contiguous()
    with pytest.raises(ValueError):
        ctx.crf_decisions(p4, images[:, :10], _params(0), ident, out)              # another size
    with pytest.raises(ValueError):
        ctx.crf_decisions(p4.double(), images, _params(0), ident, out)
    with pytest.raises(ValueError):
        ctx.crf_decisions(probs[..., :ct], images, _params(0), ident, out)         # not contiguous
    with pytest.raises(ValueError):
        ctx.crf_decisions(p4, images, _params(0), ident, out.long())
    with pytest.raises(RuntimeError, match="workspace"):
        ctx.crf_decisions(p4, images, _params(1), ident, out)
    assert bool((out == -7).all())


# ---- evaluate.py / predict.py --------------------------------------------------------------------

EVAL_ARGS = ["--height_feature_extractor", "48", "--width_feature_extractor", "64",
             "--compute_dtype", "fp32"]
MODES = {
    "alone": ([], (48, 64)),
    "flip": (["--tta_flip"], (48, 64)),
    "windows": (["--window_canvas", "72", "100", "--window_stride", "24", "36"], (72, 100)),
}
CRF_ARGS = ["--crf_iterations", "2", "--replace_voids"]


@pytest.fixture
def crf_calls(monkeypatch):
    """Records (probs, images, cid_map, decisions, replace_voids, settings) of every
    CRFDriver.decisions call, after it ran."""
    import estimator.crf as crf
    calls = []
    real = crf.CRFDriver.decisions

    def spy(self, probs, images, cid_map, out, replace_voids=False, probs_out=None):
        real(self, probs, images, cid_map, out, replace_voids, probs_out)
        calls.append((probs.cpu().numpy(), images.cpu().numpy(), list(cid_map), out.cpu().numpy(),
                      bool(replace_voids), self.settings,
                      None if probs_out is None else probs_out.cpu().numpy()))
    monkeypatch.setattr(crf.CRFDriver, "decisions", spy)
    return calls


def _check_against_reference(calls, hw, what):
    assert calls
    for probs, images, cid_map, decs, rv, st, q in calls:
        assert probs.shape[1:3] == hw and images.shape[1:3] == hw and rv
        assert (st.iterations, st.radius, st.dilation) == (2, 3, 1)
        q64 = crf_ref.mean_field(probs, images, st.radius, st.dilation, st.iterations)
        ref = crf_ref.decisions(q64, "cityscapes", cid_map, decs.shape[1:], rv)
        mism = float(np.mean(decs != ref))
        moved = float(np.mean(crf_ref.decisions(probs, "cityscapes", cid_map, decs.shape[1:], rv) != ref))
        print(f"{what}: decisions differ from the reference on {mism:.2e} (the refinement moved "
              f"{moved:.3f}), Q^T {crf_ref.rel(q, q64):.2e} norm-relative")
        assert mism <= 1e-3
        assert crf_ref.rel(q, q64) <= 1e-5


@pytest.mark.parametrize("mode", sorted(MODES))
def test_evaluate_with_crf(cuda, tmp_path, init_ckpt, crf_calls, mode):
    from input_pipelines.synthetic import images, pixel_labels
    from models.resnet50_extended_model_hierarchical import release_contexts
    extra, (h, w) = MODES[mode]
    ev = _script("evaluate")
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=2, dtype="fp32")
    release_contexts()
    res = ev.main([str(tmp_path), "2", PROBLEM, "cityscapes", "--Nb", "2"] + EVAL_ARGS + extra + CRF_ARGS
                  + ["--eval_res_dir", str(tmp_path / "c")])
    # the one batch evaluate_input draws (seed 1234): images first, then the labels
    rng = np.random.default_rng(1234)
    images(rng, 2, h, w)
    labels = pixel_labels(rng, 2, h, w)
    voids = int((labels == 19).sum())
    assert voids < labels.size
    cm = res[0]["confusion_matrix"]
    assert cm.shape == (19, 19)
    assert int(cm.sum()) == 2 * h * w - voids
    np.testing.assert_array_equal(cm.sum(1), np.bincount(labels.ravel(), minlength=20)[:19])
    assert len(crf_calls) == 1
    _check_against_reference(crf_calls, (h, w), f"evaluate {mode}")
    release_contexts()


def test_evaluate_zero_iterations_changes_nothing(cuda, tmp_path, init_ckpt, crf_calls):
    from models.resnet50_extended_model_hierarchical import release_contexts
    ev = _script("evaluate")
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=1, dtype="fp32")
    base = [str(tmp_path), "2", PROBLEM, "cityscapes", "--Nb", "1"] + EVAL_ARGS
    plain = ev.main(base + ["--eval_res_dir", str(tmp_path / "a")])
    zero = ev.main(base + ["--eval_res_dir", str(tmp_path / "b"), "--crf_iterations", "0"])
    assert int(plain[0]["confusion_matrix"].sum()) > 0
    np.testing.assert_array_equal(zero[0]["confusion_matrix"], plain[0]["confusion_matrix"])
    assert not crf_calls
    release_contexts()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_predict_script_exports_with_crf(cuda, tmp_path, init_ckpt, crf_calls, mode):
    from PIL import Image
    from models.resnet50_extended_model_hierarchical import release_contexts
    extra, hw = MODES[mode]
    pdir, rdir = tmp_path / "in", tmp_path / "out"
    pdir.mkdir()
    rdir.mkdir()
    rng = np.random.default_rng(6)
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (50, 90, 3), dtype=np.uint8)).save(pdir / f"img{i}.png")
    init_ckpt(tmp_path, pyramid="none", height=48, width=64, nb_pp=2, dtype="fp32")
    release_contexts()
    pr = _script("predict")
    n = pr.main([str(tmp_path), PROBLEM, str(pdir), "cityscapes", "--Nb", "2"] + EVAL_ARGS
                + ["--results_dir", str(rdir), "--export_lids_images", "--export_color_decisions"]
                + extra + CRF_ARGS)
    assert n == 3
    for i in range(3):
        lids = np.asarray(Image.open(rdir / f"img{i}_result_lids.png"))
        col = np.asarray(Image.open(rdir / f"img{i}_result_color.png"))
        assert lids.shape == (50, 90) and col.shape == (50, 90, 3)
    assert len(crf_calls) == 2                      # two batches of Nb = 2 for three images
    assert all(c[3].shape == (2, 50, 90) for c in crf_calls)
    _check_against_reference(crf_calls, hw, f"predict {mode}")
    release_contexts()


def test_lazy_predictions_reflect_the_refined_probabilities(cuda, crf_calls):
    """The EVAL spec with crf_iterations: *_probabilities are slices of Q^T, *_decisions their
    argmax, and the *_logits entries are still the model's."""
    import argparse
    from estimator.define_estimator_hierarchical import _eval_spec
    from estimator.mode_keys import ModeKeys
    from input_pipelines.synthetic import batch
    from models.resnet50_extended_model_hierarchical import get_context, model, release_contexts
    release_contexts()
    s = argparse.Namespace(Nb=2, height_feature_extractor=64, width_feature_extractor=128,
                           per_pixel_dataset_name="cityscapes", compute_dtype="fp32", pyramid="psp",
                           name_feature_extractor="resnet_v1_50", init_seed=3, crf_iterations=1,
                           crf_radius=2, training_cids2evaluation_cids=MAPS["identity"],
                           replace_voids=False)
    ctx = get_context(None, s, mode=ModeKeys.EVAL)
    data = batch(12, 2, 0, 0, 64, 128)
    x = torch.as_tensor(data["images"]).to(cuda)
    _, _, pred = model(ModeKeys.EVAL, x, None, None, s)
    labels = {"prolabels": torch.as_tensor(data["px"]).to(cuda)}
    spec = _eval_spec(pred, labels, None, s, x)
    assert len(crf_calls) == 1
    probs, _, _, decs, _, st, q = crf_calls[0]
    assert (st.iterations, st.radius) == (1, 2)
    np.testing.assert_array_equal(spec.predictions["decisions"].cpu().numpy(), decs)
    lo = 0
    for head, c in zip(("l1", "l2_vehicle", "l2_human"), (14, 7, 3)):
        p = pred[f"{head}_probabilities"]
        np.testing.assert_array_equal(p.cpu().numpy(), q[..., lo:lo + c])
        assert torch.equal(pred[f"{head}_decisions"].long(), torch.argmax(p, dim=-1))
        assert tuple(pred[f"{head}_logits"].shape) == (2, 64, 128, c)
        np.testing.assert_array_equal(pred[f"{head}_probabilities"].cpu().numpy(), q[..., lo:lo + c])
        lo += c
    assert not np.array_equal(q, probs)
    from estimator.crf import driver_for_crf
    drv = driver_for_crf(ctx, s)
    assert drv is driver_for_crf(ctx, s) and list(drv._buffers) == [(2, 64, 128)]
    release_contexts()


# ---- the one decide path: source x refinement x mode ---------------------------------------------

SOURCES = {
    # extra settings, (height, width) of the prepared batch, forwards beyond model_fn's
    "single": ({}, (64, 128), 0),
    "tta": (dict(tta_scales=[0.75, 1.0], tta_flip=True), (64, 128), 3),      # 48 x 96 and 64 x 128, flipped
    "windows": (dict(window_canvas=[64, 200], window_stride=[24, 40]), (64, 200), 3),   # xs 0, 40, 72
}
NO_TTA_LOGITS = ("l1_logits: test-time augmentation (--tta_scales / --tta_flip) averages probabilities "
                 "over several forwards; there are no full-resolution logits of the average (the "
                 "*_probabilities entries hold it)")
NO_WINDOW_LOGITS = ("{}: sliding windows (--window_canvas) average probabilities over the windows that "
                    "cover a pixel; no forward saw the canvas, so there are no logits of it (the "
                    "*_probabilities entries hold the average)")


@pytest.fixture(scope="module")
def shared_contexts():
    """The cases below share the cached contexts (and their drivers): released before and after."""
    from models.resnet50_extended_model_hierarchical import release_contexts
    release_contexts()
    yield
    release_contexts()


@pytest.mark.parametrize("mode", ["EVAL", "PREDICT"])
@pytest.mark.parametrize("crf", [0, 2])
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_decide_batch_is_the_low_level_sequence_bitwise(cuda, shared_contexts, source, crf, mode):
    """estimator.inference.decide_batch against the same sequence of low-level calls made here, for
    every source, with and without the CRF (T = 2, r = 1), in both modes, with and without
    replace_voids: bitwise equal decisions, the same number of forwards, and the lazy predictions'
    key set and KeyError texts of each mode."""
    import argparse
    from estimator.crf import crf_settings
    from estimator.inference import decide_batch
    from estimator.mode_keys import ModeKeys
    from estimator.tta import driver_for
    from estimator.windows import driver_for_windows
    from input_pipelines.synthetic import batch
    from inference_common import _realistic_moving_stats
    from models.resnet50_extended_model_hierarchical import LAZY_KEYS, get_context, model
    from seg_hip import CrfParams, crf_workspace_bytes, resize_images, window_images
    extra, hw, forwards = SOURCES[source]
    s = argparse.Namespace(Nb=2, height_feature_extractor=64, width_feature_extractor=128,
                           per_pixel_dataset_name="cityscapes", compute_dtype="fp32", pyramid="psp",
                           name_feature_extractor="resnet_v1_50", init_seed=3, crf_iterations=crf,
                           crf_radius=1, **extra)
    mode = getattr(ModeKeys, mode)
    order = "predict" if mode == ModeKeys.PREDICT else "eval"
    cid_map = list(range(20)) if mode == ModeKeys.PREDICT else MAPS["merge"]
    ctx = get_context(None, s, mode=mode)
    if not getattr(ctx, "_realistic", False):     # once per context: logits of a trained range
        _realistic_moving_stats(ctx, torch.as_tensor(batch(99, 2, 0, 0, 64, 128)["images"]).to(cuda))
        ctx._realistic = True
    x = torch.as_tensor(batch(12, 2, 0, 0, *hw)["images"]).to(cuda)
    tta, win = driver_for(ctx, None, s, mode) if source == "tta" else None, driver_for_windows(ctx, None, s, mode)
    assert (tta is not None, win is not None) == (source == "tta", source == "windows")
    contexts = {id(c): c for c in [ctx] + (tta.contexts if tta else [])}.values()
    count = lambda: sum(getattr(c, "forward_count", 0) for c in contexts)
    lazy = [k for k in LAZY_KEYS if source == "single" or not k.endswith("_logits")]
    lowres = [] if source == "windows" else [f"{h}_logits_lowres" for h in ("l1", "l2_vehicle", "l2_human")]
    for rv in (False, True):
        _, _, pred = model(mode, x, None, None, s)
        before = count()
        got = torch.full((2, 45, 77), -9, dtype=torch.int32, device=cuda)
        decide_batch(pred, x, ctx, None, s, mode, cid_map, got, rv, order=order)
        print(f"{source} crf {crf} {order} rv {rv}: {count() - before} forwards")
        assert count() - before == forwards
        # the lazy predictions
        assert set(pred.materialised()) == set(["decisions", "_context"] + lowres)     # no launch so far
        assert set(pred) == set(lazy + lowres + ["decisions", "_context"])
        if source == "single":
            assert tuple(pred["l1_logits"].shape) == (2, 64, 128, 14)
        else:
            with pytest.raises(KeyError) as e:
                pred["l1_logits"]
            assert e.value.args[0] == (NO_TTA_LOGITS if source == "tta" else NO_WINDOW_LOGITS.format("l1_logits"))
        if source == "windows":
            with pytest.raises(KeyError) as e:
                pred["l2_human_logits_lowres"]
            assert e.value.args[0] == NO_WINDOW_LOGITS.format("l2_human_logits_lowres")
        lazy_probs = torch.cat([pred[f"{h}_probabilities"] for h in ("l1", "l2_vehicle", "l2_human")], -1)
        assert tuple(lazy_probs.shape) == (2,) + hw + (24,)
        # the same sequence of low-level calls, as the specs made them before there was one path
        model(mode, x, None, None, s)
        want = torch.full((2, 45, 77), -7, dtype=torch.int32, device=cuda)
        probs = torch.full((2,) + hw + (24,), -1.0, device=cuda) if crf else None
        at_size = torch.empty((2,) + hw, dtype=torch.int32, device=cuda)
        if source == "single":
            if crf:
                ctx.full_predictions(probs=probs)
            else:
                ctx.predict(cid_map, want, replace_voids=rv, order=order)
        elif source == "tta":
            ents = []
            for c in tta.contexts:
                for flip in (False, True):
                    if c is not ctx or flip:
                        c.forward(resize_images(x, c.cfg.height, c.cfg.width, flip))
                    ents.append((c.outputs()[2].clone(), flip))
            if crf:
                ctx.tta_decisions(ents, list(range(20)), at_size, mean_probs=probs)
            else:
                ctx.tta_decisions(ents, cid_map, want, replace_voids=rv)
        else:
            ents = []
            for x0 in (0, 40, 72):
                ctx.forward(window_images(x, 0, x0, 64, 128, False))
                ents.append(ctx.outputs()[2].clone())
            if crf:
                ctx.window_decisions(ents, [0], [0, 40, 72], False, (64, 200), list(range(20)), at_size,
                                     mean_probs=probs)
            else:
                ctx.window_decisions(ents, [0], [0, 40, 72], False, (64, 200), cid_map, want, replace_voids=rv)
        if crf:
            q = torch.full_like(probs, -2.0)
            ws = torch.empty(crf_workspace_bytes(2, hw[0], hw[1], 24), dtype=torch.uint8, device=cuda)
            ctx.crf_decisions(probs, x, CrfParams(*crf_settings(s)), cid_map, want, replace_voids=rv,
                              workspace=ws, probs_out=q)
            assert torch.equal(lazy_probs, q)       # the lazy probabilities are Q^T
        assert int(want.min()) >= 0 and len(torch.unique(want)) > 1
        assert torch.equal(got, want)
