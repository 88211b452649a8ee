"""Boundary-band (trimap) confusion on the GPU (include/seg_hip.h at seg_boundary_distance): the
distance pass, the band confusion on both histogram paths, every refusal of the C entries, and
evaluate.py with --boundary_widths. Everything is integer arithmetic and compared exactly with the
numpy reference of tests/boundary_ref.py (brute force over the disc of offsets).

* distance: 3 x 37 x 45 blocky labels (ragged against every tile, a single-class image between two
  whose boundaries touch it, max_width 1, 5 and 64: the halo then exceeds the image), 200 x 33 and
  33 x 300 maps of isolated pixels (taller / wider than a tile plus two halos; discs tell Euclidean
  from Chebyshev and are clipped at the corners), labels with -1 and nc.
* band confusion: the same maps with seeded decisions (2 % out of range), widths [1], the eight
  widths 1..64 and [64]; nc = 20 (private histogram), nc = 66 (eight widths: in memory; one width:
  private), with and without an ignored class; overwrite, repeatability, invariants.
* EVAL: evaluate.py --boundary_widths 1 2 4 8 against the reference on the recorded labels and
  decisions of every batch; with --crf_iterations; and without the flag nothing changes.
"""
import ctypes
import errno
import functools

import numpy as np
import pytest
import torch

import boundary_ref as ref
from inference_common import PROBLEM, _script, city_ctx, vistas_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = sorted(ref.CASES)
EIGHT = [1, 2, 3, 5, 8, 13, 21, 64]
WIDTH_SETS = {"one": [1], "eight": EIGHT, "widest": [64]}


@functools.lru_cache(maxsize=None)
def _labels(case, nc):
    lab = ref.CASES[case](nc)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _d2(case, nc, ignore, width):
    d = ref.d2_brute(_labels(case, nc), nc, ignore, width)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _decisions(case, nc):
    dec = ref.decisions_for(_labels(case, nc), nc)
    dec.setflags(write=False)
    return dec


def _band_reference(case, nc, ignore, widths):
    """int64 [K, nc, nc] from the shared brute-force distances at the widest width of the set."""
    lab, dec = _labels(case, nc), _decisions(case, nc)
    d2 = _d2(case, nc, ignore, max(widths))
    return np.stack([ref.confusion(lab, dec, nc, d2 <= w * w) for w in widths])


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


# ---- the distance pass -------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 5, 64])
@pytest.mark.parametrize("case", CASES)
def test_distance_is_the_brute_force(cuda, city_ctx, case, width):
    lab = _labels(case, 20)
    out = torch.full(lab.shape, -5, dtype=torch.int16, device=cuda)
    got = city_ctx.boundary_distance(_dev(lab, cuda), 20, 19, width, out=out)
    torch.cuda.synchronize()
    assert got is out
    want = _d2(case, 20, 19, width)
    np.testing.assert_array_equal(out.cpu().numpy().astype(np.int32), want)
    if case == "blocky":
        assert (want[1] == width * width + 1).all() and (want[0] == 0).any() and (want[2] == 0).any()
    if case.endswith("dots") and width == 5:
        # the centre pixel's plus: its arm at (cy, cx + 1) reaches (+3, +4) but not (+4, +4)
        cy, cx = lab.shape[1] // 2, lab.shape[2] // 2
        assert want[0, cy + 3, cx + 5] == 25 and want[0, cy + 4, cx + 5] == 26
        # the corner disc, clipped by the image: (4, 4) is 25 from both arms of the corner's plus
        assert want[0, 0, 0] == 0 and want[0, 4, 4] == 25 and want[0, 5, 4] == 26


def test_distance_without_an_ignored_class_and_with_another_class_count(cuda, city_ctx, vistas_ctx):
    lab = _labels("out_of_range", 20)
    got = city_ctx.boundary_distance(_dev(lab, cuda), 20, -1, 8)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int32), _d2("out_of_range", 20, -1, 8))
    assert not np.array_equal(_d2("out_of_range", 20, -1, 8), _d2("out_of_range", 20, 19, 8))
    lab = _labels("blocky", 66)
    got = vistas_ctx.boundary_distance(_dev(lab, cuda), 66, 65, 13)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int32), _d2("blocky", 66, 65, 13))
    # the context's buffer grows with the call: a larger map after a smaller one
    big = np.tile(_labels("blocky", 20), (1, 2, 3))
    got = city_ctx.boundary_distance(_dev(big, cuda), 20, 19, 5)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int32), ref.d2_separable(big, 20, 19, 5))


# ---- the band confusion ------------------------------------------------------------------------

def _band(ctx, case, nc, ignore, widths, cuda, fill=-12345):
    lab, dec = _dev(_labels(case, nc), cuda), _dev(_decisions(case, nc), cuda)
    out = torch.full((len(widths), nc, nc), fill, dtype=torch.int32, device=cuda)   # garbage: overwritten
    ctx.band_confusion(lab, dec, nc, ignore, widths, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("wname", sorted(WIDTH_SETS))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("nc,ignore", [(20, 19), (66, 65), (20, -1)])
def test_band_confusion_is_the_reference(cuda, city_ctx, vistas_ctx, nc, ignore, case, wname):
    """nc = 20: the block's private histogram; nc = 66: in memory with eight widths (8 * 66 * 66
    ints are beyond a block's LDS), private with one."""
    ctx = city_ctx if nc == 20 else vistas_ctx
    widths = WIDTH_SETS[wname]
    got = _band(ctx, case, nc, ignore, widths, cuda)
    again = _band(ctx, case, nc, ignore, widths, cuda, fill=7)
    want = _band_reference(case, nc, ignore, widths)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(again, got)
    assert want[-1].sum() > 0


@pytest.mark.parametrize("nc,ignore", [(20, 19), (66, 65)])
def test_band_confusion_invariants(cuda, city_ctx, vistas_ctx, nc, ignore):
    ctx = city_ctx if nc == 20 else vistas_ctx
    lab, dec = _labels("blocky", nc), _decisions("blocky", nc)
    got = _band(ctx, "blocky", nc, ignore, EIGHT, cuda).astype(np.int64)
    whole = torch.empty((nc, nc), dtype=torch.int32, device=cuda)
    ctx.confusion(_dev(lab, cuda), _dev(dec, cuda), nc, whole)
    whole = whole.cpu().numpy().astype(np.int64)
    # nested bands: non-decreasing in k
    assert (np.diff(got, axis=0) >= 0).all()
    # every band is part of the image
    assert (got <= whole[None]).all()
    assert 0 < got[0].sum() < got[-1].sum() <= whole.sum()
    # seg_confusion on the pixels of the brute-force band (the others' labels made unacceptable)
    d2 = _d2("blocky", nc, ignore, 64)
    for k, w in enumerate(EIGHT):
        masked = np.where(d2 <= w * w, lab, -1).astype(np.int32)
        cm = torch.empty((nc, nc), dtype=torch.int32, device=cuda)
        ctx.confusion(_dev(masked, cuda), _dev(dec, cuda), nc, cm)
        np.testing.assert_array_equal(cm.cpu().numpy(), got[k], err_msg=f"w = {w}")


def test_band_workspace_is_kept_on_the_context(cuda, city_ctx):
    from seg_hip import band_confusion_workspace_bytes
    _band(city_ctx, "blocky", 20, 19, [2, 4], cuda)
    ws = city_ctx._band_workspaces[(3, 37, 45)]
    _band(city_ctx, "blocky", 20, 19, [1, 2, 3], cuda)
    assert city_ctx._band_workspaces[(3, 37, 45)] is ws
    need = band_confusion_workspace_bytes(3, 37, 45, 2, 20)
    assert need >= 3 * 37 * 45 and need % 16 == 0 and ws.numel() == need


# ---- refusals ----------------------------------------------------------------------------------

def test_entries_reject_bad_arguments(cuda, city_ctx):
    from seg_hip import LIB, band_confusion_workspace_bytes
    ctx = city_ctx
    n, H, W, nc = 2, 20, 24, 20
    lab = torch.zeros((n, H, W), dtype=torch.int32, device=cuda)
    lab[:, :, 12:] = 3
    dec = lab.clone()
    need = band_confusion_workspace_bytes(n, H, W, 3, nc)
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    cm = torch.full((8, nc, nc), -7, dtype=torch.int32, device=cuda)
    d2 = torch.full((n, H, W), -7, dtype=torch.int16, device=cuda)

    def band(ctx_h=ctx.h, lab_ptr=lab.data_ptr(), dec_ptr=dec.data_ptr(), nhw=(n, H, W), nc_=nc, ignore=19,
             widths=(1, 2, 4), null_widths=False, k=None, ws_ptr=ws.data_ptr(), ws_bytes=need,
             cm_ptr=cm.data_ptr()):
        w = (ctypes.c_int32 * max(len(widths), 1))(*widths)
        return LIB.seg_band_confusion(ctx_h, lab_ptr, dec_ptr, nhw[0], nhw[1], nhw[2], nc_, ignore,
                                      None if null_widths else w, len(widths) if k is None else k,
                                      ws_ptr, ws_bytes, cm_ptr, None)

    def dist(ctx_h=ctx.h, lab_ptr=lab.data_ptr(), nhw=(n, H, W), nc_=nc, ignore=19, width=4,
             out_ptr=d2.data_ptr()):
        return LIB.seg_boundary_distance(ctx_h, lab_ptr, nhw[0], nhw[1], nhw[2], nc_, ignore, width,
                                         out_ptr, None)
    assert band() == 0 and dist() == 0                      # the baseline calls are valid
    torch.cuda.synchronize()
    assert int(cm[:3].min()) >= 0 and int(cm[2].sum()) == n * H * 10 and int(d2.min()) == 0
    cm.fill_(-7)
    d2.fill_(-7)
    band_cases = {
        "null labels": (dict(lab_ptr=None), "labels"),
        "null decisions": (dict(dec_ptr=None), "decisions"),
        "null widths": (dict(null_widths=True), "widths"),
        "null workspace": (dict(ws_ptr=None), "workspace"),
        "null cm_out": (dict(cm_ptr=None), "cm_out"),
        "n 0": (dict(nhw=(0, H, W)), "n ="),
        "H 0": (dict(nhw=(n, 0, W)), "H ="),
        "W -1": (dict(nhw=(n, H, -1)), "W ="),
        "nc 0": (dict(nc_=0, ignore=-1), "num_classes"),
        "nc 257": (dict(nc_=257), "num_classes"),
        "ignore = nc": (dict(ignore=20), "ignore"),
        "ignore -2": (dict(ignore=-2), "ignore"),
        "K 0": (dict(k=0), "n_widths"),
        "K 9": (dict(widths=tuple(range(1, 10))), "n_widths"),
        "width 0": (dict(widths=(0, 2)), "widths[0]"),
        "width 65": (dict(widths=(2, 65)), "widths[1]"),
        "equal widths": (dict(widths=(2, 2)), "increasing"),
        "decreasing widths": (dict(widths=(1, 4, 3)), "increasing"),
        "small workspace": (dict(ws_bytes=need - 1), "workspace"),
    }
    for name, (kw, word) in band_cases.items():
        rc = band(**kw)
        msg = LIB.seg_last_error(ctx.h).decode()
        assert rc == -errno.EINVAL, (name, rc)
        assert "seg_band_confusion" in msg and word in msg, (name, msg)
    assert band(ctx_h=None) == -errno.EINVAL
    assert b"seg_band_confusion" in LIB.seg_last_error(None) and b"ctx" in LIB.seg_last_error(None)
    dist_cases = {
        "null labels": (dict(lab_ptr=None), "labels"),
        "null d2_out": (dict(out_ptr=None), "d2_out"),
        "n 0": (dict(nhw=(0, H, W)), "n ="),
        "H -3": (dict(nhw=(n, -3, W)), "H ="),
        "W 0": (dict(nhw=(n, H, 0)), "W ="),
        "nc 0": (dict(nc_=0, ignore=-1), "num_classes"),
        "nc 300": (dict(nc_=300), "num_classes"),
        "ignore = nc": (dict(ignore=20), "ignore"),
        "ignore -2": (dict(ignore=-2), "ignore"),
        "max_width 0": (dict(width=0), "max_width"),
        "max_width 65": (dict(width=65), "max_width"),
    }
    for name, (kw, word) in dist_cases.items():
        rc = dist(**kw)
        msg = LIB.seg_last_error(ctx.h).decode()
        assert rc == -errno.EINVAL, (name, rc)
        assert "seg_boundary_distance" in msg and word in msg, (name, msg)
    assert dist(ctx_h=None) == -errno.EINVAL
    assert b"seg_boundary_distance" in LIB.seg_last_error(None) and b"ctx" in LIB.seg_last_error(None)
    b = ctypes.c_int64(-1)
    for args in ((0, H, W, 3, nc), (n, 0, W, 3, nc), (n, H, 0, 3, nc), (n, H, W, 0, nc), (n, H, W, 9, nc),
                 (n, H, W, 3, 0), (n, H, W, 3, 257)):
        assert LIB.seg_band_confusion_workspace(*args, ctypes.byref(b)) == -errno.EINVAL
        assert b"seg_band_confusion_workspace" in LIB.seg_last_error(None)
    assert LIB.seg_band_confusion_workspace(n, H, W, 3, nc, None) == -errno.EINVAL and b.value == -1
    torch.cuda.synchronize()
    assert bool((cm == -7).all()) and bool((d2 == -7).all())     # no launch wrote anything
    # the wrappers' own checks
    with pytest.raises(ValueError):
        ctx.band_confusion(lab.long(), dec, nc, 19, [1], cm[:1])
    with pytest.raises(ValueError):
        ctx.band_confusion(lab, dec[:, :10], nc, 19, [1], cm[:1])
    with pytest.raises(ValueError):
        ctx.band_confusion(lab, dec, nc, 19, [1, 2], cm[:1])
    with pytest.raises(ValueError):
        ctx.boundary_distance(lab, nc, 19, 4, out=d2.int())
    with pytest.raises(RuntimeError, match="increasing"):
        ctx.band_confusion(lab, dec, nc, 19, [4, 2], cm[:2])
    assert bool((cm == -7).all())


# ---- evaluate.py ---------------------------------------------------------------------------------

EVAL_ARGS = ["--height_feature_extractor", "64", "--width_feature_extractor", "128",
             "--compute_dtype", "fp32", "--psp_module", "--Nb", "2"]
WIDTHS = [1, 2, 4, 8]


def _evaluate(tmp_path, name, extra, record=None):
    """evaluate.py's objects driven as its main drives them, max_steps = 2; ``record`` takes
    (prolabels, decisions) of every EVAL spec."""
    from system_factory import SemanticSegmentation
    ev = _script("evaluate")
    argv = [str(tmp_path), "4", PROBLEM, "cityscapes", "--eval_res_dir", str(tmp_path / name)] + EVAL_ARGS + extra
    if record is None:
        return ev.main(argv, max_steps=2), tmp_path / name
    real = SemanticSegmentation.__init__

    def spying_init(self, *a, **kw):
        real(self, *a, **kw)
        fn = self._estimator_fn

        def spy(mode, features, labels, **kws):
            spec = fn(mode, features, labels, **kws)
            record.append((labels["prolabels"].cpu().numpy(), spec.predictions["decisions"].cpu().numpy()))
            return spec
        self._estimator_fn = spy
    SemanticSegmentation.__init__ = spying_init
    try:
        return ev.main(argv, max_steps=2), tmp_path / name
    finally:
        SemanticSegmentation.__init__ = real


def test_evaluate_with_boundary_widths(cuda, tmp_path, init_ckpt):
    from models.resnet50_extended_model_hierarchical import release_contexts
    init_ckpt(tmp_path, pyramid="psp", height=64, width=128, nb_pp=2, dtype="fp32")
    release_contexts()
    plain, plain_dir = _evaluate(tmp_path, "plain", [])
    batches = []
    res, res_dir = _evaluate(tmp_path, "band", ["--boundary_widths"] + [str(w) for w in WIDTHS], batches)
    assert len(batches) == 2 and len(res) == 1
    m = res[0]
    # off means off: today's keys and today's arrays
    assert set(plain[0]) == {"global_step", "loss", "confusion_matrix"}
    with np.load(plain_dir / "all_metrics.npz") as z:
        assert set(z.files) == {"global_step", "confusion_matrix"}
    assert not (plain_dir / "boundary_metrics.txt").exists()
    # on: two more keys, the whole-image matrix unchanged
    assert set(m) == {"global_step", "loss", "confusion_matrix", "boundary_widths", "band_confusion_matrices"}
    np.testing.assert_array_equal(m["confusion_matrix"], plain[0]["confusion_matrix"])
    assert m["boundary_widths"] == WIDTHS
    bands = m["band_confusion_matrices"]
    assert bands.shape == (4, 19, 19) and bands.dtype == np.int32
    # the reference on the recorded labels and decisions of both batches, void row and column dropped
    want = sum(ref.band_confusion(lab, dec, 20, 19, WIDTHS) for lab, dec in batches)[:, :-1, :-1]
    assert want[0].sum() > 0
    np.testing.assert_array_equal(bands, want)
    assert (np.diff(bands.astype(np.int64), axis=0) >= 0).all() and (bands <= m["confusion_matrix"][None]).all()
    with np.load(res_dir / "all_metrics.npz") as z:
        assert set(z.files) == {"global_step", "confusion_matrix", "boundary_widths", "band_confusion_matrix"}
        np.testing.assert_array_equal(z["boundary_widths"], WIDTHS)
        np.testing.assert_array_equal(z["band_confusion_matrix"], bands[None])
        np.testing.assert_array_equal(z["confusion_matrix"], m["confusion_matrix"][None])
    lines = (res_dir / "boundary_metrics.txt").read_text().splitlines()
    assert len(lines) == 4
    assert [ln.split()[:2] for ln in lines] == [["00000", str(w)] for w in WIDTHS]
    assert (res_dir / "all_metrics.txt").read_text() == (plain_dir / "all_metrics.txt").read_text()
    # composes with the CRF: shapes and invariants
    crf, _ = _evaluate(tmp_path, "crf", ["--boundary_widths"] + [str(w) for w in WIDTHS] + ["--crf_iterations", "1"])
    cb = crf[0]["band_confusion_matrices"]
    assert cb.shape == (4, 19, 19) and cb.dtype == np.int32
    assert (np.diff(cb.astype(np.int64), axis=0) >= 0).all() and (cb <= crf[0]["confusion_matrix"][None]).all()
    release_contexts()
