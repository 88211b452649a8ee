"""Box-constrained pseudo-labels: per-pixel training labels for images that carry only boxes.

The reference has no counterpart; the semantics are fixed in ``include/seg_hip.h`` at
``seg_box_constrain``. The probabilities of whichever inference path is active -- one forward,
``--tta_scales`` / ``--tta_flip``, or ``--window_canvas`` -- are restricted per pixel to the fine
classes of the boxes covering it, optionally refined by the mean-field CRF (``--crf_iterations``),
and decided: the boxes choose the fine class, a vehicle or human pixel without a box and a pixel
below ``--pseudo_tau`` become the void cid, and a box the model filled with less than
``--pseudo_min_fill`` of its own class blanks its whole rectangle.

The two defaults (0 and 0) switch the thresholds off. Nothing here tunes them, and the accuracy
effect of training on these labels is unmeasured.

This module imports without a GPU and without the library: torch and ``seg_hip`` are imported
where they are used.
"""
from __future__ import annotations

import math

import numpy as np


def add_pseudo_arguments(argparser):
    """``--pseudo_tau`` / ``--pseudo_min_fill`` of pseudo_label.py (both off by default)."""
    argparser.add_argument(
        '--pseudo_tau', type=float, default=0.0, metavar='TAU',
        help='a pixel whose l1 confidence (the maximum l1 probability, after the box constraint '
             'and the CRF) is below TAU gets the void label. In [0, 1]. Default: 0 = no pixel is '
             'dropped for confidence. An off-switch, not a recommendation: nothing here tunes it.')
    argparser.add_argument(
        '--pseudo_min_fill', type=float, default=0.0, metavar='F',
        help='a vehicle or human box of which less than the share F of the covered pixels got the '
             "box's own class is rejected: its whole rectangle gets the void label. In [0, 1]. "
             'Default: 0 = no box is rejected. An off-switch, not a recommendation: nothing here '
             'tunes it.')


def _unit(flag, v):
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f'{flag} {v!r}: a number in [0, 1]') from None
    if isinstance(v, bool) or not math.isfinite(x) or not 0.0 <= x <= 1.0:
        raise ValueError(f'{flag} {v!r}: a number in [0, 1]')
    return x


def pseudo_settings(params):
    """(tau, min_fill) of the settings (0 where absent), each validated in [0, 1] naming its flag."""
    def setting(name):
        v = getattr(params, name, None)
        return 0.0 if v is None else v
    return _unit('--pseudo_tau', setting('pseudo_tau')), _unit('--pseudo_min_fill', setting('pseudo_min_fill'))


def rejected_boxes(counts, cids, min_fill, kinds):
    """int32 [len(cids)]: 1 for a vehicle or human box with area > 0 and hit < min_fill * area
    (float64). ``counts``: [len(cids), 2] = (area, hit) of seg_box_decisions. ``kinds``: per weak
    class 0 for an inert one (``SegContext.box_kinds()``: the tables the kernels use). Inert boxes
    and boxes of zero area are never rejected."""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1, 2)[:len(cids)]
    live = np.asarray(kinds, dtype=np.int64)[np.asarray(cids, dtype=np.int64)] != 0
    return (live & (counts[:, 0] > 0) & (counts[:, 1] < float(min_fill) * counts[:, 0])).astype(np.int32)


def batches_by_size(sizes, nb):
    """Batches of consecutive items of one size: [(indices of the real items, padded indices of
    length nb)]. A size change closes the batch; a short batch is padded with its last item."""
    out, cur = [], []
    for i, s in enumerate(sizes):
        if cur and (len(cur) == nb or tuple(sizes[cur[0]]) != tuple(s)):
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return [(c, c + [c[-1]] * (nb - len(c))) for c in out]


def label_id_palette(problem_def):
    """uint8 [n_cids]: training cid -> label id; a cid without one (the void cid of Vistas) takes the
    first label id that ``lids2cids`` maps to void."""
    lids2cids = list(problem_def['lids2cids'])
    pal = []
    for lid in problem_def['cids2lids']:
        if lid < 0:
            if -1 not in lids2cids:
                raise ValueError('cids2lids has a void entry but lids2cids maps no label id to void')
            lid = lids2cids.index(-1)
        pal.append(lid)
    return np.asarray(pal, dtype=np.uint8)


def pseudo_example(raw, lids, image_path, label_path):
    """One serialized example of the per-pixel stream (what ``parse_cityscapes_example`` reads):
    ``raw`` uint8 [h, w, 3], ``lids`` uint8 [h, w] label ids."""
    from input_pipelines.tfrecords import encode_example, encode_png
    return encode_example({
        'image/encoded': [encode_png(np.ascontiguousarray(raw))],
        'label/encoded': [encode_png(np.ascontiguousarray(lids))],
        'image/path': [image_path.encode()], 'label/path': [label_path.encode()]})


def label_batch(predictions, images, box_lists, ctx, config, params, out):
    """Pseudo-labels of the batch ``images`` (the prepared batch, or the canvas) into ``out``
    (device int32 [N, Ho, Wo], training cids): the source's mean probabilities -> constrain ->
    the CRF if ``--crf_iterations`` > 0 -> decide -> rejects from the counts on the host ->
    finalize to out's size. ``box_lists``: per image (cids, coords (k, 4) = (xmin, xmax, ymin,
    ymax) normalised, src_size (h, w)); the probabilities live at the source's size, so every geom
    is (src_h, src_w, size_h, size_w, 0, 0). The source is chosen as ``decide_batch`` chooses it.
    Returns (out, report): per image the share of labelled pixels and per box its class, area, hit
    and rejected flag. ``predictions`` get the lazy entries of the probabilities decided on."""
    import torch
    from estimator.crf import driver_for_crf
    from estimator.inference import pick_source
    from estimator.mode_keys import ModeKeys
    from input_pipelines.weak_labels import BoxLists
    tau, min_fill = pseudo_settings(params)
    source = pick_source(ctx, config, params, ModeKeys.PREDICT, 'predict')
    crf = driver_for_crf(ctx, params)
    size = tuple(int(v) for v in source.size)
    items = BoxLists((np.asarray(it[0], np.int32), np.asarray(it[1], np.float32).reshape(-1, 4),
                      (int(it[2][0]), int(it[2][1])), size, (0, 0)) for it in box_lists)
    entries = source.entries(images)
    probs = source.mean_probabilities(entries)
    n = int(probs.shape[0])
    boxes = ctx.upload_boxes(items, size)      # once per batch
    q = torch.empty_like(probs)
    ctx.box_constrain(probs, boxes, q)
    if crf is not None:
        refined = torch.empty_like(q)
        scratch = torch.empty((n,) + size, dtype=torch.int32, device=q.device)
        crf.decisions(q, images, list(range(ctx.n_classes)), scratch, probs_out=refined)
        q = refined
    labels = torch.empty((n,) + size, dtype=torch.int32, device=q.device)
    counts = torch.empty((max(boxes.total, 1), 2), dtype=torch.int32, device=q.device)
    ctx.box_decisions(q, boxes, tau, labels, counts)
    counts_h = counts.cpu().numpy()[:boxes.total]
    cids = np.concatenate([it[0] for it in items] + [np.zeros(0, np.int32)])
    reject_h = rejected_boxes(counts_h, cids, min_fill, ctx.box_kinds())
    reject = torch.zeros(max(boxes.total, 1), dtype=torch.int32)
    reject[:boxes.total] = torch.from_numpy(reject_h)
    ctx.box_finalize(labels, boxes, reject.to(q.device), out)
    source.attach(predictions, entries, q)
    ignore = ctx.n_classes - 1
    share = (out != ignore).float().mean(dim=(1, 2)).cpu().numpy()
    report, b0 = [], 0
    for i, it in enumerate(items):
        k = len(it[0])
        report.append({'labelled': float(share[i]),
                       'boxes': [{'class': int(cids[b]), 'area': int(counts_h[b, 0]),
                                  'hit': int(counts_h[b, 1]), 'rejected': bool(reject_h[b])}
                                 for b in range(b0, b0 + k)]})
        b0 += k
    return out, report
