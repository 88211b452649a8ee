"""Boundary-band (trimap) accuracy for EVAL.

The reference has no counterpart; the semantics are fixed in ``include/seg_hip.h`` at
``seg_boundary_distance``. With ``--boundary_widths W [W ...]`` evaluate.py reports, beside the
whole-image confusion matrix, one confusion matrix per width w over the ground-truth pixels within
w pixels (Euclidean) of a label boundary: a boundary pixel carries a counted label (an evaluation
class that is not the dropped void class) and has a 4-neighbour in its image with another counted
label; the band of width w holds the pixels whose squared distance to the nearest boundary pixel
of their image is <= w^2. The bands are nested. It reads only the labels and the decisions of a
batch, so it composes with ``--tta_*``, ``--window_*`` and ``--crf_*`` as it stands.

The widths are sorted and de-duplicated when the settings are read (``--boundary_widths 8 2 2 4``
is ``2 4 8``); the limits apply to what remains.

This module imports without a GPU and without the library: torch and ``seg_hip`` are imported
where they are used.
"""
from __future__ import annotations

MAX_WIDTHS, MAX_WIDTH = 8, 64   # the limits of seg_band_confusion


def add_boundary_arguments(argparser):
    """``--boundary_widths`` of evaluate.py (off by default)."""
    argparser.add_argument(
        '--boundary_widths', type=int, nargs='+', default=None, metavar='W',
        help='boundary-band (trimap) accuracy: also report the confusion matrix over the '
             'ground-truth pixels within W pixels (Euclidean) of a label boundary, for each of 1..'
             f'{MAX_WIDTHS} widths W in 1..{MAX_WIDTH} (sorted and de-duplicated). Boundaries against '
             'the dropped void class do not count. Default: off. Composes with --tta_scales / '
             '--tta_flip, --window_canvas and --crf_iterations.')


def boundary_settings(params):
    """The band widths of the settings as a strictly increasing tuple of ints, or None when the
    metric is off (``boundary_widths`` None or absent). Validated here, when the settings are read,
    naming the flag."""
    v = getattr(params, 'boundary_widths', None)
    if v is None:
        return None
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    for w in v:
        if isinstance(w, bool) or not isinstance(w, int) or not 1 <= w <= MAX_WIDTH:
            raise ValueError(f'--boundary_widths {w!r}: an integer in 1..{MAX_WIDTH}')
    widths = tuple(sorted(set(int(w) for w in v)))
    if not 1 <= len(widths) <= MAX_WIDTHS:
        raise ValueError(f'--boundary_widths takes 1..{MAX_WIDTHS} distinct widths, got {len(widths)}')
    return widths


def void_dropped(params):
    """Whether ``SemanticSegmentation.evaluate`` drops the last (void) row and column of the
    confusion matrices: the evaluation problem maps some label id to void and the void class is
    not trained."""
    return (-1 in params.evaluation_problem_def['lids2cids']
            and not getattr(params, 'train_void_class', False))


def band_confusion(ctx, prolabels, decisions, num_classes, params, widths):
    """Device int32 [K, nc, nc]: the band confusion matrices of one batch (seg_band_confusion).
    The void class, ``num_classes`` - 1, makes no boundary exactly when evaluate() drops it."""
    import torch
    ignore = num_classes - 1 if void_dropped(params) else -1
    out = torch.empty((len(widths), num_classes, num_classes), dtype=torch.int32, device=prolabels.device)
    ctx.band_confusion(prolabels, decisions, num_classes, ignore, widths, out)
    return out


def band_metrics_lines(step, widths, matrices):
    """The lines of boundary_metrics.txt for one checkpoint: step, w, global accuracy, mean
    accuracy, mean IoU per width, in the number formats of all_metrics.txt."""
    import numpy as np
    from utils.utils import metrics_from_confusion_matrix
    lines = []
    for w, cm in zip(widths, matrices):
        g, ma, mi = metrics_from_confusion_matrix(np.asarray(cm))[:3]
        lines.append(f"{step:>05} {w:>2d} {g:>5.2f} {ma:>5.2f} {mi:>5.2f}")
    return lines
