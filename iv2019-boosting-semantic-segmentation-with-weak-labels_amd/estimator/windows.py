"""Sliding-window inference for EVAL and PREDICT.

The reference's system sketch foresees it (``input || image || [tile] -> batch -> ... -> [stich]
|| labels || output``, utils/utils.py) and builds neither; the semantics are fixed in
``include/seg_hip.h`` at ``seg_window_decisions``. With ``--window_canvas HC WC`` the input
functions prepare the batch at the canvas size, the network runs at its own size H x W on
overlapping windows of the canvas, and the decisions come from the per-head softmax
probabilities averaged, per canvas pixel, over the windows that cover it. The windows are the
product ``ys x xs`` of ``window_origins`` per axis; entries follow rows of ``ys`` outermost,
then ``xs``, then, with ``--tta_flip``, the unflipped entry followed by the mirrored one. The
primary context alone runs every window: no other context, no copy of the parameters.

This module imports without a GPU and without the library: torch and ``seg_hip`` are imported
where they are used.
"""
from __future__ import annotations

from estimator.inference import Source, cached_driver

MAX_ENTRIES = 64   # SEG_WIN_MAX_ENTRIES: windows x (1 + flip) of one decision launch


def add_window_arguments(argparser):
    """``--window_canvas`` / ``--window_stride`` of evaluate.py and predict.py (off by default)."""
    argparser.add_argument(
        '--window_canvas', type=int, nargs=2, default=None, metavar=('HC', 'WC'),
        help='sliding-window inference: prepare the images (and EVAL labels) at HC x WC instead '
             'of the network size, run the network at its own size on overlapping windows of '
             'that canvas and average the softmax probabilities where windows overlap. '
             'Default: off. --tta_flip adds the mirrored forward of every window; --tta_scales '
             'cannot be combined with it.')
    argparser.add_argument(
        '--window_stride', type=int, nargs=2, default=None, metavar=('SY', 'SX'),
        help='distance between window origins per axis, 1..network size; the last window of an '
             'axis is flush with the canvas edge. Default: ((2 * H + 2) // 3, (2 * W + 2) // 3), '
             'about one third overlap.')


def default_stride(H, W):
    return (2 * int(H) + 2) // 3, (2 * int(W) + 2) // 3


def window_origins(C, n, s):
    """Origins of the windows of length ``n`` on a canvas axis of length ``C`` at stride ``s``:
    i * s for every i >= 0 with i * s < C - n, followed by C - n (the last window is flush with
    the edge); C == n gives [0]. A stride above n would leave a gap."""
    C, n, s = int(C), int(n), int(s)
    if C < n:
        raise ValueError(f'window_origins: the canvas length {C} is below the window length {n}')
    if s < 1 or s > n:
        raise ValueError(f'window_origins: stride {s} must be in 1..{n} (the window length); a '
                         'larger stride would leave a gap')
    return list(range(0, C - n, s)) + [C - n]


def window_grid(canvas, net, stride, flip):
    """(ys, xs) of the window grid of a ``canvas`` (Hc, Wc) for the network size ``net`` (H, W);
    refuses more than MAX_ENTRIES entries."""
    ys = window_origins(canvas[0], net[0], stride[0])
    xs = window_origins(canvas[1], net[1], stride[1])
    entries = len(ys) * len(xs) * (2 if flip else 1)
    if entries > MAX_ENTRIES:
        raise ValueError(f'sliding windows: canvas {canvas[0]} x {canvas[1]} at stride '
                         f'{stride[0]} x {stride[1]} gives {len(ys)} x {len(xs)} windows'
                         f'{" with flip" if flip else ""} = {entries} entries; at most '
                         f'{MAX_ENTRIES} fit one decision launch (raise the stride or lower the '
                         'canvas)')
    return ys, xs


def window_settings(params):
    """(canvas, stride, flip) of the settings, or None when sliding windows are off."""
    canvas = getattr(params, 'window_canvas', None)
    if not canvas:
        if getattr(params, 'window_stride', None):
            raise ValueError('--window_stride needs --window_canvas')
        return None
    if getattr(params, 'tta_scales', None):
        raise ValueError('--tta_scales and --window_canvas cannot be combined: multi-scale '
                         'sliding windows are not built (--tta_flip composes with --window_canvas)')
    stride = getattr(params, 'window_stride', None) or default_stride(
        params.height_feature_extractor, params.width_feature_extractor)
    return (tuple(int(v) for v in canvas), tuple(int(v) for v in stride),
            bool(getattr(params, 'tta_flip', False)))


def input_size(params):
    """The size the input functions prepare ``proimages`` at: the canvas under sliding windows,
    else the network size."""
    st = window_settings(params)
    if st is None:
        return params.height_feature_extractor, params.width_feature_extractor
    return st[0]


class WindowDriver(Source):
    """The window grid of one primary context and the per-batch entry loop (a source of
    ``estimator.inference``; the mean probabilities live at the canvas size): every entry is a
    forward of ``primary`` itself on one window of the canvas. Neither ``*_logits`` nor
    ``*_logits_lowres`` exist in the predictions (no single forward saw the canvas): the model's
    ``Predictions`` of a canvas say so from the start."""

    def __init__(self, primary, canvas, stride, flip):
        self.primary = primary
        self.canvas = self.size = (int(canvas[0]), int(canvas[1]))
        self.stride = (int(stride[0]), int(stride[1]))
        self.flip = bool(flip)
        self.net = (primary.cfg.height, primary.cfg.width)
        self.ys, self.xs = window_grid(self.canvas, self.net, self.stride, self.flip)

    def placements(self):
        """[(y0, x0, flip)] in entry order."""
        return [(y0, x0, f) for y0 in self.ys for x0 in self.xs
                for f in ((False, True) if self.flip else (False,))]

    def entries(self, proimages):
        """One forward per entry on ``proimages`` (device f32 [N, Hc, Wc, 3] in [-1, 1)); returns
        the low-resolution logits in entry order. They are clones: every forward overwrites the
        context's output buffer. Afterwards the context's own state (``outputs()``, ``predict``,
        ``full_predictions``) is that of the last entry."""
        from seg_hip import window_images
        p = self.primary
        x = proimages.contiguous()
        if tuple(x.shape[1:3]) != self.canvas:
            raise ValueError(f'sliding windows: the batch is {x.shape[1]} x {x.shape[2]}, the '
                             f'canvas {self.canvas[0]} x {self.canvas[1]}')
        H, W = self.net
        out = []
        for y0, x0, flip in self.placements():
            p.forward(window_images(x, y0, x0, H, W, flip))
            out.append(p.outputs()[2].clone())
        return out

    def decide(self, entries, cid_map, out, replace_voids=False, mean_probs=None):
        """One ``seg_window_decisions`` launch over ``entries`` into ``out`` (device int32
        [N, Ho, Wo])."""
        self.primary.window_decisions(entries, self.ys, self.xs, self.flip, self.canvas, cid_map, out,
                                      replace_voids=replace_voids, mean_probs=mean_probs)


def driver_for_windows(ctx, config, params, mode):
    """The primary context's window driver for these settings (built on first use, kept on the
    context), or None when the settings ask for no sliding windows."""
    st = window_settings(params)
    return cached_driver(ctx, '_window_drivers', st and (st, mode), lambda: WindowDriver(ctx, *st))
