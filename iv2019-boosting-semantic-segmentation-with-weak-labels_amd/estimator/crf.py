"""Mean-field CRF refinement of the probabilities for EVAL and PREDICT.

The reference has no counterpart (its predict.py stops at the argmax); the semantics are fixed in
``include/seg_hip.h`` at ``seg_crf_decisions``. With ``--crf_iterations T`` (T >= 1) the decisions
of a batch come from the per-head probabilities of whichever inference path is active -- one
forward, ``--tta_scales`` / ``--tta_flip``, or ``--window_canvas`` -- after T mean-field steps of
a Potts model whose pairwise weight is a bilateral (position + colour) kernel plus a spatial
kernel over the (2r + 1)^2 - 1 offsets (dy * d, dx * d), conditioned on the prepared batch at
the size of the probabilities.

The defaults (T = 5 when switched on by hand, r = 3, d = 1, weights 4 / 3, thetas 67 / 3 / 3) are
the commonly published DenseCRF settings for street scenes. Nothing here tunes them: they are
untuned for this model, and no accuracy claim is made.

This module imports without a GPU and without the library: torch and ``seg_hip`` are imported
where they are used.
"""
from __future__ import annotations

import math
from collections import namedtuple

from estimator.inference import cached_driver

MAX_ITERATIONS, MAX_RADIUS, MAX_DILATION = 32, 5, 4   # the limits of seg_crf_decisions
DEFAULT_ITERATIONS = 5   # the published setting; the flag itself defaults to 0 = off
DEFAULT_RADIUS, DEFAULT_DILATION = 3, 1
DEFAULT_WEIGHTS = (4.0, 3.0)          # w_a (appearance), w_s (smoothness)
DEFAULT_THETAS = (67.0, 3.0, 3.0)     # theta_alpha [px], theta_beta [grey levels], theta_gamma [px]

CRFSettings = namedtuple('CRFSettings', ['iterations', 'radius', 'dilation', 'w_appearance',
                                         'w_smoothness', 'theta_alpha', 'theta_beta', 'theta_gamma'])


def add_crf_arguments(argparser):
    """``--crf_*`` of evaluate.py and predict.py (off by default)."""
    argparser.add_argument(
        '--crf_iterations', type=int, default=0, metavar='T',
        help='mean-field CRF refinement of the probabilities before the argmax: T parallel '
             f'updates, 0..{MAX_ITERATIONS}. Default: 0 = off ({DEFAULT_ITERATIONS} is the commonly '
             'published setting). Composes with --tta_scales / --tta_flip and --window_canvas '
             '(their averaged probabilities are refined). With --replace_voids the voids are '
             'replaced from the top-2 of the refined l1 probabilities before the resize (the EVAL '
             'order). The default parameters are published street-scene settings, not tuned here.')
    argparser.add_argument(
        '--crf_radius', type=int, default=DEFAULT_RADIUS, metavar='R',
        help=f'neighbourhood radius r, 1..{MAX_RADIUS}: the (2r + 1)^2 - 1 offsets (dy * d, dx * d). '
             f'Default: {DEFAULT_RADIUS}.')
    argparser.add_argument(
        '--crf_dilation', type=int, default=DEFAULT_DILATION, metavar='D',
        help=f'neighbourhood dilation d, 1..{MAX_DILATION}. Default: {DEFAULT_DILATION}.')
    argparser.add_argument(
        '--crf_weights', type=float, nargs=2, default=list(DEFAULT_WEIGHTS), metavar=('WA', 'WS'),
        help='weights of the appearance (bilateral) and the smoothness (spatial) kernel, >= 0. '
             f'Default: {DEFAULT_WEIGHTS[0]:g} {DEFAULT_WEIGHTS[1]:g}.')
    argparser.add_argument(
        '--crf_thetas', type=float, nargs=3, default=list(DEFAULT_THETAS),
        metavar=('ALPHA', 'BETA', 'GAMMA'),
        help='theta_alpha (pixels) and theta_beta (grey levels of the 0..255 image) of the '
             'appearance kernel, theta_gamma (pixels) of the smoothness kernel, all > 0. '
             f'Default: {DEFAULT_THETAS[0]:g} {DEFAULT_THETAS[1]:g} {DEFAULT_THETAS[2]:g}.')


def _int_in(flag, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f'{flag} {v!r}: an integer in {lo}..{hi}')
    return int(v)


def _floats(flag, v, n, names, positive):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    if len(v) != n:
        raise ValueError(f'{flag} takes {n} values ({" ".join(names)}), got {len(v)}')
    out = []
    for name, x in zip(names, v):
        x = float(x)
        if not math.isfinite(x):
            raise ValueError(f'{flag}: {name} = {x!r} is not finite')
        if (x <= 0.0) if positive else (x < 0.0):
            raise ValueError(f'{flag}: {name} = {x:g} must be {"> 0" if positive else ">= 0"}')
        out.append(x)
    return out


def crf_settings(params):
    """CRFSettings of the settings, or None when the refinement is off (``crf_iterations`` 0 or
    absent). Every value is validated here, when the settings are read, naming its flag."""
    def setting(name, default):
        v = getattr(params, name, None)
        return default if v is None else v
    it = _int_in('--crf_iterations', setting('crf_iterations', 0), 0, MAX_ITERATIONS)
    r = _int_in('--crf_radius', setting('crf_radius', DEFAULT_RADIUS), 1, MAX_RADIUS)
    d = _int_in('--crf_dilation', setting('crf_dilation', DEFAULT_DILATION), 1, MAX_DILATION)
    wa, ws = _floats('--crf_weights', setting('crf_weights', DEFAULT_WEIGHTS), 2, ('WA', 'WS'),
                     positive=False)
    ta, tb, tg = _floats('--crf_thetas', setting('crf_thetas', DEFAULT_THETAS), 3,
                         ('ALPHA', 'BETA', 'GAMMA'), positive=True)
    if it == 0:
        return None
    return CRFSettings(it, r, d, wa, ws, ta, tb, tg)


def offsets(radius, dilation):
    """[(dy * d, dx * d)] in the order of seg_crf_decisions: row-major (dy, dx), (0, 0) left out."""
    r, d = int(radius), int(dilation)
    return [(dy * d, dx * d) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy or dx]


class CRFDriver(object):
    """The workspace of one context's refinement: allocated once per (n, H, W), then reused."""

    def __init__(self, ctx, settings):
        from seg_hip import CrfParams
        self.ctx = ctx
        self.settings = settings
        self.params = CrfParams(*settings)
        self._buffers = {}

    def _workspace(self, n, H, W):
        import torch
        from seg_hip import crf_workspace_bytes
        key = (n, H, W)
        if key not in self._buffers:
            nbytes = crf_workspace_bytes(n, H, W, sum(self.ctx.head_widths))
            self._buffers[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.ctx.device)
        return self._buffers[key]

    def decisions(self, probs, images, cid_map, out, replace_voids=False, probs_out=None):
        """Decisions of Q^T into ``out`` (device int32 [n, Ho, Wo]) from ``probs`` (device f32
        [n, H, W, CT]) and ``images`` (device f32 [n, H, W, 3]); ``probs_out`` optionally takes
        Q^T."""
        images = images.contiguous()
        if tuple(images.shape[:3]) != tuple(probs.shape[:3]):
            raise ValueError(f'CRF refinement: the probabilities are {tuple(probs.shape[:3])}, the '
                             f'images {tuple(images.shape[:3])}: both must have one size')
        n, H, W = (int(v) for v in probs.shape[:3])
        self.ctx.crf_decisions(probs, images, self.params, cid_map, out, replace_voids=replace_voids,
                               workspace=self._workspace(n, H, W), probs_out=probs_out)


def driver_for_crf(ctx, params):
    """The context's CRF driver for these settings (built on first use, kept on the context), or
    None when the settings ask for no refinement."""
    st = crf_settings(params)
    return cached_driver(ctx, '_crf_drivers', st, lambda: CRFDriver(ctx, st))
