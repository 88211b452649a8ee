"""Test-time augmentation for EVAL and PREDICT: multi-scale and flip inference.

The reference has no counterpart; the semantics are fixed in ``include/seg_hip.h`` at
``seg_tta_decisions``. With ``--tta_scales S [S ...]`` and / or ``--tta_flip`` the decisions of a
batch come from the per-head softmax probabilities averaged over one forward per entry: the
entries follow the scale order, each scale giving its unflipped entry and then, with flip, its
mirrored one. Every entry runs in a native context of its own size (``tta_sizes``) that shares
the primary context's parameters; the probabilities are averaged at the network size and never
written to memory (one ``seg_tta_decisions`` launch reads the entries' low-resolution logits).

This module imports without a GPU and without the library: torch and ``seg_hip`` are imported
where they are used.
"""
from __future__ import annotations

import copy
import math

from estimator.inference import Source, cached_driver

MAX_ENTRIES = 16   # SEG_TTA_MAX_ENTRIES: scales x (1 + flip) of one decision launch
NO_LOGITS = ('test-time augmentation (--tta_scales / --tta_flip) averages probabilities over several '
             'forwards; there are no full-resolution logits of the average (the *_probabilities '
             'entries hold it)')


def add_tta_arguments(argparser):
    """``--tta_scales`` / ``--tta_flip`` of evaluate.py and predict.py (off by default)."""
    argparser.add_argument(
        '--tta_scales', type=float, nargs='+', default=None, metavar='S',
        help='test-time augmentation: average the softmax probabilities over one forward per '
             'scale S of the network input (1.0 = the network size itself; any other S runs at '
             '8 * max(4, floor(S * size / 8 + 0.5)) per side). Default: none (one forward). '
             'With --replace_voids the voids are replaced from the top-2 of the averaged l1 '
             'probabilities at the network size, before the resize (the EVAL order).')
    argparser.add_argument(
        '--tta_flip', action='store_true',
        help='test-time augmentation: add the horizontally mirrored forward of every scale '
             '(of the network size alone without --tta_scales).')


def tta_settings(params):
    """(scales, flip) of the settings, or None when test-time augmentation is off."""
    scales = getattr(params, 'tta_scales', None)
    flip = bool(getattr(params, 'tta_flip', False))
    if not scales and not flip:
        return None
    return tuple(float(s) for s in (scales or [1.0])), flip


def tta_sizes(H, W, scales):
    """[(h, w)] of the forwards of ``scales`` at the base network size H x W: scale 1.0 is
    exactly (H, W); any other s gives 8 * max(4, floor(s * H / 8 + 0.5)) and likewise for W.
    Scales must be positive and map to distinct sizes."""
    def side(n, s):
        return 8 * max(4, int(math.floor(s * n / 8.0 + 0.5)))
    sizes = []
    for s in scales:
        s = float(s)
        if not (s > 0.0 and math.isfinite(s)):
            raise ValueError(f'tta_scales: scale {s!r} must be a positive number')
        hw = (int(H), int(W)) if s == 1.0 else (side(H, s), side(W, s))
        if hw in sizes:
            other = float(scales[sizes.index(hw)])
            raise ValueError(f'tta_scales: scales {other:g} and {s:g} both run at '
                             f'{hw[0]} x {hw[1]}; give one of them')
        sizes.append(hw)
    return sizes


class TTADriver(Source):
    """The scale contexts of one primary context and the per-batch entry loop (a source of
    ``estimator.inference``; the mean probabilities live at the network size).

    ``primary`` is the context ``model_fn`` runs (the network size H x W). One context per other
    size comes from ``get_context`` (so ``release_contexts()`` frees them), must lay its
    parameters out exactly as the primary does, and gets the primary's flat ``params`` and
    ``moving`` buffers copied whenever the primary's parameters were (re)loaded
    (``SegContext.params_version``; ``--eval_all_ckpts`` restores inside its loop)."""

    no_logits = NO_LOGITS

    def __init__(self, primary, config, params, mode, scales, flip):
        self.primary = primary
        self.scales = tuple(scales)
        self.flip = bool(flip)
        self.size = (primary.cfg.height, primary.cfg.width)
        self.sizes = tta_sizes(*self.size, self.scales)
        n_entries = len(self.sizes) * (2 if self.flip else 1)
        if n_entries > MAX_ENTRIES:
            raise ValueError(f'test-time augmentation: {len(self.sizes)} scales'
                             f'{" with flip" if self.flip else ""} are {n_entries} entries; at '
                             f'most {MAX_ENTRIES} fit one decision launch')
        self.contexts = [self._context(config, params, mode, s, hw) for s, hw in
                         zip(self.scales, self.sizes)]
        self._synced = None

    def _context(self, config, params, mode, scale, hw):
        from models.resnet50_extended_model_hierarchical import get_context
        p = self.primary
        if hw == (p.cfg.height, p.cfg.width):
            return p
        sp = copy.copy(params)
        sp.height_feature_extractor, sp.width_feature_extractor = hw
        try:
            ctx = get_context(config, sp, device=p.device.index, mode=mode)
        except RuntimeError as e:
            raise RuntimeError(f'tta scale {scale:g} ({hw[0]} x {hw[1]}): {e}') from e
        layout = lambda c: [(q.name, q.offset, q.numel) for q in c.param_info]
        assert layout(ctx) == layout(p) and ctx.n_train == p.n_train and ctx.n_moving == p.n_moving, (
            f'tta scale {scale:g}: the parameter layout of the {hw[0]} x {hw[1]} context differs '
            'from the primary context\'s')
        return ctx

    def sync(self):
        """Copy the primary's parameters and moving statistics into every scale context."""
        p = self.primary
        infer = bool(getattr(p, 'bn_inference', False))
        for ctx in self.contexts:
            if ctx is p:
                continue
            ctx.params.copy_(p.params)
            ctx.moving.copy_(p.moving)
            ctx.params_updated()
            ctx.set_bn_inference(infer)
        self._synced = (p.params_version, infer)

    def entries(self, proimages):
        """One forward per entry on ``proimages`` (device f32 [N, H, W, 3] in [-1, 1)); returns
        [(low-resolution logits, flip)] in entry order. The logits are clones: the flipped run of
        a context overwrites its unflipped logits. The primary context's last forward was on
        ``proimages`` (``model_fn`` has run), so its unflipped entry is there already.
        Afterwards a context's own state (``outputs()``, ``predict``, ``full_predictions``) is
        that of the last entry it ran: with flip, the primary's is the mirrored image's."""
        from seg_hip import resize_images
        p = self.primary
        if self._synced != (p.params_version, bool(getattr(p, 'bn_inference', False))):
            self.sync()
        x = proimages.contiguous()
        out = []
        for ctx in self.contexts:
            h, w = ctx.cfg.height, ctx.cfg.width
            for flip in ((False, True) if self.flip else (False,)):
                if not (ctx is p and not flip):   # the primary's unflipped forward is model_fn's
                    ctx.forward(resize_images(x, h, w, flip))
                out.append((ctx.outputs()[2].clone(), flip))
        return out

    def decide(self, entries, cid_map, out, replace_voids=False, mean_probs=None):
        """One ``seg_tta_decisions`` launch over ``entries`` into ``out`` (device int32 [N, Ho, Wo])."""
        self.primary.tta_decisions(entries, cid_map, out, replace_voids=replace_voids,
                                   mean_probs=mean_probs)

    def primary_entry(self):
        """Index of the primary context's unflipped entry, or None when no scale runs at the
        network size."""
        if self.primary not in self.contexts:
            return None
        return self.contexts.index(self.primary) * (2 if self.flip else 1)

    def attach(self, predictions, entries, refined=None):
        """Under test-time augmentation the model's lazy full-resolution entries come from the
        averaged probabilities (or ``refined``): ``*_probabilities`` are slices of them,
        ``*_decisions`` their per-head argmax, and ``*_logits`` do not exist.

        The eager ``*_logits_lowres`` entries are views of the primary context's output buffer, which
        the primary's mirrored forward has overwritten when flip is on: they are replaced by slices
        of the clone of its unflipped logits, so they keep describing ``proimages`` itself."""
        from models.resnet50_extended_model_hierarchical import HEADS
        i = self.primary_entry()
        if i is not None:
            lo = 0
            for head, ci in zip(HEADS, self.primary.head_widths):
                predictions[f'{head}_logits_lowres'] = entries[i][0][..., lo:lo + ci]
                lo += ci
        super().attach(predictions, entries, refined)


def driver_for(ctx, config, params, mode):
    """The primary context's driver for these settings (built on first use, kept on the
    context), or None when the settings ask for no test-time augmentation."""
    st = tta_settings(params)
    return cached_driver(ctx, '_tta_drivers', st and (st, mode),
                         lambda: TTADriver(ctx, config, params, mode, *st))
