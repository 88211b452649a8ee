"""The one inference path of EVAL and PREDICT: a probability source, an optional refinement, one
decide step.

A **source** turns the prepared batch into per-head softmax probabilities: ``ForwardSource`` (the
one forward ``model_fn`` ran), ``estimator.tta.TTADriver`` (one forward per scale and flip) or
``estimator.windows.WindowDriver`` (one forward per window of a canvas). All three have

* ``entries(images)``: the forwards of a batch, in a form only the source reads;
* ``decide(entries, cid_map, out, replace_voids)``: the decisions in one launch that writes no
  probabilities (the multi-entry sources also take ``mean_probs``);
* ``size``: the (height, width) the probabilities live at, the network size or the canvas;
* ``mean_probabilities(entries)``: the probabilities themselves, f32 [N, size, c1 + c2 + c3];
* ``attach(predictions, entries, refined)``: what the model's lazy predictions then hold.

``decide_batch`` picks the source from the settings, lets ``estimator.crf`` refine its probabilities
when ``--crf_iterations`` asks for it, and attaches the lazy predictions: the EVAL and the PREDICT
spec call nothing else.

This module imports without a GPU and without the library: torch and ``seg_hip`` are imported
where they are used.
"""
from __future__ import annotations


def cached_driver(ctx, attr, key, build):
    """The driver of ``ctx`` for ``key`` (``build()`` on first use, kept in the dict ``ctx.attr``),
    or None when ``key`` is None: the settings switch the feature off."""
    if key is None:
        return None
    cache = ctx.__dict__.setdefault(attr, {})
    if key not in cache:
        cache[key] = build()
    return cache[key]


def head_entries(probs, widths):
    """The lazy ``*_probabilities`` (per-head slices of ``probs``, f32 [N, H, W, c1 + c2 + c3]) and
    ``*_decisions`` (their argmax) entries of the model's predictions."""
    import torch
    from models.resnet50_extended_model_hierarchical import HEADS
    out, lo = {}, 0
    for head, ci in zip(HEADS, widths):
        out[f'{head}_probabilities'] = probs[..., lo:lo + ci]
        out[f'{head}_decisions'] = torch.argmax(probs[..., lo:lo + ci], dim=-1).to(torch.int32)
        lo += ci
    return out


class Source(object):
    """What the multi-entry sources share. A subclass sets ``primary`` (the context ``model_fn``
    runs) and ``size``, and defines ``entries`` and ``decide``."""

    no_logits = None   # why the predictions have no ``*_logits`` under this source, if they have none

    def decisions(self, images, cid_map, out, replace_voids=False):
        """Decisions of the batch into ``out`` (device int32 [N, Ho, Wo]); returns the entries."""
        ents = self.entries(images)
        self.decide(ents, cid_map, out, replace_voids)
        return ents

    def mean_probabilities(self, entries):
        """Mean probabilities f32 [N, size, c1 + c2 + c3] of ``entries``. This launches the decision
        head over all entries a second time (the decisions path keeps no full-resolution tensor),
        which is the price of asking for them."""
        import torch
        p = self.primary
        shape = (p.batch_size,) + tuple(self.size)
        probs = torch.empty(shape + (sum(p.head_widths),), dtype=torch.float32, device=p.device)
        decs = torch.empty(shape, dtype=torch.int32, device=p.device)
        self.decide(entries, list(range(p.n_classes)), decs, mean_probs=probs)
        return probs

    def attach(self, predictions, entries, refined=None):
        """The lazy ``*_probabilities`` / ``*_decisions`` come from ``refined`` (Q^T of the CRF) or,
        without it, from the mean probabilities, computed when one of them is first read."""
        from models.resnet50_extended_model_hierarchical import LAZY_KEYS
        probs = (lambda: refined) if refined is not None else (lambda: self.mean_probabilities(entries))
        logits = tuple(k for k in LAZY_KEYS if k.endswith('_logits'))
        predictions.replace_lazy(tuple(k for k in LAZY_KEYS if k not in logits),
                                 lambda: head_entries(probs(), self.primary.head_widths),
                                 absent=logits if self.no_logits else (), why=self.no_logits)


class ForwardSource(Source):
    """The one forward ``model_fn`` ran on the batch. ``order``: where ``--replace_voids`` replaces,
    as in ``SegContext.predict`` ("eval" before the resize, "predict" after it)."""

    def __init__(self, ctx, order='eval'):
        self.primary = ctx
        self.size = (ctx.cfg.height, ctx.cfg.width)
        self.order = order

    def entries(self, images):
        return None   # the context's own logits

    def decide(self, entries, cid_map, out, replace_voids=False):
        self.primary.predict(cid_map, out, replace_voids=replace_voids, order=self.order)

    def mean_probabilities(self, entries):
        """The probabilities of the forward: ``probs_out`` of ``seg_full_predictions``."""
        import torch
        p = self.primary
        probs = torch.empty((p.batch_size,) + self.size + (sum(p.head_widths),), dtype=torch.float32,
                            device=p.device)
        p.full_predictions(probs=probs)
        return probs

    def attach(self, predictions, entries, refined=None):
        if refined is not None:   # without a refinement the model's own lazy entries stand
            super().attach(predictions, entries, refined)


def pick_source(ctx, config, params, mode, order='eval'):
    """The probability source the settings name: ``--window_canvas``, else ``--tta_scales`` /
    ``--tta_flip``, else the forward ``model_fn`` ran, which alone honours ``order``."""
    from estimator.tta import driver_for
    from estimator.windows import driver_for_windows
    return (driver_for_windows(ctx, config, params, mode) or driver_for(ctx, config, params, mode)
            or ForwardSource(ctx, order))


def decide_batch(predictions, images, ctx, config, params, mode, cid_map, decs, replace_voids,
                 order='eval'):
    """The decisions of the batch ``images`` into ``decs`` (device int32 [N, Ho, Wo]), mapped through
    ``cid_map``, from the source the settings name: ``--window_canvas`` (``images`` is the canvas),
    else ``--tta_scales`` / ``--tta_flip``, else the forward ``model_fn`` ran, which alone honours
    ``order``. With ``--crf_iterations`` the source's probabilities are refined on ``images`` before
    the argmax, and ``--replace_voids`` replaces before the resize whatever ``order`` says.
    ``predictions`` (the model's, of ``ctx``) get the matching lazy entries."""
    import torch
    from estimator.crf import driver_for_crf
    source = pick_source(ctx, config, params, mode, order)
    crf = driver_for_crf(ctx, params)
    entries = source.entries(images)
    refined = None
    if crf is None:
        source.decide(entries, cid_map, decs, replace_voids)
    else:
        probs = source.mean_probabilities(entries)
        refined = torch.empty_like(probs)
        crf.decisions(probs, images, cid_map, decs, replace_voids, probs_out=refined)
    source.attach(predictions, entries, refined)
