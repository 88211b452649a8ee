"""Float64 restatement of the bootstrapped per-pixel l1 loss (seg_set_bootstrap in
include/seg_hip.h), built from the oracle's own pieces:

  m    = the l1 sparse softmax-CE of the align-corners upsampled l1 logits of the strong images
         where the l1 weight is 1, exactly 0 elsewhere                       (l1_loss_map)
  K    = max(1, p * M // 100), M = npp * H * W                                (k_of)
  tau  = the K-th largest of the M entries of m                               (threshold)
  mask = l1 weight & (m >= tau), ties at tau all selected                     (select_mask)
  l1   = sum(m over mask) / count(mask), seg = l1 + 0.1 * (l2v + l2h), both l2 terms as the
         oracle computes them                                                 (losses_with_mask)
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.tfseg import TABLES, resize_bilinear_ac, weighted_loss, xent


def k_of(p: int, M: int) -> int:
    """K of a percentage p in 1..100 over M map entries (64-bit integer arithmetic)."""
    if not 1 <= p <= 100:
        raise ValueError(f"bootstrapping percentage {p} outside 1..100")
    return max(1, (int(p) * int(M)) // 100)


def is_on(p) -> bool:
    """p <= 0 is off; > 100 is an error."""
    if p > 100:
        raise ValueError(f"bootstrapping_percentage {p}: must be at most 100")
    return p > 0


def l1_weight(cfg, px_labels):
    """bool [npp, H, W]: l1 label <= max(pp2l1) - 1 (define_losses_hierarchical.py:129-140)."""
    t = TABLES[cfg.dataset]
    l1lab = np.asarray(t["pp2l1"], np.int64)[np.asarray(px_labels, np.int64)]
    return l1lab <= max(t["pp2l1"]) - 1


def _l1_raw(cfg, l1_low, px_labels, dtype=torch.float64):
    """Per-pixel l1 cross-entropy [npp, H, W] of low-res l1 logits [N, C1, Hl, Wl] (torch, keeps
    the autograd graph) for the strong slice."""
    t = TABLES[cfg.dataset]
    up = resize_bilinear_ac(l1_low[:cfg.nb_pp].to(dtype), cfg.height, cfg.width)
    l1lab = torch.as_tensor(np.asarray(t["pp2l1"], np.int64))[torch.as_tensor(np.asarray(px_labels, np.int64))]
    onehot = F.one_hot(l1lab, up.shape[1]).permute(0, 3, 1, 2).to(dtype)
    return xent(up, onehot)


def l1_loss_map(cfg, l1_low, px_labels):
    """(m float64 [npp, H, W], weight bool [npp, H, W])."""
    w = l1_weight(cfg, px_labels)
    raw = _l1_raw(cfg, torch.as_tensor(l1_low).detach(), px_labels).numpy()
    return np.where(w, np.maximum(raw, 0.0), 0.0), w


def threshold(m, k: int):
    """The k-th largest entry of m (counted over all entries)."""
    flat = np.sort(np.asarray(m).ravel())
    return flat[flat.size - k]


def select_mask(m, w, tau):
    return w & (m >= tau)


def bootstrap(cfg, l1_low, px_labels, p: int):
    """(m, tau, mask, K) of percentage p on these logits and labels."""
    m, w = l1_loss_map(cfg, l1_low, px_labels)
    k = k_of(p, m.size)
    tau = threshold(m, k)
    return m, tau, select_mask(m, w, tau), k


def losses_with_mask(net, low, px_labels, bbox_soft, tag_soft, mask, weak_l1_decisions=None):
    """OracleNet.losses with the l1 weights replaced by `mask` (bool [npp, H, W]); `low` may
    require grad. Returns the oracle's dict with 'segmentation', 'l1_segmentation' and 'counts'
    restated under the mask; the l2 terms are the oracle's own."""
    L = net.losses(low, px_labels, bbox_soft, tag_soft, weak_l1_decisions=weak_l1_decisions)
    raw = _l1_raw(net.cfg, low["l1_logits"], px_labels, dtype=net.dtype)
    l1, n1 = weighted_loss(raw, torch.as_tensor(mask).to(net.dtype))
    out = dict(L)
    out["l1_segmentation"] = l1
    out["segmentation"] = l1 + 0.1 * (L["l2_vehicle_segmentation"] + L["l2_human_segmentation"])
    out["counts"] = (n1,) + tuple(L["counts"][1:])
    return out
