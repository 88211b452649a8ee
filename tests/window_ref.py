"""Torch reference of the sliding-window decision head (seg_window_decisions), parameterised on
the dtype the arithmetic runs in (float64: the yardstick; float32: what the kernel computes in,
used to measure how many decisions the number format alone can move).

* window_reference: per entry, in entry order (rows of ys outermost, then xs, then with flip the
  unflipped entry followed by the mirrored one), the align-corners upsampling
  (oracle.tfseg.resize_bilinear_ac) to the window size, read at column W - 1 - x for a mirrored
  entry, and the per-head softmax, added into the window's slice of the canvas; the coverage
  count k per pixel; mean = sum / k; then the decisions on the sums as tta_ref.tta_reference
  forms them: per-head first-maximum argmax, the hierarchical fusion (oracle.tfseg.TABLES), the
  cid map, the stable top-2 void replacement and the nearest align-corners resize
  (oracle.tfseg.nearest_ac_index) from the canvas.
* origins: the geometry rule written out independently of estimator/windows.py.
* synthetic_entries: the seeded logits shared by the CPU precondition test and the GPU tests;
  synthetic_reference caches their references so that they are computed once and never modified.
"""
import functools

import numpy as np
import torch

from oracle.tfseg import TABLES, nearest_ac_index, resize_bilinear_ac

WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}
N_PP = {"cityscapes": 20, "vistas": 66}
IDENTITY_MAP = {"cityscapes": list(range(19)) + [-1], "vistas": list(range(65)) + [-1]}

# the synthetic case: network = window size, canvas, stride, low-resolution size, batch
NET_HW = (64, 128)
CANVAS_HW = (100, 200)
STRIDE = (24, 40)
LOW_HW = (8, 16)
BATCH = 2


def origins(C, n, s):
    """i * s while i * s < C - n, then C - n."""
    out, i = [], 0
    while i * s < C - n:
        out.append(i * s)
        i += 1
    return out + [C - n]


def placements(ys, xs, flip):
    """[(y0, x0, mirrored)] in entry order."""
    return [(y0, x0, f) for y0 in ys for x0 in xs for f in ((False, True) if flip else (False,))]


def window_reference(entries, ys, xs, flip, net_hw, canvas_hw, dataset, cid_map, out_hw,
                     replace_voids=False, dtype=torch.float64):
    """entries: logits [N, h_low, w_low, >= CT] (numpy or tensor) in entry order. Returns (mean
    probabilities [N, Hc, Wc, CT] in dtype, decisions int64 [N, out_h, out_w], coverage count
    int64 [Hc, Wc], stats), the first three numpy."""
    c1, c2, c3 = WIDTHS[dataset]
    ct = c1 + c2 + c3
    H, W = net_hw
    Hc, Wc = canvas_hw
    place = placements(ys, xs, flip)
    assert len(entries) == len(place)
    n = np.asarray(entries[0]).shape[0]
    total = torch.zeros((n, ct, Hc, Wc), dtype=dtype)
    count = torch.zeros((Hc, Wc), dtype=torch.long)
    for lg, (y0, x0, mirrored) in zip(entries, place):
        x = torch.as_tensor(np.asarray(lg))[..., :ct].permute(0, 3, 1, 2).to(dtype)
        up = resize_bilinear_ac(x, H, W)
        if mirrored:
            up = torch.flip(up, dims=(3,))      # u at column W - 1 - x
        p = torch.cat([torch.softmax(up[:, :c1], dim=1), torch.softmax(up[:, c1:c1 + c2], dim=1),
                       torch.softmax(up[:, c1 + c2:], dim=1)], dim=1)
        total[:, :, y0:y0 + H, x0:x0 + W] += p   # 0 + p is p: the sum starts from the first entry
        count[y0:y0 + H, x0:x0 + W] += 1
    assert int(count.min()) >= 1
    mean = total * (torch.ones((), dtype=dtype) / count.to(dtype))
    t = TABLES[dataset]
    lt = lambda v: torch.as_tensor(v, dtype=torch.long)
    s1, sv, sh = total[:, :c1], total[:, c1:c1 + c2], total[:, c1 + c2:]
    l1d, vd, hd = (torch.argmax(s, dim=1) for s in (s1, sv, sh))     # first maximum
    fused = torch.where(l1d == t["cid_l1_vehicle"], lt(t["veh_to_common"])[vd],
                        torch.where(l1d == t["cid_l1_human"], lt(t["hum_to_common"])[hd],
                                    lt(t["l1_to_common"])[l1d]))
    m = np.asarray(cid_map, dtype=np.int64)
    m = np.where(m == -1, m.max() + 1, m)              # utils._replacevoids
    d = torch.as_tensor(m)[fused]
    if replace_voids:
        order = torch.sort(-s1, dim=1, stable=True).indices   # top_k(k = 2), stable
        d = torch.where(d == c1 - 1, order[:, 1], order[:, 0])
    hy = nearest_ac_index(Hc, out_hw[0])
    wx = nearest_ac_index(Wc, out_hw[1])
    d = d[:, hy][:, :, wx]
    stats = {"vehicle": float((l1d == t["cid_l1_vehicle"]).double().mean()),
             "human": float((l1d == t["cid_l1_human"]).double().mean())}
    return mean.permute(0, 2, 3, 1).contiguous().numpy(), d.numpy(), count.numpy(), stats


def synthetic_grid(canvas_hw=CANVAS_HW):
    return origins(canvas_hw[0], NET_HW[0], STRIDE[0]), origins(canvas_hw[1], NET_HW[1], STRIDE[1])


def synthetic_entries(dataset, amplitude, canvas_hw=CANVAS_HW, flip=True):
    """The seeded synthetic entries of the grid of canvas_hw at STRIDE: amplitude x standard
    normal logits [BATCH, 8, 16, CT] float32, drawn in entry order."""
    ct = sum(WIDTHS[dataset])
    rng = np.random.default_rng(30260 + int(round(10 * amplitude)) + (7 if dataset == "vistas" else 0))
    ys, xs = synthetic_grid(canvas_hw)
    return [(amplitude * rng.standard_normal((BATCH,) + LOW_HW + (ct,))).astype(np.float32)
            for _ in placements(ys, xs, flip)]


@functools.lru_cache(maxsize=None)
def synthetic_reference(dataset, amplitude, out_hw, replace_voids, dtype, canvas_hw=CANVAS_HW):
    """window_reference of synthetic_entries(dataset, amplitude, canvas_hw) with flip and the
    identity map (last class void); cached, shared by the tests, never modified by them."""
    ys, xs = synthetic_grid(canvas_hw)
    return window_reference(synthetic_entries(dataset, amplitude, canvas_hw), ys, xs, True, NET_HW,
                            canvas_hw, dataset, IDENTITY_MAP[dataset], out_hw, replace_voids, dtype)
