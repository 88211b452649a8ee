"""Torch / numpy references of the test-time augmentation kernels, parameterised on the dtype
the arithmetic runs in (float64: the yardstick; float32: what the kernels compute in, used to
measure how many decisions the number format alone can move).

* resize_images_ref: seg_resize_images -- TF 1.12's legacy bilinear resize with align_corners =
  False of an fp32 NHWC image, mirrored in x first when flip. The index / lerp tables are fp32
  (they are part of the definition, as in oracle.tfseg.prepare_images_np); the lerps run in dtype.
* tta_reference: seg_tta_decisions -- per entry the align-corners upsampling
  (oracle.tfseg.resize_bilinear_ac) read at column W - 1 - x for a flipped entry, the per-head
  softmax, the sum in entry order times 1 / E, the per-head first-maximum argmax, the
  hierarchical fusion (oracle.tfseg.TABLES), the cid map, the stable top-2 void replacement and
  the nearest align-corners resize (oracle.tfseg.nearest_ac_index).
* synthetic_entries: the seeded logits shared by the CPU precondition test and the GPU parity
  test; synthetic_reference caches their references so they are computed once.
"""
import functools

import numpy as np
import torch

from oracle.tfseg import TABLES, nearest_ac_index, resize_bilinear_ac

WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}
N_PP = {"cityscapes": 20, "vistas": 66}

# (h_low, w_low) of the synthetic entries, each with and without flip; network size and batch
LOW_SIZES = [(4, 8), (6, 12), (8, 16), (10, 20), (13, 13)]
NET_HW = (64, 128)
BATCH = 2


def legacy_tables(n_in, n_out):
    """TF 1.12 legacy scaler, align_corners = False: scale = float(in) / float(out), in_f = o *
    scale, lo = (int)in_f, hi = min(lo + 1, in - 1), lerp = in_f - lo, all in float32."""
    scale = np.float32(np.float32(n_in) / np.float32(n_out))
    fin = (np.arange(n_out, dtype=np.float32) * scale).astype(np.float32)
    lo = fin.astype(np.int64)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, (fin - lo.astype(np.float32)).astype(np.float32)


def resize_images_ref(x, h_out, w_out, flip=False, dtype=np.float64):
    """x [n, H, W, 3] -> [n, h_out, w_out, 3] in dtype."""
    x = np.asarray(x).astype(dtype)
    if flip:
        x = x[:, :, ::-1]          # the mirror, then the resize
    yl, yh, ylr = legacy_tables(x.shape[1], h_out)
    xl, xh, xlr = legacy_tables(x.shape[2], w_out)
    ylr = ylr.astype(dtype)[None, :, None, None]
    xlr = xlr.astype(dtype)[None, None, :, None]
    tl, tr = x[:, yl][:, :, xl], x[:, yl][:, :, xh]
    bl, br = x[:, yh][:, :, xl], x[:, yh][:, :, xh]
    top = tl + (tr - tl) * xlr
    bot = bl + (br - bl) * xlr
    return (top + (bot - top) * ylr).astype(dtype)


def tta_reference(entries, net_hw, dataset, cid_map, out_hw, replace_voids=False,
                  dtype=torch.float64):
    """entries: [(logits [N, h_low, w_low, >= CT] numpy or tensor, flip)]. Returns (mean
    probabilities [N, H, W, CT] in dtype, decisions int64 [N, out_h, out_w]), both numpy."""
    c1, c2, c3 = WIDTHS[dataset]
    ct = c1 + c2 + c3
    H, W = net_hw
    total = None
    for lg, flip in entries:
        x = torch.as_tensor(np.asarray(lg))[..., :ct].permute(0, 3, 1, 2).to(dtype)
        up = resize_bilinear_ac(x, H, W)
        if flip:
            up = torch.flip(up, dims=(3,))      # u_e at column W - 1 - x
        p = torch.cat([torch.softmax(up[:, :c1], dim=1), torch.softmax(up[:, c1:c1 + c2], dim=1),
                       torch.softmax(up[:, c1 + c2:], dim=1)], dim=1)
        total = p if total is None else total + p
    one = torch.ones((), dtype=dtype)
    mean = total * (one / torch.as_tensor(float(len(entries)), dtype=dtype))
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
    hy = nearest_ac_index(H, out_hw[0])
    wx = nearest_ac_index(W, out_hw[1])
    d = d[:, hy][:, :, wx]
    stats = {"vehicle": float((l1d == t["cid_l1_vehicle"]).double().mean()),
             "human": float((l1d == t["cid_l1_human"]).double().mean())}
    return mean.permute(0, 2, 3, 1).contiguous().numpy(), d.numpy(), stats


def synthetic_entries(dataset, amplitude, extra_low=()):
    """The seeded synthetic entries: for every size of LOW_SIZES (+ extra_low) an unflipped and a
    flipped entry of amplitude x standard normal logits [BATCH, h, w, CT] float32."""
    ct = sum(WIDTHS[dataset])
    rng = np.random.default_rng(20260 + int(round(amplitude * 10)) + (7 if dataset == "vistas" else 0))
    out = []
    for (h, w) in list(LOW_SIZES) + list(extra_low):
        for flip in (False, True):
            out.append(((amplitude * rng.standard_normal((BATCH, h, w, ct))).astype(np.float32), flip))
    return out


IDENTITY_MAP = {"cityscapes": list(range(19)) + [-1], "vistas": list(range(65)) + [-1]}


@functools.lru_cache(maxsize=None)
def synthetic_reference(dataset, amplitude, extra_low, out_hw, replace_voids, dtype):
    """tta_reference of synthetic_entries(dataset, amplitude, extra_low) with the identity map
    (last class void); cached, shared by the tests, never modified by them."""
    return tta_reference(synthetic_entries(dataset, amplitude, extra_low), NET_HW, dataset,
                         IDENTITY_MAP[dataset], out_hw, replace_voids, dtype)
