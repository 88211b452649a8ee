"""Numpy reference of the mean-field CRF refinement (include/seg_hip.h at seg_crf_decisions),
parameterised on the dtype the arithmetic runs in (float64: the yardstick; float32: what the
kernel computes in, used to measure what the number format alone can move).

* offsets / tables: the neighbourhood in row-major (dy, dx) order without (0, 0) and the host
  tables ga, gs (double, rounded to float32) and inv2b, written from the header's text
  independently of estimator/crf.py and csrc/api.cpp.
* mean_field: Q^T of (P, I). The tables enter as float32; exp is np.exp; the message is
  accumulated in offset order and Z in channel order, both in dtype.
* decisions: the decision head on a probability tensor as tta_ref.tta_reference forms it:
  per-head first-maximum argmax, the hierarchical fusion (oracle.tfseg.TABLES), the cid map, the
  stable top-2 void replacement, the nearest align-corners resize (oracle.tfseg.nearest_ac_index).
* synthetic_inputs / CASES: the seeded inputs and (r, d, T) cases shared by the CPU precondition
  test and the GPU parity test; reference caches Q^T so that it is computed once and never
  modified.
"""
import functools

import numpy as np
import torch

from oracle.tfseg import TABLES, nearest_ac_index, resize_bilinear_ac

WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}
N_PP = {"cityscapes": 20, "vistas": 66}
IDENTITY_MAP = {"cityscapes": list(range(19)) + [-1], "vistas": list(range(65)) + [-1]}

DEFAULT_WEIGHTS = (4.0, 3.0)          # w_a, w_s
DEFAULT_THETAS = (67.0, 3.0, 3.0)     # theta_alpha, theta_beta, theta_gamma

BATCH, HW = 2, (37, 45)               # odd, ragged against any tile, below twice the largest halo
CASES = [(3, 1, 3), (2, 3, 5), (1, 1, 1), (5, 4, 2)]   # (r, d, T), default weights and thetas
TINY_HW, TINY_CASE = (5, 3), (5, 4, 2)                 # almost every neighbour outside the image


def offsets(r, d):
    return [(dy * d, dx * d) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
            if (dy, dx) != (0, 0)]


def tables(r, d, weights=DEFAULT_WEIGHTS, thetas=DEFAULT_THETAS):
    """(ga float32 [K], gs float32 [K], inv2b float32): formed in double, rounded to float."""
    wa, ws = (float(v) for v in weights)
    ta, tb, tg = (float(v) for v in thetas)
    o2 = np.array([oy * oy + ox * ox for oy, ox in offsets(r, d)], dtype=np.float64)
    ga = (wa * np.exp(-o2 / (2.0 * ta * ta))).astype(np.float32)
    gs = (ws * np.exp(-o2 / (2.0 * tg * tg))).astype(np.float32)
    sb = tb * 2.0 / 255.0
    return ga, gs, np.float32(1.0 / (2.0 * sb * sb))


def mean_field(P, I, r, d, T, weights=DEFAULT_WEIGHTS, thetas=DEFAULT_THETAS, widths=(14, 7, 3),
               dtype=np.float64):
    """P [N, H, W, CT], I [N, H, W, 3] -> Q^T [N, H, W, CT] in dtype."""
    P = np.asarray(P).astype(dtype)
    I = np.asarray(I).astype(dtype)
    N, H, W, CT = P.shape
    assert CT == sum(widths) and I.shape == (N, H, W, 3)
    ga, gs, inv2b = tables(r, d, weights, thetas)
    ga, gs, inv2b = ga.astype(dtype), gs.astype(dtype), dtype(inv2b)
    offs = offsets(r, d)
    # k_ij per offset on the region whose neighbour is inside the image (the image only)
    ks = []
    for o, (oy, ox) in enumerate(offs):
        y0, y1 = max(0, -oy), min(H, H - oy)
        x0, x1 = max(0, -ox), min(W, W - ox)
        if y0 >= y1 or x0 >= x1:
            ks.append(None)
            continue
        diff = I[:, y0:y1, x0:x1] - I[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        dist = diff[..., 0] * diff[..., 0]
        dist = dist + diff[..., 1] * diff[..., 1]
        dist = dist + diff[..., 2] * diff[..., 2]
        k = ga[o] * np.exp(-dist * inv2b) + gs[o]
        ks.append(((y0, y1, x0, x1), k.astype(dtype)))
    Q = P
    for _ in range(T):
        m = np.zeros_like(P)
        for (oy, ox), entry in zip(offs, ks):          # offset order
            if entry is None:
                continue
            (y0, y1, x0, x1), k = entry
            m[:, y0:y1, x0:x1] += k[..., None] * Q[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        new = np.empty_like(P)
        lo = 0
        for c in widths:
            mh, ph = m[..., lo:lo + c], P[..., lo:lo + c]
            v = (ph * np.exp(mh - mh.max(axis=-1, keepdims=True))).astype(dtype)
            z = np.zeros(v.shape[:-1], dtype=dtype)
            for j in range(c):                          # channel order
                z = z + v[..., j]
            ok = z >= dtype(1e-30)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = v * (dtype(1.0) / z)[..., None]
            new[..., lo:lo + c] = np.where(ok[..., None], q, ph)
            lo += c
        Q = new.astype(dtype)
    return Q


def head_argmax(Q, widths):
    """[N, H, W, 3] first-maximum argmax per head."""
    out, lo = [], 0
    for c in widths:
        out.append(np.argmax(Q[..., lo:lo + c], axis=-1))
        lo += c
    return np.stack(out, axis=-1)


def decisions(Q, dataset, cid_map, out_hw, replace_voids=False):
    """Decisions int64 [N, out_h, out_w] of probabilities Q [N, H, W, CT]."""
    c1, c2, c3 = WIDTHS[dataset]
    q = torch.as_tensor(np.array(Q)).permute(0, 3, 1, 2)   # a copy: Q may be a read-only cached array
    H, W = q.shape[2], q.shape[3]
    t = TABLES[dataset]
    lt = lambda v: torch.as_tensor(v, dtype=torch.long)
    s1, sv, sh = q[:, :c1], q[:, c1:c1 + c2], q[:, c1 + c2:]
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
    return d[:, hy][:, :, wx].numpy()


def _softmax_heads(u, widths):
    out, lo = [], 0
    for c in widths:
        out.append(torch.softmax(u[:, lo:lo + c], dim=1))
        lo += c
    return torch.cat(out, dim=1)


@functools.lru_cache(maxsize=None)
def synthetic_inputs(dataset, n=BATCH, hw=HW, seed_offset=0):
    """(P float32 [n, H, W, CT], I float32 [n, H, W, 3]). P: the per-head softmax of 2.0 x
    standard-normal logits [n, CT, 6, 7] upsampled align-corners to H x W. I: uniform(-1, 1)
    [n, 3, 5, 6] upsampled the same way plus uniform(-4, 4) grey levels of noise, quantised to the
    256 levels of the prepared image and mapped back to [-1, 1)."""
    widths = WIDTHS[dataset]
    H, W = hw
    rng = np.random.default_rng(20270 + (7 if dataset == "vistas" else 0) + seed_offset)
    logits = 2.0 * rng.standard_normal((n, sum(widths), 6, 7))
    coarse = rng.uniform(-1.0, 1.0, (n, 3, 5, 6))
    noise = rng.uniform(-4.0, 4.0, (n, H, W, 3)) * (2.0 / 255.0)
    P = _softmax_heads(resize_bilinear_ac(torch.as_tensor(logits), H, W), widths)
    P = P.permute(0, 2, 3, 1).contiguous().numpy().astype(np.float32)
    img = resize_bilinear_ac(torch.as_tensor(coarse), H, W).permute(0, 2, 3, 1).numpy() + noise
    level = np.clip(np.floor((img + 1.0) * 127.5 + 0.5), 0, 255)
    I = (level * (2.0 / 255.0) - 1.0).astype(np.float32)
    P.setflags(write=False)
    I.setflags(write=False)
    return P, I


@functools.lru_cache(maxsize=None)
def two_seed_inputs(dataset, hw=(64, 128)):
    """N = 2 at hw with image 1 drawn from a different seed than image 0."""
    a = synthetic_inputs(dataset, 1, hw, 11)
    b = synthetic_inputs(dataset, 1, hw, 23)
    P, I = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    P.setflags(write=False)
    I.setflags(write=False)
    return P, I


def tiny_inputs(dataset):
    return synthetic_inputs(dataset, 1, TINY_HW, 100)


@functools.lru_cache(maxsize=None)
def reference(dataset, case, dtype=np.float64, which="synthetic"):
    """Q^T of the cached inputs ``which`` ("synthetic", "tiny", "two_seed") for case (r, d, T) with
    the default weights and thetas; cached, shared by the tests, never modified by them."""
    P, I = {"synthetic": synthetic_inputs, "tiny": tiny_inputs, "two_seed": two_seed_inputs}[which](dataset)
    r, d, T = case
    Q = mean_field(P, I, r, d, T, widths=WIDTHS[dataset], dtype=dtype)
    Q.setflags(write=False)
    return Q


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
