"""Numpy reference of the box-constrained pseudo-labels (include/seg_hip.h at seg_box_constrain),
parameterised on the dtype the arithmetic runs in (float64: the yardstick; float32: what the
kernels compute in).

* cover: per box, the pixels of the probability map it covers, from
  input_pipelines.weak_labels.bbox_label_map(...) > 0 on the box alone: the rasteriser the
  training path is pinned to.
* constrain / decide / rejects / finalize: (a), (b), the reject rule and (c) of the header, with the
  tables of oracle.tfseg.TABLES.
* box_lists / CASES / inputs: the seeded cases shared by the CPU and the GPU tests (probabilities
  from crf_ref.synthetic_inputs); the references are cached and never modified.
"""
import functools

import numpy as np

from crf_ref import N_PP, WIDTHS, synthetic_inputs
from input_pipelines.weak_labels import BoxLists, bbox_label_map
from oracle.tfseg import TABLES, nearest_ac_index

HW = (37, 45)                                   # 1665 pixels: a ragged last block at 128 and 256
OUT_SIZES = [(37, 45), (75, 44), (111, 95)]
TAU, MIN_FILL = 0.15, 0.02                      # fixtures of the tests, not recommendations
N_WEAK = 14                                     # weak classes 0..13


def kinds(dataset):
    """Per weak class 0..13: (vehicle channel or -1, human channel or -1, expected training cid or
    -1 for an inert class)."""
    t = TABLES[dataset]
    _, c2, c3 = WIDTHS[dataset]
    out = []
    for k in range(N_WEAK):
        v = t["pb2veh"][k] if t["pb2veh"][k] != c2 - 1 else -1
        h = t["pb2hum"][k] if t["pb2hum"][k] != c3 - 1 else -1
        tgt = t["veh_to_common"][v] if v >= 0 else t["hum_to_common"][h] if h >= 0 else -1
        out.append((v, h, tgt))
    return out


def box_kinds(dataset):
    """What seg_box_kinds reports: per weak class 1 vehicle, 2 human, 0 inert."""
    return [1 if v >= 0 else 2 if h >= 0 else 0 for v, h, _ in kinds(dataset)]


def cover(items, hw):
    """Per image a bool array [k_i, H, W]: box b covers pixel (y, x) of the hw map."""
    out = []
    for cids, coords, src, rs, off in items:
        c = np.zeros((len(cids),) + tuple(hw), dtype=bool)
        for b, (cid, xy) in enumerate(zip(cids, coords)):
            c[b] = bbox_label_map([int(cid)], [xy], src, rs, off, hw)[..., int(cid)] > 0
        out.append(c)
    return out


def masks(items, covers, hw):
    """uint16 [n, H, W]: bit k = some box of class k covers the pixel."""
    m = np.zeros((len(items),) + tuple(hw), dtype=np.uint16)
    for i, (it, c) in enumerate(zip(items, covers)):
        for b, cid in enumerate(it[0]):
            m[i] |= (c[b].astype(np.uint16) << np.uint16(int(cid)))
    return m


def allowed(mask, dataset):
    """(AV bool [n, H, W, c2], AH bool [n, H, W, c3]) of a mask."""
    _, c2, c3 = WIDTHS[dataset]
    av = np.zeros(mask.shape + (c2,), dtype=bool)
    ah = np.zeros(mask.shape + (c3,), dtype=bool)
    for k, (v, h, _) in enumerate(kinds(dataset)):
        bit = (mask >> np.uint16(k)) & np.uint16(1) > 0
        if v >= 0:
            av[..., v] |= bit
        if h >= 0:
            ah[..., h] |= bit
    return av, ah


def _constrain_head(ph, a, dtype):
    s = np.zeros(ph.shape[:-1], dtype=dtype)
    for c in range(ph.shape[-1]):                       # channel order
        s = s + np.where(a[..., c], ph[..., c], dtype(0))
    ok = a.any(-1) & (s >= dtype(1e-30))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(a, ph * (dtype(1.0) / s)[..., None], dtype(0))
    return np.where(ok[..., None], q, ph).astype(dtype)


def constrain(P, mask, dataset, dtype=np.float64):
    """(a): P' in dtype."""
    c1, c2, _ = WIDTHS[dataset]
    P = np.asarray(P).astype(dtype)
    av, ah = allowed(mask, dataset)
    out = P.copy()
    out[..., c1:c1 + c2] = _constrain_head(P[..., c1:c1 + c2], av, dtype)
    out[..., c1 + c2:] = _constrain_head(P[..., c1 + c2:], ah, dtype)
    return out


def _first_max_allowed(q, a):
    return np.argmax(np.where(a, q, -np.inf), axis=-1)


def decide(Q, items, covers, mask, dataset, tau, dtype=np.float64):
    """(b): (labels int32 [n, H, W], conf dtype [n, H, W], counts int32 [total, 2]). tau is the
    float the entry takes."""
    t = TABLES[dataset]
    c1, c2, _ = WIDTHS[dataset]
    ignore = N_PP[dataset] - 1
    Q = np.asarray(Q).astype(dtype)
    av, ah = allowed(mask, dataset)
    d1 = np.argmax(Q[..., :c1], axis=-1)
    conf = np.take_along_axis(Q[..., :c1], d1[..., None], -1)[..., 0]
    dv = _first_max_allowed(Q[..., c1:c1 + c2], av)
    dh = _first_max_allowed(Q[..., c1 + c2:], ah)
    lv = np.where(av.any(-1), np.asarray(t["veh_to_common"])[dv], ignore)
    lh = np.where(ah.any(-1), np.asarray(t["hum_to_common"])[dh], ignore)
    labels = np.where(d1 == t["cid_l1_vehicle"], lv,
                      np.where(d1 == t["cid_l1_human"], lh, np.asarray(t["l1_to_common"])[d1]))
    labels = np.where(conf >= dtype(np.float32(tau)), labels, ignore).astype(np.int32)
    counts = []
    kd = kinds(dataset)
    for i, (it, c) in enumerate(zip(items, covers)):
        for b, cid in enumerate(it[0]):
            tgt = kd[int(cid)][2]
            counts.append((int(c[b].sum()), int((c[b] & (labels[i] == tgt)).sum()) if tgt >= 0 else 0))
    return labels, conf, np.asarray(counts, dtype=np.int32).reshape(-1, 2)


def all_cids(items):
    return np.concatenate([np.asarray(it[0], dtype=np.int64).reshape(-1) for it in items]
                          + [np.zeros(0, np.int64)])


def rejects(counts, cids, dataset, min_fill):
    """The host rule: 1 for a vehicle or human box with area > 0 and hit < min_fill * area (float64)."""
    kd = kinds(dataset)
    counts = np.asarray(counts, dtype=np.float64).reshape(-1, 2)
    live = np.asarray([kd[int(k)][2] >= 0 for k in cids], dtype=bool)
    return (live & (counts[:, 0] > 0) & (counts[:, 1] < float(min_fill) * counts[:, 0])).astype(np.int32)


def finalize(labels, covers, reject, out_hw, dataset):
    """(c): int32 [n, out_h, out_w]."""
    ignore = N_PP[dataset] - 1
    H, W = labels.shape[1:]
    hy, wx = nearest_ac_index(H, out_hw[0]).numpy(), nearest_ac_index(W, out_hw[1]).numpy()
    out = np.empty((labels.shape[0],) + tuple(out_hw), dtype=np.int32)
    b0 = 0
    for i, c in enumerate(covers):
        rj = np.asarray(reject[b0:b0 + len(c)]) != 0
        b0 += len(c)
        dead = c[rj].any(0) if rj.any() else np.zeros((H, W), dtype=bool)
        out[i] = np.where(dead, ignore, labels[i])[hy][:, wx]
    return out


# ---- the seeded cases ------------------------------------------------------------------------

def _geom(src, crop):
    """(src, resized, offset) of an HW map: the map itself, or a crop of a slightly larger resize."""
    return (src, (HW[0] + 3, HW[1] + 5), (2, 3)) if crop else (src, HW, (0, 0))


def _random_boxes(rng, k, max_extent):
    lo = rng.random((k, 2)).astype(np.float32)
    ext = (rng.random((k, 2)) * max_extent).astype(np.float32)
    hi = np.minimum(lo + ext, np.float32(1.0))
    return np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]], 1).astype(np.float32)


# (xmin, xmax, ymin, ymax): a vehicle box ending at exactly 1.0 on both axes; two overlapping boxes
# of one vehicle class; a human box under a vehicle box; a box one source pixel wide; inert boxes
_HAND = [(0, (0.40, 1.0, 0.35, 1.0)),
         (2, (0.05, 0.45, 0.05, 0.60)), (2, (0.25, 0.70, 0.30, 0.80)),
         (7, (0.30, 0.80, 0.20, 0.70)), (4, (0.35, 0.75, 0.25, 0.65)),
         (6, (0.52, 0.525, 0.10, 0.90)),
         (12, (0.0, 0.5, 0.5, 1.0)), (11, (0.6, 0.9, 0.0, 0.3)),
         (9, (0.02, 0.30, 0.55, 0.98)), (5, (0.55, 0.98, 0.02, 0.40))]


def _hand_item(rng, src, crop, extra):
    cids = [c for c, _ in _HAND] + list(rng.integers(0, N_WEAK, size=extra))
    coords = np.concatenate([np.asarray([b for _, b in _HAND], np.float32),
                             _random_boxes(rng, extra, 0.3)]).astype(np.float32)
    return (np.asarray(cids, np.int64), coords) + _geom(src, crop)


@functools.lru_cache(maxsize=None)
def box_lists(case):
    """'n2': two images, hand-made boxes at source 50 x 70 (nearest up-sampling) and 1024 small
    boxes at source 111 x 95 (down-sampling, cropped). 'n3': three images, the middle one without
    a box."""
    rng = np.random.default_rng({"n2": 4101, "n3": 4102}[case])
    if case == "n2":
        many = (rng.integers(0, N_WEAK, size=1024).astype(np.int64), _random_boxes(rng, 1024, 0.08))
        return BoxLists([_hand_item(rng, (50, 70), False, 3), many + _geom((111, 95), True)])
    empty = (np.zeros(0, np.int64), np.zeros((0, 4), np.float32)) + _geom((50, 70), False)
    return BoxLists([_hand_item(rng, (111, 95), True, 2), empty, _hand_item(rng, (50, 70), False, 5)])


CASES = [(d, c) for d in ("cityscapes", "vistas") for c in ("n2", "n3")]


def probabilities(dataset, case):
    """P float32 [n, 37, 45, CT] of crf_ref.synthetic_inputs (read-only)."""
    return synthetic_inputs(dataset, len(box_lists(case)), HW)[0]


@functools.lru_cache(maxsize=None)
def case_cover(case):
    items = box_lists(case)
    cv = cover(items, HW)
    return cv, masks(items, cv, HW)


def hand_reject(case):
    """One rejected box per image that has boxes: its second box."""
    items = box_lists(case)
    rj = np.zeros(max(len(all_cids(items)), 1), dtype=np.int32)
    b0 = 0
    for it in items:
        if len(it[0]) > 1:
            rj[b0 + 1] = 1
        b0 += len(it[0])
    return rj


@functools.lru_cache(maxsize=None)
def reference(dataset, case, dtype=np.float64):
    """dict of the whole chain on the case in dtype: P', labels, conf, counts (tau = TAU), reject
    (MIN_FILL) and the final maps per output size. Cached, read-only."""
    items = box_lists(case)
    cv, mask = case_cover(case)
    Pc = constrain(probabilities(dataset, case), mask, dataset, dtype)
    labels, conf, counts = decide(Pc, items, cv, mask, dataset, TAU, dtype)
    rj = rejects(counts, all_cids(items), dataset, MIN_FILL)
    out = dict(constrained=Pc, labels=labels, conf=conf, counts=counts, reject=rj,
               final={hw: finalize(labels, cv, rj, hw, dataset) for hw in OUT_SIZES})
    for v in list(out.values()) + list(out["final"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
