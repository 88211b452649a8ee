"""Numpy reference of the boundary-band confusion (include/seg_hip.h at seg_boundary_distance),
written from the definitions, and the label maps the CPU and GPU tests share.

* counted label: 0 <= l < nc and l != ignore (ignore = -1: none);
* boundary pixel: a counted label with a 4-neighbour in the same image that carries another
  counted label;
* d2: the least dy^2 + dx^2 to a boundary pixel of the same image, capped at cap_width^2 + 1;
* band w: d2 <= w^2; cm[k][l][d] counts the pixels of band w_k with label l and decision d, both
  in [0, nc).

``d2_brute`` walks the disc of offsets (the definition); ``d2_separable`` is the row-then-column
form the kernels use. Everything is integer arithmetic: every comparison is exact.
"""
import numpy as np

MAX_WIDTH = 64


def counted(lab, nc, ignore):
    lab = np.asarray(lab)
    return (lab >= 0) & (lab < nc) & (lab != ignore)


def boundary(lab, nc, ignore):
    """bool [n, H, W] (or [H, W]): the boundary pixels of every image."""
    lab = np.asarray(lab)
    if lab.ndim == 2:
        return boundary(lab[None], nc, ignore)[0]
    ok = counted(lab, nc, ignore)
    out = np.zeros(lab.shape, dtype=bool)
    # vertical pairs (y, y + 1), then horizontal pairs (x, x + 1): both pixels of a pair
    pair = ok[:, :-1] & ok[:, 1:] & (lab[:, :-1] != lab[:, 1:])
    out[:, :-1] |= pair
    out[:, 1:] |= pair
    pair = ok[:, :, :-1] & ok[:, :, 1:] & (lab[:, :, :-1] != lab[:, :, 1:])
    out[:, :, :-1] |= pair
    out[:, :, 1:] |= pair
    return out


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that is inside the image, ``fill`` elsewhere ([n, H, W])."""
    n, H, W = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        b[:, yd, xd] = a[:, ys, xs]
    return b


def d2_brute(lab, nc, ignore, cap_width=MAX_WIDTH):
    """int32 [n, H, W]: min over the offsets of the disc dy^2 + dx^2 <= cap_width^2 that lead to a
    boundary pixel of the same image, cap_width^2 + 1 where there is none."""
    lab = np.asarray(lab)
    if lab.ndim == 2:
        return d2_brute(lab[None], nc, ignore, cap_width)[0]
    b = boundary(lab, nc, ignore)
    w = int(cap_width)
    out = np.full(lab.shape, w * w + 1, dtype=np.int32)
    if not b.any():
        return out
    for dy in range(-w, w + 1):
        for dx in range(-w, w + 1):
            d = dy * dy + dx * dx
            if d > w * w:
                continue
            hit = _shifted(b, dy, dx, False)
            out = np.where(hit & (d < out), np.int32(d), out)
    return out


def row_distance(lab, nc, ignore, cap_width=MAX_WIDTH):
    """int32 [n, H, W]: min(|dx| to the nearest boundary pixel of the same row, cap_width + 1)."""
    b = boundary(lab, nc, ignore)
    w = int(cap_width)
    g = np.full(b.shape, w + 1, dtype=np.int32)
    for dx in range(-w, w + 1):
        g = np.where(_shifted(b, 0, dx, False) & (abs(dx) < g), np.int32(abs(dx)), g)
    return g


def d2_separable(lab, nc, ignore, cap_width=MAX_WIDTH):
    """The two-pass form: g per row, then min over |dy| <= cap_width of dy^2 + g(y + dy, x)^2; rows
    outside the image contribute nothing."""
    lab = np.asarray(lab)
    if lab.ndim == 2:
        return d2_separable(lab[None], nc, ignore, cap_width)[0]
    w = int(cap_width)
    g = row_distance(lab, nc, ignore, w)
    out = np.full(lab.shape, w * w + 1, dtype=np.int32)
    for dy in range(-w, w + 1):
        gs = _shifted(g, dy, 0, w + 1)
        out = np.minimum(out, dy * dy + gs * gs)
    return np.minimum(out, w * w + 1).astype(np.int32)


def band_masks(lab, nc, ignore, widths):
    """bool [K, n, H, W]: the band of every width, from the brute-force distances."""
    d2 = d2_brute(lab, nc, ignore, max(widths))
    return np.stack([d2 <= w * w for w in widths])


def confusion(lab, dec, nc, mask=None):
    """seg_confusion's rule: int64 [nc, nc] over the pixels with both values in [0, nc)."""
    lab, dec = np.asarray(lab), np.asarray(dec)
    ok = (lab >= 0) & (lab < nc) & (dec >= 0) & (dec < nc)
    if mask is not None:
        ok &= mask
    return np.bincount(lab[ok].astype(np.int64) * nc + dec[ok], minlength=nc * nc).reshape(nc, nc)


def band_confusion(lab, dec, nc, ignore, widths):
    """int64 [K, nc, nc]."""
    masks = band_masks(lab, nc, ignore, widths)
    return np.stack([confusion(lab, dec, nc, m) for m in masks])


# ---- the cases ---------------------------------------------------------------------------------

def blocky_case(nc=20, seed=7):
    """int32 [3, 37, 45]: seeded patches of 8 x 8 (ragged against every tile, ~10 % of the patches
    are the void class nc - 1); image 1 is a single class; image 0 gets a boundary on its last row
    and image 2 one on its first row, so a distance that leaked into the neighbouring image of the
    batch would show in image 1, which has no boundary of its own."""
    from input_pipelines.synthetic import pixel_labels
    lab = pixel_labels(np.random.default_rng(seed), 3, 37, 45, n_classes=nc, patch=8)
    lab[1] = 4
    lab[0, 36, :] = 2
    lab[0, 36, 20:30] = 3
    lab[2, 0, :] = 5
    lab[2, 0, 10:17] = 6
    return lab


def dots_case(H, W):
    """int32 [1, H, W] of class 0 with single pixels of class 3 at the four corners and the
    centre: every band is a union of discs, clipped by the image at the corners."""
    lab = np.zeros((1, H, W), dtype=np.int32)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        lab[0, y, x] = 3
    return lab


def out_of_range_case(nc=20, seed=11):
    """The blocky case with seeded rectangles of -1 and of nc: neither is a boundary, neither makes
    a neighbour one."""
    lab = blocky_case(nc, seed)
    lab[0, 5:15, 10:30] = -1
    lab[2, 20:30, 0:12] = nc
    lab[0, 30, 3] = -1
    lab[2, 3, 40] = nc + 7
    return lab


def decisions_for(lab, nc, seed=3):
    """Seeded decisions: the label where it is a class, otherwise random; 30 % replaced by a random
    class and about 2 % out of range (-1 or nc)."""
    rng = np.random.default_rng(seed)
    dec = np.where((lab >= 0) & (lab < nc), lab, 0).astype(np.int32)
    r = rng.random(lab.shape)
    dec = np.where(r < 0.3, rng.integers(0, nc, lab.shape), dec)
    dec = np.where(r > 0.98, np.where(rng.random(lab.shape) < 0.5, -1, nc), dec)
    return np.ascontiguousarray(dec.astype(np.int32))


CASES = {
    "blocky": lambda nc: blocky_case(nc),
    "tall_dots": lambda nc: dots_case(200, 33),
    "wide_dots": lambda nc: dots_case(33, 300),
    "out_of_range": lambda nc: out_of_range_case(nc),
    # a width that is a multiple of 4: the kernels move four row distances at a time
    "aligned": lambda nc: np.ascontiguousarray(blocky_case(nc)[:, :, :44]),
}
