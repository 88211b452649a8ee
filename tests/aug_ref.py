"""Numpy restatement of the training augmentation (input_pipelines/augment.py, csrc/augment.hip),
written from the formulas of TF 1.12 and the reference's preprocessing/augmentation_library.py,
with the arithmetic dtype as an argument: float32 restates the kernels operation by operation
(no FMA, the same lerp form), float64 is the same function in higher precision. The resize
geometry (source indices and lerp weights from the float32 legacy scaler, scale = in / out) is
part of the specification and is float32 for both.

Per image: resize -> colour -> flip stage -> scaling -> (x - 0.5) / 0.5. A helper module, not a
test file."""
import numpy as np

# distort_color's op orders
ORDERS = {0: "BSHC", 1: "SBCH", 2: "CHBS", 3: "HSCB"}


def tables(n_in, n_out):
    """Legacy bilinear scaler: lo = (int)(o * scale), hi = min(lo + 1, in - 1), lerp."""
    scale = np.float32(np.float32(n_in) / np.float32(n_out))
    fin = (np.arange(n_out, dtype=np.float32) * scale).astype(np.float32)
    lo = fin.astype(np.int64)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, (fin - lo.astype(np.float32)).astype(np.float32)


def nearest(n_in, n_out):
    scale = np.float32(np.float32(n_in) / np.float32(n_out))
    f = (np.arange(n_out, dtype=np.float32) * scale).astype(np.float32)
    return np.minimum(np.floor(f).astype(np.int64), n_in - 1)


def bilinear(x, ytab, xtab, dtype):
    """x [h, w, 3] -> [len(ytab), len(xtab), 3]: top = tl + (tr - tl) * xl, ..."""
    yl, yh, ylr = ytab
    xl, xh, xlr = xtab
    xlr = xlr.astype(dtype)[None, :, None]
    ylr = ylr.astype(dtype)[:, None, None]
    tl, tr = x[yl][:, xl], x[yl][:, xh]
    bl, br = x[yh][:, xl], x[yh][:, xh]
    top = tl + (tr - tl) * xlr
    bot = bl + (br - bl) * xlr
    return (top + (bot - top) * ylr).astype(dtype)


def quant(x, dtype):
    """convert_image_dtype to uint8 and back: trunc(x * 255.5), q * (1 / 255)."""
    q = np.trunc(x * dtype(255.5))
    return (q.astype(dtype) * dtype(np.float32(1.0 / 255.0))).astype(dtype)


def rgb_to_hsv(c, dtype):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(r, np.maximum(g, b))
    rng = v - np.minimum(r, np.minimum(g, b))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, rng / v, dtype(0))
        n = dtype(1) / (dtype(6) * rng)
        h = np.where(r == v, n * (g - b),
                     np.where(g == v, n * (b - r) + dtype(2) / dtype(6),
                              n * (r - g) + dtype(4) / dtype(6)))
    h = np.where(rng == 0, dtype(0), h)
    h = np.where(h < 0, h + dtype(1), h)
    return h.astype(dtype), s.astype(dtype), v.astype(dtype)


def hsv_to_rgb(h, s, v, dtype):
    dh = dtype(6) * h
    d = np.stack([np.clip(np.abs(dh - dtype(3)) - dtype(1), 0, 1),
                  np.clip(dtype(2) - np.abs(dh - dtype(2)), 0, 1),
                  np.clip(dtype(2) - np.abs(dh - dtype(4)), 0, 1)], -1).astype(dtype)
    return (((d - dtype(1)) * s[..., None] + dtype(1)) * v[..., None]).astype(dtype)


def colour(x, rec, dtype):
    """x [H, W, 3] in [0, 1] -> the four ops in rec's order, then clip(0, 1)."""
    order = int(rec["color_order"])
    if order < 0:
        return x
    for op in ORDERS[order]:
        if op == "B":
            x = x + dtype(rec["brightness_delta"])
        elif op == "C":
            m = x.mean(axis=(0, 1), dtype=dtype)
            x = (x - m) * dtype(rec["contrast_factor"]) + m
        else:
            h, s, v = rgb_to_hsv(x, dtype)
            if op == "S":
                s = np.clip(s * dtype(rec["saturation_factor"]), 0, 1).astype(dtype)
            else:
                h = h + dtype(rec["hue_delta"])
                h = h - np.floor(h)
            x = hsv_to_rgb(h, s, v, dtype)
        x = x.astype(dtype)
    return np.clip(x, 0, 1).astype(dtype)


def resized01(raw, H, W, resized=None, offset=(0, 0), dtype=np.float32):
    """raw uint8 [h, w, 3] -> the [0, 1] image of prepare_images[_crop] before its centring."""
    x = raw.astype(dtype) * dtype(np.float32(1.0 / 255.0))
    rh, rw = resized if resized is not None else (H, W)
    cy, cx = offset
    yt = tuple(t[cy:cy + H] for t in tables(raw.shape[0], rh))
    xt = tuple(t[cx:cx + W] for t in tables(raw.shape[1], rw))
    return bilinear(x, yt, xt, dtype)


def augment_image(raw, rec, H, W, resized=None, offset=(0, 0), dtype=np.float32):
    """One image. Returns (out [H, W, 3] centred, fill [H, W] bool: the down-scale pad region,
    whose value is the mean of the down-scaled image)."""
    x = colour(resized01(raw, H, W, resized, offset, dtype), rec, dtype)
    if rec["quantize"]:
        x = quant(x, dtype)
    if rec["flip"]:
        x = x[:, ::-1]
    fill = np.zeros((H, W), bool)
    sh, sw = int(rec["sh"]), int(rec["sw"])
    if rec["scale_mode"] == 1:
        oy, ox = int(rec["oy"]), int(rec["ox"])
        x = bilinear(quant(x[oy:oy + sh, ox:ox + sw], dtype), tables(sh, H), tables(sw, W), dtype)
    elif rec["scale_mode"] == 2:
        d = bilinear(x, tables(H, sh), tables(W, sw), dtype)
        top, left = (H - sh) // 2, (W - sw) // 2
        x = np.full((H, W, 3), d.mean(dtype=dtype), dtype)
        x[top:top + sh, left:left + sw] = d
        fill[:] = True
        fill[top:top + sh, left:left + sw] = False
    return ((x - dtype(0.5)) / dtype(0.5)).astype(dtype), fill


def augment_label(raw, rec, H, W, lids2cids):
    """raw uint8 ids [h, w] -> int32 [H, W]: lids2cids (-1 -> max + 1), nearest resize, flip,
    the scaling's nearest resize / void_cid pad."""
    m = np.asarray(lids2cids, np.int64)
    m = np.where(m == -1, m.max() + 1, m)
    lab = m[raw.astype(np.int64)][nearest(raw.shape[0], H)][:, nearest(raw.shape[1], W)]
    if rec["flip"]:
        lab = lab[:, ::-1]
    sh, sw = int(rec["sh"]), int(rec["sw"])
    if rec["scale_mode"] == 1:
        oy, ox = int(rec["oy"]), int(rec["ox"])
        lab = lab[oy:oy + sh, ox:ox + sw][nearest(sh, H)][:, nearest(sw, W)]
    elif rec["scale_mode"] == 2:
        d = lab[nearest(H, sh)][:, nearest(W, sw)]
        top, left = (H - sh) // 2, (W - sw) // 2
        lab = np.full((H, W), int(rec["void_cid"]), np.int64)
        lab[top:top + sh, left:left + sw] = d
    return lab.astype(np.int32)


def augment_images(raw, params, H, W, resized=None, offset=(0, 0), dtype=np.float32):
    """Batch: raw [n, h, w, 3] -> (out [n, H, W, 3], fill [n, H, W])."""
    r = [augment_image(raw[i], params[i], H, W, resized, offset, dtype) for i in range(len(raw))]
    return np.stack([a for a, _ in r]), np.stack([f for _, f in r])


def augment_labels(raw, params, H, W, lids2cids):
    return np.stack([augment_label(raw[i], params[i], H, W, lids2cids) for i in range(len(raw))])
