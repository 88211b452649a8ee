"""Numpy restatement of the blur stage of the training augmentation (random_blur,
augmentation_library.py:408-466; csrc/augment.hip pass 2b), with the arithmetic dtype as an
argument like tests/aug_ref.py: float32 restates the kernels operation by operation (the same
order of the tap sums, no FMA), float64 is the same function in higher precision.

  median    : q = trunc(x * 255) as uint8, per-channel median of the k x k window with replicated
              borders (k * k is odd: the median is an element), q_med / 255
  bilateral : taps (i, j) with i^2 + j^2 <= (k // 2)^2, reflect-101 borders, weight
              exp(coef * (i^2 + j^2)) * exp(coef * (|dR| + |dG| + |dB|)^2), coef = -0.5 / sigma^2,
              weighted mean per channel; taps are summed row by row

``augment_image_blur`` is aug_ref.augment_image with the blur between the colour stage and the
flip stage. The chain cases of the GPU test and of profiles/augment_blur_margins.txt
(tools/aug_blur_margins.py) are defined here so that both use the same inputs. A helper module,
not a test file."""
import numpy as np

import aug_ref

VOID = 19


def median(x, k, dtype=np.float32):
    """x [H, W, 3] in [0, 1] -> cv2.medianBlur of its 8-bit image, back in [0, 1]."""
    H, W, _ = x.shape
    r = k // 2
    q = np.trunc(x * dtype(255)).astype(np.uint8)
    p = np.pad(q, ((r, r), (r, r), (0, 0)), mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(p, (k, k), axis=(0, 1))   # [H, W, 3, k, k]
    med = np.sort(win.reshape(H, W, 3, k * k), axis=-1)[..., (k * k) // 2]
    return (med.astype(dtype) / dtype(255)).astype(dtype)


def bilateral(x, k, sigma, dtype=np.float32):
    """x [H, W, 3] -> the closed-form bilateral filter with sigmaColor = sigmaSpace = sigma."""
    H, W, _ = x.shape
    r = k // 2
    x = x.astype(dtype)
    p = np.pad(x, ((r, r), (r, r), (0, 0)), mode="reflect")
    coef = dtype(-0.5) / (dtype(sigma) * dtype(sigma))
    acc = np.zeros((H, W, 3), dtype)
    tot = np.zeros((H, W), dtype)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy * dy + dx * dx > r * r:
                continue
            t = p[r + dy:r + dy + H, r + dx:r + dx + W]
            a = np.abs(t - x)
            d = (a[..., 0] + a[..., 1]) + a[..., 2]
            w = (np.exp(dtype(dy * dy + dx * dx) * coef) * np.exp((d * d) * coef)).astype(dtype)
            acc = (acc + t * w[..., None]).astype(dtype)
            tot = (tot + w).astype(dtype)
    return (acc / tot[..., None]).astype(dtype)


def blur(x, rec, dtype=np.float32):
    mode = int(rec["blur"]["mode"])
    if mode == 1:
        return median(x, int(rec["blur"]["ksize"]), dtype)
    if mode == 2:
        return bilateral(x, int(rec["blur"]["ksize"]), rec["blur"]["sigma"], dtype)
    return x


def augment_image_blur(raw, rec, H, W, resized=None, offset=(0, 0), dtype=np.float32):
    """One image through resize -> colour -> blur -> flip stage -> scaling -> centring. Returns
    (out [H, W, 3], fill [H, W] bool: the down-scale pad), as aug_ref.augment_image."""
    x = aug_ref.colour(aug_ref.resized01(raw, H, W, resized, offset, dtype), rec, dtype)
    x = blur(x, rec, dtype)
    if rec["quantize"]:
        x = aug_ref.quant(x, dtype)
    if rec["flip"]:
        x = x[:, ::-1]
    fill = np.zeros((H, W), bool)
    sh, sw = int(rec["sh"]), int(rec["sw"])
    if rec["scale_mode"] == 1:
        oy, ox = int(rec["oy"]), int(rec["ox"])
        x = aug_ref.bilinear(aug_ref.quant(x[oy:oy + sh, ox:ox + sw], dtype), aug_ref.tables(sh, H),
                             aug_ref.tables(sw, W), dtype)
    elif rec["scale_mode"] == 2:
        d = aug_ref.bilinear(x, aug_ref.tables(H, sh), aug_ref.tables(W, sw), dtype)
        top, left = (H - sh) // 2, (W - sw) // 2
        x = np.full((H, W, 3), d.mean(dtype=dtype), dtype)
        x[top:top + sh, left:left + sw] = d
        fill[:] = True
        fill[top:top + sh, left:left + sw] = False
    return ((x - dtype(0.5)) / dtype(0.5)).astype(dtype), fill


def augment_images_blur(raw, params, H, W, resized=None, offset=(0, 0), dtype=np.float32):
    r = [augment_image_blur(raw[i], params[i], H, W, resized, offset, dtype) for i in range(len(raw))]
    return np.stack([a for a, _ in r]), np.stack([f for _, f in r])


# ---- the chain cases: colour + blur + flip + scaling up (image 0) and down (image 1) ----------
CHAIN_SHAPES = [(37, 53), (70, 131)]
CHAIN_MODES = {"median": 1, "bilateral": 2}
# (mode, H) -> seed of the inputs and of the draws: those for which the float32 chain differs
# from the float64 one by more than the colour bound on a non-zero but small share of the
# elements (profiles/augment_blur_margins.txt lists the shares)
CHAIN_SEEDS = {("median", 37): 3, ("median", 70): 7, ("bilateral", 37): 1, ("bilateral", 70): 3}
CHAIN_KSIZE = {37: [5, 3], 70: [9, 7]}


def chain_case(mode, H, W, seed=None):
    """(raw uint8 [2, h, w, 3], records [2]) of one chain case."""
    from input_pipelines.augment import draw_params
    seed = CHAIN_SEEDS[(mode, H)] if seed is None else seed
    rng = np.random.default_rng([seed, H, CHAIN_MODES[mode]])
    raw = rng.integers(0, 256, (2, H + 8, W + 17, 3), dtype=np.uint8)
    p = draw_params(rng, 2, H, W, color=True, flip=True, scale_poi=[1.0, 2.0], void_cid=VOID,
                    blur=True, blur_rng=np.random.default_rng(seed), blur_mode=CHAIN_MODES[mode],
                    blur_ksize=CHAIN_KSIZE[H])
    p["color_order"] = [seed % 4, (seed + 1) % 4]
    p["flip"] = [1, 0]
    p["scale_mode"] = [1, 2]
    p["oy"], p["ox"] = [(H - p["sh"][0]) // 2, 0], [(W - p["sw"][0]) // 3, 0]
    return raw, p


def colour_bound(raw, p, H, W):
    """The colour-only bound of tests/test_gpu_augment.py: 4 x the largest error of the float32
    restatement against float64 with every later stage off, floor 2^-22 (centred units)."""
    q = p.copy()
    q["quantize"] = q["flip"] = q["scale_mode"] = q["blur"]["mode"] = 0
    r32, _ = aug_ref.augment_images(raw, q, H, W, dtype=np.float32)
    r64, _ = aug_ref.augment_images(raw, q, H, W, dtype=np.float64)
    return max(4.0 * float(np.abs(r32 - r64).max()), 2.0 ** -22)


def chain_reference(mode, H, W, seed=None):
    """(raw, records, bound, float64 chain, share of the float32 chain's elements further than
    bound from the float64 one)."""
    raw, p = chain_case(mode, H, W, seed)
    bound = colour_bound(raw, p, H, W)
    r32, _ = augment_images_blur(raw, p, H, W, dtype=np.float32)
    r64, _ = augment_images_blur(raw, p, H, W, dtype=np.float64)
    return raw, p, bound, r64, float((np.abs(r32 - r64) > bound).mean())
