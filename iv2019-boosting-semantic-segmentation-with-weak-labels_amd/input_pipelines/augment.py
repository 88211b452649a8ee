"""Training augmentation (the reference's preprocessing/augmentation_library.py: random_color
:359-406, random_blur :408-466, random_flipping :298-321, random_scaling :21-296), the call block
its train pipelines hold between the resize and from_0_1_to_m1_1 (input_cityscapes.py:106-118):
colour -> blur -> flip -> scaling.

The random numbers are drawn here, on the host, into one record per image (``AUG_DTYPE``, the
layout of ``seg_aug_params`` in include/seg_hip.h); the device kernels (csrc/augment.hip) are
pure functions of (raw input, record): ``augment_images`` / ``augment_labels`` replace
``prepare_images[_crop]`` / ``prepare_labels`` and give bitwise their output for an all-off
record.

Distributions (the reference's): one colour selector per batch from integers(0, 8): 0..3 is the
op order of every image, 4..7 means no colour; per image brightness delta ~ U(-32/255, 32/255),
saturation and contrast factors ~ U(0.7, 1.3), hue delta ~ U(-0.1, 0.1); flip per image with
p = 1/2 (an enabled flip stage sends every image through uint8, flipped or not); scaling up or
down per image with p = 1/2, factor f ~ U(1/high, 1/low) of ``scale_poi = [low, high]``, sizes
floor(f * H) x floor(f * W), up-scaling crop offsets uniform in [0, H - sh] x [0, W - sw];
``scale_poi == [1.0, 1.0]`` turns scaling off.

Blur (from a generator of its own, so that switching it on moves no other draw): one selector
per batch from integers(0, 4): 0 is the median for every image, 1 the bilateral filter, 2 and 3
no blur; per image the kernel size k = 2 * (integers(0, m) + 1) + 1 with
m = int(rint(1.4 * (res + 1))) and res = H * W / 1e6 (k in {3, 5} at 512 x 1024, {3, 5, 7, 9} at
1024 x 2048); the bilateral sigma (colour and space, on values in [0, 1] as the reference has
it) is rint(25 * (res + 1)). The kernels take odd k from 3 to 9, which is every network size
with 1.4 * (res + 1) <= 4.5; a larger one is a ValueError here.
"""
from __future__ import annotations

import numpy as np

# the record's last three words: 0 none / 1 median / 2 bilateral, the odd window size 3..9, the
# bilateral sigma (colour and space); all zero = no blur
BLUR_DTYPE = np.dtype([('mode', np.int32), ('ksize', np.int32), ('sigma', np.float32)])
AUG_DTYPE = np.dtype([
    ('color_order', np.int32), ('brightness_delta', np.float32),
    ('saturation_factor', np.float32), ('hue_delta', np.float32),
    ('contrast_factor', np.float32), ('quantize', np.int32), ('flip', np.int32),
    ('scale_mode', np.int32), ('sh', np.int32), ('sw', np.int32), ('oy', np.int32),
    ('ox', np.int32), ('void_cid', np.int32), ('blur', BLUR_DTYPE)])
AUG_PARAMS_BYTES = 64   # SEG_AUG_PARAMS_BYTES
assert AUG_DTYPE.itemsize == AUG_PARAMS_BYTES

MAX_DELTA_BRIGHTNESS = 32.0 / 255.0
FACTOR_RANGE = (0.7, 1.3)       # saturation, contrast
MAX_DELTA_HUE = 0.1
BLUR_NONE, BLUR_MEDIAN, BLUR_BILATERAL = 0, 1, 2
BLUR_MAX_KSIZE = 9              # the kernels' largest window


def off_params(n, H, W, void_cid=0):
    """n records with every stage off (the output of the prepare_* functions)."""
    p = np.zeros(n, AUG_DTYPE)
    p['color_order'] = -1
    p['saturation_factor'] = p['contrast_factor'] = 1.0
    p['sh'], p['sw'] = H, W
    p['void_cid'] = void_cid
    return p


def blur_draw_range(H, W):
    """(m, sigma) of random_blur at the network size H x W: k = 2 * (integers(0, m) + 1) + 1."""
    res = H * W / 1e6
    m = int(np.rint(1.4 * (res + 1)))
    if 2 * m + 1 > BLUR_MAX_KSIZE:
        raise ValueError(f'augment blur: a {H}x{W} network size draws kernel sizes up to '
                         f'{2 * m + 1}, the blur kernels take 3..{BLUR_MAX_KSIZE} '
                         f'(H * W <= 2214285)')
    return m, float(np.rint(25 * (res + 1)))


def draw_params(rng, n, H, W, *, color=False, flip=False, scale_poi=None, void_cid=0,
                blur=False, blur_rng=None, blur_mode=None, blur_ksize=None):
    """One batch's records from ``rng`` (numpy Generator); see the module docstring. The blur
    draws come from ``blur_rng`` alone; ``blur_mode`` / ``blur_ksize`` (scalars or [n]) replace
    what was drawn (the draws are still made)."""
    p = off_params(n, H, W, void_cid)
    if blur:
        if blur_rng is None:
            raise ValueError('blur=True needs blur_rng, a generator of its own')
        m, sigma = blur_draw_range(H, W)
        sel = int(blur_rng.integers(0, 4))
        ks = 2 * (blur_rng.integers(0, m, n) + 1) + 1
        mode = np.full(n, {0: BLUR_MEDIAN, 1: BLUR_BILATERAL}.get(sel, BLUR_NONE), np.int32)
        if blur_mode is not None:
            mode[:] = blur_mode
        if blur_ksize is not None:
            ks[:] = blur_ksize
        p['blur']['mode'] = mode
        p['blur']['ksize'] = np.where(mode != BLUR_NONE, ks, 0)
        p['blur']['sigma'] = np.where(mode == BLUR_BILATERAL, sigma, 0.0)
    if color:
        sel = int(rng.integers(0, 8))
        p['color_order'] = sel if sel < 4 else -1
        p['brightness_delta'] = rng.uniform(-MAX_DELTA_BRIGHTNESS, MAX_DELTA_BRIGHTNESS, n)
        p['saturation_factor'] = rng.uniform(*FACTOR_RANGE, n)
        p['hue_delta'] = rng.uniform(-MAX_DELTA_HUE, MAX_DELTA_HUE, n)
        p['contrast_factor'] = rng.uniform(*FACTOR_RANGE, n)
    if flip:
        p['quantize'] = 1
        p['flip'] = rng.random(n) < 0.5
    if scale_poi is not None and tuple(float(v) for v in scale_poi) != (1.0, 1.0):
        low, high = (float(v) for v in scale_poi)
        if not 0.0 < low <= high:
            raise ValueError(f'scale_poi must be 0 < low <= high, got {scale_poi}')
        for i in range(n):
            up = rng.random() < 0.5
            f = rng.uniform(1.0 / high, 1.0 / low)
            sh = min(max(int(np.floor(f * H)), 1), H)
            sw = min(max(int(np.floor(f * W)), 1), W)
            p['scale_mode'][i], p['sh'][i], p['sw'][i] = (1 if up else 2), sh, sw
            if up:
                p['oy'][i] = rng.integers(0, H - sh + 1)
                p['ox'][i] = rng.integers(0, W - sw + 1)
    return p


def _table(params, n, device):
    """(host array kept alive by the caller, device copy) of n records."""
    import torch
    host = np.ascontiguousarray(params, dtype=AUG_DTYPE)
    if host.shape != (n,):
        raise ValueError(f'{n} images need {n} parameter records, got shape {host.shape}')
    dev = torch.from_numpy(host.view(np.uint8).reshape(n, AUG_PARAMS_BYTES).copy()).to(device)
    return host, dev


def augment_images(raw, params, H: int, W: int, resized=None, offset=(0, 0), stream=None):
    """raw: device uint8 [n, h, w, 3] -> resize to `resized` (default H x W), window at `offset`
    (as prepare_images_crop) -> colour, blur, flip stage, scaling per ``params`` (AUG_DTYPE [n])
    -> fp32 [n, H, W, 3] centred."""
    import ctypes
    import torch
    from seg_hip import LIB, _ptr, _stream, check
    assert raw.dtype == torch.uint8 and raw.dim() == 4 and raw.shape[-1] == 3 and raw.is_cuda
    raw = raw.contiguous()
    n = raw.shape[0]
    host, dev = _table(params, n, raw.device)
    rs = (H, W) if resized is None else (int(resized[0]), int(resized[1]))
    need = ctypes.c_int64(0)
    check(LIB.seg_augment_workspace(n, H, W, ctypes.byref(need)))
    ws = torch.empty(max(int(need.value), 16), dtype=torch.uint8, device=raw.device)
    out = torch.empty((n, H, W, 3), dtype=torch.float32, device=raw.device)
    check(LIB.seg_augment_images(_ptr(raw), n, raw.shape[1], raw.shape[2], rs[0], rs[1],
                                 int(offset[0]), int(offset[1]), H, W, host.ctypes.data,
                                 _ptr(dev), _ptr(out), _ptr(ws), ws.numel(), _stream(stream)))
    return out


def augment_labels(raw, params, H: int, W: int, lids2cids, stream=None):
    """raw: device uint8 label ids [n, h, w] -> int32 [n, H, W] training cids with the flip and
    the scaling of ``params`` (nearest resize; the down-scale pad is ``void_cid``)."""
    import ctypes
    import torch
    from seg_hip import LIB, _ptr, _stream, check
    assert raw.dtype == torch.uint8 and raw.dim() == 3 and raw.is_cuda
    raw = raw.contiguous()
    n = raw.shape[0]
    host, dev = _table(params, n, raw.device)
    out = torch.empty((n, H, W), dtype=torch.int32, device=raw.device)
    m = (ctypes.c_int32 * len(lids2cids))(*[int(v) for v in lids2cids])
    check(LIB.seg_augment_labels(_ptr(raw), n, raw.shape[1], raw.shape[2], H, W, m,
                                 len(lids2cids), host.ctypes.data, _ptr(dev), _ptr(out),
                                 _stream(stream)))
    return out
