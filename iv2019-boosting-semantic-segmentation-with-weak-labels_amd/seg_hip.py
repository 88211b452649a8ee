"""ctypes binding of ``libseg_hip.so`` (C ABI in ``include/seg_hip.h``).

This is the only way the host code reaches the GPU path. There is no fallback: if the
library is missing or does not load, importing this module raises ``RuntimeError``.
PyTorch is used only for device memory (flat parameter buffers, inputs) and the stream
handle; every kernel of the training step is in the HIP library.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEG_HIP_LIB: development override (kernel A/B variants built by `make VARIANT=...`)
LIB_PATH = os.environ.get("SEG_HIP_LIB") or os.path.join(_HERE, "libseg_hip.so")

EXPORTED_SYMBOLS = [
    "seg_create", "seg_destroy", "seg_last_error", "seg_sizes", "seg_bind_buffers",
    "seg_param_count", "seg_param_info", "seg_param_shape", "seg_params_updated", "seg_forward", "seg_loss",
    "seg_backward", "seg_apply_update", "seg_outputs", "seg_confusion", "seg_debug_tensor",
    "seg_profile", "seg_profile_dump",
    "seg_profile_read", "seg_op_conv_fwd", "seg_op_conv_stat_rows", "seg_op_conv_dgrad",
    "seg_op_conv_dgrad_res",
    "seg_op_conv_wgrad", "seg_op_conv_wgrad_cfg", "seg_op_conv_dgrad_fused",
    "seg_op_conv_plan", "seg_op_conv_wgrad_plan", "seg_op_bn_rowblocks", "seg_op_bn_stats_finalize",
    "seg_op_bn_apply", "seg_op_bn_backward", "seg_op_bn_backward_dual", "seg_bbox_labels", "seg_tag_labels",
    "seg_grad_buckets", "seg_stream_wait_bucket", "seg_set_loss_scale", "seg_found_inf",
    "seg_set_bn_sync", "seg_set_bn_inference", "seg_predict", "seg_full_predictions",
    "seg_set_nesterov", "seg_set_defer_stem", "seg_flush_grads", "seg_set_premask", "seg_set_lbf",
    "seg_counter",
    "seg_crc32c", "seg_prepare_images", "seg_prepare_labels", "seg_prepare_images_crop",
    "seg_bbox_labels_flip", "seg_augment_workspace", "seg_augment_images", "seg_augment_labels", "seg_augment_profile",
    "seg_augment_profile_blur", "seg_set_bootstrap", "seg_op_bootstrap_threshold",
    "seg_resize_images", "seg_tta_decisions",
    "seg_window_images", "seg_window_decisions",
    "seg_crf_workspace", "seg_crf_decisions",
    "seg_box_kinds", "seg_box_constrain", "seg_box_decisions", "seg_box_finalize",
    "seg_boundary_distance", "seg_band_confusion_workspace", "seg_band_confusion",
]

# int (*seg_allreduce_fn)(void* user, float* buf, int64_t n, void* stream)
SEG_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                    ctypes.c_void_p)

PYRAMID = {"none": 0, "psp": 1, "aspp": 2}
DTYPE = {"fp32": 0, "bf16": 1, "fp16": 2}
DATASET = {"cityscapes": 0, "vistas": 1}
# dataset -> (head widths l1 | l2 vehicle | l2 human, training classes)
HEAD_LAYOUT = {"cityscapes": ((14, 7, 3), 20), "vistas": ((53, 12, 5), 66)}
PARAM_KIND = {0: "weights", 1: "gamma", 2: "beta", 3: "moving_mean", 4: "moving_variance",
              5: "biases"}
UPSAMPLING = {"bilinear": 0, "hybrid": 1}
NORM = {"batch": 0, "group": 1}


class SegCfg(ctypes.Structure):
    _fields_ = [
        ("depth", ctypes.c_int), ("pyramid", ctypes.c_int), ("height", ctypes.c_int),
        ("width", ctypes.c_int), ("nb_pp", ctypes.c_int), ("nb_pb", ctypes.c_int),
        ("nb_pi", ctypes.c_int), ("dtype", ctypes.c_int), ("dataset", ctypes.c_int),
        ("output_stride", ctypes.c_int), ("feature_dims", ctypes.c_int),
        ("bn_decay", ctypes.c_float), ("train_bn", ctypes.c_int),
        ("weight_decay", ctypes.c_float), ("fov_k", ctypes.c_int), ("fov_rate", ctypes.c_int),
        ("upsampling", ctypes.c_int), ("norm", ctypes.c_int), ("groups", ctypes.c_int),
    ]


_VP, _FP, _INT = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int


class BnApplyArgs(ctypes.Structure):
    """seg_bn_apply_args (include/seg_hip.h); pointers are device addresses (tensor.data_ptr())"""
    _fields_ = [
        ("y", _VP), ("ldy", _INT), ("M", ctypes.c_int64), ("C", _INT),
        ("mean", _FP), ("scale", _FP), ("beta", _FP), ("relu", _INT),
        ("res", _VP), ("ldres", _INT), ("rs", _INT),
        ("Ho", _INT), ("Wo", _INT), ("Hr", _INT), ("Wr", _INT),
        ("y2", _VP), ("ldy2", _INT), ("mean2", _FP), ("scale2", _FP), ("beta2", _FP),
        ("out", _VP), ("ldo", _INT), ("mask", _VP),
    ]


class BnBwdArgs(ctypes.Structure):
    """seg_bn_bwd_args (include/seg_hip.h)"""
    _fields_ = [
        ("dz", _VP), ("lddz", _INT), ("z", _VP), ("ldz", _INT), ("mask", _VP),
        ("y", _VP), ("ldy", _INT), ("M", ctypes.c_int64), ("C", _INT),
        ("mean", _FP), ("invstd", _FP), ("scale", _FP), ("sdy", _FP), ("sdyx", _FP),
        ("dy", _VP), ("lddy", _INT), ("dyhat", _VP), ("lddyhat", _INT),
        ("dzscale", _FP), ("dshift", _FP), ("beta", _FP), ("cs_part", _FP),
        ("part", _FP), ("dgamma", _FP), ("dbeta", _FP),
    ]


TTA_MAX_ENTRIES = 16   # SEG_TTA_MAX_ENTRIES
WIN_MAX_ENTRIES = 64   # SEG_WIN_MAX_ENTRIES


class TtaEntry(ctypes.Structure):
    """seg_tta_entry (include/seg_hip.h); logits is a device address"""
    _fields_ = [("logits", _VP), ("h_low", _INT), ("w_low", _INT), ("ld", _INT), ("flip", _INT)]


class CrfParams(ctypes.Structure):
    """seg_crf_params (include/seg_hip.h)"""
    _fields_ = [("iterations", _INT), ("radius", _INT), ("dilation", _INT),
                ("w_appearance", ctypes.c_float), ("w_smoothness", ctypes.c_float),
                ("theta_alpha", ctypes.c_float), ("theta_beta", ctypes.c_float),
                ("theta_gamma", ctypes.c_float)]


def _load():
    # torch first: its HIP runtime must be the process's one before libseg_hip.so resolves
    # libamdhip64 (loading the library first left torch's later device init with
    # "no ROCm-capable device" on the box)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libseg_hip.so not found at {LIB_PATH}: build it with __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"failed to load {LIB_PATH}: {e}") from e
    vp, ip, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    sig = {
        "seg_create": (ip, [ip, ctypes.POINTER(SegCfg), ctypes.POINTER(vp)]),
        "seg_destroy": (ip, [vp]),
        "seg_last_error": (ctypes.c_char_p, [vp]),
        "seg_sizes": (ip, [vp] + [ctypes.POINTER(i64)] * 4),
        "seg_bind_buffers": (ip, [vp, vp, vp, vp, vp, vp]),
        "seg_param_count": (i64, [vp]),
        "seg_param_info": (ip, [vp, i64, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i64),
                                ctypes.POINTER(i64), ctypes.POINTER(ip)]),
        "seg_param_shape": (ip, [vp, i64, ctypes.POINTER(i64)]),
        "seg_params_updated": (ip, [vp, vp]),
        "seg_forward": (ip, [vp, vp, vp]),
        "seg_loss": (ip, [vp, vp, vp, vp, vp, vp]),
        "seg_backward": (ip, [vp, vp]),
        "seg_apply_update": (ip, [vp, f, f, f, f, vp]),
        "seg_outputs": (ip, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                             ctypes.POINTER(ip), ctypes.POINTER(ip), ctypes.POINTER(ip)]),
        "seg_confusion": (ip, [vp, vp, vp, i64, ip, vp, vp]),
        "seg_debug_tensor": (ip, [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(ip),
                                  ctypes.POINTER(ip), ctypes.POINTER(ip)]),
        "seg_profile": (ip, [vp, ip]),
        "seg_profile_dump": (ip, [vp, ctypes.c_char_p, ip]),
        "seg_profile_read": (ip, [vp, ip, ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64),
                                  ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ip]),
        "seg_op_conv_fwd": (ip, [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, ip, ip, vp, ip, vp, vp]),
        "seg_op_conv_stat_rows": (ip, [ip] * 12),
        "seg_op_conv_dgrad": (ip, [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, ip, ip, ip, ip, vp,
                                   ip, vp]),
        "seg_op_conv_dgrad_res": (ip, [ip, vp, ip, ip, ip, ip, ip, vp, ip, vp, ip, vp, ip, vp, vp]),
        "seg_op_conv_wgrad": (ip, [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, ip, ip, ip, ip, ip,
                                   vp, vp, i64, vp]),
        "seg_op_conv_wgrad_cfg": (ip, [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, ip, ip, ip, ip,
                                       ip, vp, vp, i64, ip, ip, ip, vp]),
        "seg_op_conv_plan": (ip, [ip, ip, ctypes.POINTER(ctypes.c_int), ip, ip, ctypes.c_char_p, ip]),
        "seg_op_conv_wgrad_plan": (ip, [ip, ctypes.POINTER(ctypes.c_int), ip, ip, ip, ip, ctypes.c_char_p, ip]),
        "seg_op_conv_dgrad_fused": (ip, [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, vp, ip,
                                         vp, ip, vp, ip, vp, ip, ip, vp, vp, vp]),
        "seg_op_bn_rowblocks": (ip, [i64, ip]),
        "seg_op_bn_stats_finalize": (ip, [vp, i64, ip, ip, vp, vp, vp, vp, vp, vp, vp]),
        "seg_op_bn_apply": (ip, [ip, ip, ctypes.POINTER(BnApplyArgs), vp]),
        "seg_op_bn_backward": (ip, [ip, ip, ip, ip, ctypes.POINTER(BnBwdArgs), vp]),
        "seg_op_bn_backward_dual": (ip, [ip, ip, ip, ctypes.POINTER(BnBwdArgs),
                                         ctypes.POINTER(BnBwdArgs), vp]),
        "seg_bbox_labels": (ip, [vp, vp, vp, vp, ip, ip, ip, ip, vp, vp]),
        "seg_grad_buckets": (ip, [vp, ip, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
        "seg_stream_wait_bucket": (ip, [vp, ip, vp]),
        "seg_set_loss_scale": (ip, [vp, ctypes.c_float]),
        "seg_found_inf": (ip, [vp, ctypes.POINTER(ctypes.c_void_p)]),
        "seg_set_bn_sync": (ip, [vp, SEG_ALLREDUCE_FN, vp, ip]),
        "seg_tag_labels": (ip, [vp, ip, ip, ip, vp, vp]),
        "seg_set_bn_inference": (ip, [vp, ip]),
        "seg_prepare_images": (ip, [vp, ip, ip, ip, ip, ip, vp, vp]),
        "seg_prepare_images_crop": (ip, [vp, ip, ip, ip, ip, ip, ip, ip, ip, ip, vp, vp]),
        "seg_prepare_labels": (ip, [vp, ip, ip, ip, ip, ip, ctypes.POINTER(ctypes.c_int32), ip,
                                    vp, vp]),
        "seg_bbox_labels_flip": (ip, [vp, vp, vp, vp, vp, ip, ip, ip, ip, vp, vp]),
        "seg_augment_workspace": (ip, [ip, ip, ip, ctypes.POINTER(i64)]),
        "seg_augment_images": (ip, [vp, ip, ip, ip, ip, ip, ip, ip, ip, ip, vp, vp, vp, vp, i64, vp]),
        "seg_augment_labels": (ip, [vp, ip, ip, ip, ip, ip, ctypes.POINTER(ctypes.c_int32), ip,
                                    vp, vp, vp, vp]),
        "seg_augment_profile": (ip, [ip, ctypes.POINTER(ctypes.c_float)]),
        "seg_augment_profile_blur": (ip, [ctypes.POINTER(ctypes.c_float)]),
        "seg_crc32c": (ctypes.c_uint32, [ctypes.c_uint32, vp, ctypes.c_size_t]),
        "seg_predict": (ip, [vp, ctypes.POINTER(ctypes.c_int32), ip, ip, ip, ip, vp, vp]),
        "seg_full_predictions": (ip, [vp, vp, vp, vp, vp, vp]),
        "seg_set_nesterov": (ip, [vp, ip]),
        "seg_set_defer_stem": (ip, [vp, ip]),
        "seg_flush_grads": (ip, [vp, vp]),
        "seg_set_premask": (ip, [vp, ip]),
        "seg_set_lbf": (ip, [vp, ip]),
        "seg_counter": (ip, [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
        "seg_set_bootstrap": (ip, [vp, ip]),
        "seg_op_bootstrap_threshold": (ip, [vp, i64, i64, ctypes.POINTER(f), ctypes.POINTER(i64), vp]),
        "seg_resize_images": (ip, [vp, ip, ip, ip, ip, ip, ip, vp, vp]),
        "seg_tta_decisions": (ip, [vp, ctypes.POINTER(TtaEntry), ip, ctypes.POINTER(ctypes.c_int32),
                                   ip, ip, ip, ip, vp, vp, vp]),
        "seg_window_images": (ip, [vp, ip, ip, ip, ip, ip, ip, ip, ip, vp, vp]),
        "seg_window_decisions": (ip, [vp, ctypes.POINTER(vp), ip, ip, ip, ctypes.POINTER(ip), ip,
                                      ctypes.POINTER(ip), ip, ip, ip, ip,
                                      ctypes.POINTER(ctypes.c_int32), ip, ip, ip, ip, vp, vp, vp]),
        "seg_crf_workspace": (ip, [ip, ip, ip, ip, ctypes.POINTER(i64)]),
        "seg_crf_decisions": (ip, [vp, vp, vp, ip, ip, ip, ctypes.POINTER(CrfParams), vp, i64,
                                   ctypes.POINTER(ctypes.c_int32), ip, ip, ip, ip, vp, vp, vp]),
        "seg_box_kinds": (ip, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "seg_box_constrain": (ip, [vp, vp, ip, ip, ip, vp, vp, vp, vp, ip, vp, vp, vp]),
        "seg_box_decisions": (ip, [vp, vp, ip, ip, ip, vp, vp, vp, vp, ip, f, vp, vp, vp, vp]),
        "seg_box_finalize": (ip, [vp, vp, ip, ip, ip, vp, vp, vp, vp, ip, vp, ip, ip, vp, vp]),
        "seg_boundary_distance": (ip, [vp, vp, ip, ip, ip, ip, ip, ip, vp, vp]),
        "seg_band_confusion_workspace": (ip, [ip, ip, ip, ip, ip, ctypes.POINTER(i64)]),
        "seg_band_confusion": (ip, [vp, vp, vp, ip, ip, ip, ip, ip, ctypes.POINTER(ctypes.c_int32), ip,
                                    vp, i64, vp, vp]),
    }
    override = "SEG_HIP_LIB" in os.environ   # A/B builds of older commits may lack new entries
    for name, (res, args) in sig.items():
        if override and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


LIB = _load()


def check(rc: int, ctx=None):
    if rc != 0:
        msg = LIB.seg_last_error(ctx)
        raise RuntimeError(f"libseg_hip error {rc}: {msg.decode() if msg else ''}")


def crf_workspace_bytes(n: int, H: int, W: int, ct: int) -> int:
    """seg_crf_workspace: bytes of the two Q buffers of ``SegContext.crf_decisions``."""
    b = ctypes.c_int64()
    check(LIB.seg_crf_workspace(int(n), int(H), int(W), int(ct), ctypes.byref(b)))
    return b.value


def band_confusion_workspace_bytes(n: int, H: int, W: int, n_widths: int, num_classes: int) -> int:
    """seg_band_confusion_workspace: bytes of the workspace of ``SegContext.band_confusion``."""
    b = ctypes.c_int64()
    check(LIB.seg_band_confusion_workspace(int(n), int(H), int(W), int(n_widths), int(num_classes),
                                           ctypes.byref(b)))
    return b.value


def _check_tensor(t, dtype, rank, n, name, tail=()):
    """``t`` must be a contiguous device tensor of ``dtype`` and ``rank`` whose leading dimension is
    ``n`` (None: any) and whose last dimensions are ``tail``; ``name`` is what the message calls it."""
    if not (t.dtype == dtype and t.is_cuda and t.is_contiguous() and t.dim() == rank
            and (n is None or t.shape[0] == n) and tuple(t.shape[rank - len(tail):]) == tuple(tail)):
        dims = ["n" if n is None else str(n)] + ["*"] * (rank - 1 - len(tail)) + [str(v) for v in tail]
        raise ValueError(f"{name} must be a contiguous device {str(dtype).split('.')[-1]} "
                         f"[{', '.join(dims)}], got {tuple(t.shape)} {t.dtype}")


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


@dataclass
class ParamInfo:
    name: str
    offset: int
    numel: int
    kind: str
    shape: tuple


@dataclass
class DeviceBoxLists:
    """A ``BoxLists`` on the device (``SegContext.upload_boxes``): the box arrays of the C ABI,
    the per-image maximum, the total and the (H, W) of the label maps their geometry is for."""
    boxes: object
    cids: object
    box_off: object
    geom: object
    n: int
    max_boxes: int
    total: int
    size: tuple


class SegContext:
    """One device context of the native training path (one per GPU per process).

    Owns the flat fp32 buffers (as torch tensors on the context's device): ``params``,
    ``grads`` (+ BN batch-statistics tail), ``momentum``, optional ``ema`` and ``moving``.
    """

    def __init__(self, *, depth=50, pyramid="psp", height=512, width=1024, nb_pp=2, nb_pb=0,
                 nb_pi=0, dtype="bf16", dataset="cityscapes", output_stride=8,
                 feature_dims=256, bn_decay=0.9, train_bn=True, weight_decay=0.00017,
                 ema=False, device=None, fov_k=0, fov_rate=0, upsampling="bilinear",
                 norm="batch", groups=0):
        import torch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.cfg = SegCfg(depth, PYRAMID[pyramid], height, width, nb_pp, nb_pb, nb_pi,
                          DTYPE[dtype], DATASET[dataset], output_stride, feature_dims,
                          bn_decay, int(bool(train_bn)), weight_decay, fov_k, fov_rate,
                          UPSAMPLING[upsampling], NORM[norm], groups)
        self.dtype = dtype
        self.head_widths, self.n_classes = HEAD_LAYOUT[dataset]
        self.batch_size = nb_pp + nb_pb + nb_pi
        h = ctypes.c_void_p()
        check(LIB.seg_create(self.device.index, ctypes.byref(self.cfg), ctypes.byref(h)))
        self.h = h
        vals = [ctypes.c_int64() for _ in range(4)]
        check(LIB.seg_sizes(self.h, *[ctypes.byref(v) for v in vals]), self.h)
        self.n_train, self.n_decay, self.n_moving, self.n_stats = [v.value for v in vals]
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.n_train, **f32)
        self.grads = torch.zeros(self.n_train + self.n_stats, **f32)
        self.momentum = torch.zeros(self.n_train, **f32)
        self.ema = torch.zeros(self.n_train, **f32) if ema else None
        self.moving = torch.zeros(self.n_moving, **f32)
        check(LIB.seg_bind_buffers(self.h, _ptr(self.params), _ptr(self.grads),
                                   _ptr(self.momentum), _ptr(self.ema), _ptr(self.moving)), self.h)
        self.param_info = self._param_info()
        self.params_version = 0   # refreshes of the compute copies so far (params_updated)

    # ---- parameters -----------------------------------------------------------------
    def _param_info(self) -> List[ParamInfo]:
        out = []
        for i in range(LIB.seg_param_count(self.h)):
            nm, off, n, k = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
            check(LIB.seg_param_info(self.h, i, ctypes.byref(nm), ctypes.byref(off),
                                     ctypes.byref(n), ctypes.byref(k)), self.h)
            dims = (ctypes.c_int64 * 4)()
            check(LIB.seg_param_shape(self.h, i, dims), self.h)
            kind = PARAM_KIND[k.value]
            shape = tuple(dims) if kind == "weights" else (dims[0],)
            out.append(ParamInfo(nm.value.decode(), off.value, n.value, kind, shape))
        return out

    def _buffer_for(self, p: ParamInfo):
        return self.moving if p.kind in ("moving_mean", "moving_variance") else self.params

    def load_params(self, values: Dict[str, np.ndarray], stream=None):
        """Write named parameters (weights [Co][KH][KW][Ci]) and refresh compute copies."""
        import torch
        for p in self.param_info:
            if p.name in values:
                v = torch.as_tensor(np.asarray(values[p.name], dtype=np.float32).reshape(-1))
                if v.numel() != p.numel:
                    raise ValueError(f"{p.name}: expected {p.numel} values, got {v.numel()}")
                self._buffer_for(p)[p.offset:p.offset + p.numel].copy_(v.to(self.device))
        if self.ema is not None:
            self.ema.copy_(self.params)
        self.params_updated(stream)

    def params_updated(self, stream=None):
        """seg_params_updated: refresh the compute copies after ``params`` / ``moving`` were
        written. ``params_version`` counts these refreshes: holders of a copy of the parameters
        (the test-time augmentation contexts) compare it to know when to copy again."""
        check(LIB.seg_params_updated(self.h, _stream(stream)), self.h)
        self.params_version += 1

    def named(self, buffer: str = "params") -> Dict[str, np.ndarray]:
        """Host copies of named tensors of params/grads/momentum/ema."""
        buf = {"params": self.params, "grads": self.grads, "momentum": self.momentum,
               "ema": self.ema}[buffer]
        if buffer == "grads":   # a deferred stem weight gradient (seg_set_defer_stem) finishes first
            self.flush_grads()
        out = {}
        for p in self.param_info:
            if p.kind in ("moving_mean", "moving_variance"):
                src = self.moving if buffer == "params" else None
            else:
                src = buf
            if src is not None:
                out[p.name] = src[p.offset:p.offset + p.numel].detach().cpu().numpy()
        return out

    def flush_grads(self, stream=None):
        """Join a still-running deferred stem weight gradient (seg_set_defer_stem) on ``stream``
        so the gradient buffer is complete; a no-op otherwise."""
        check(LIB.seg_flush_grads(self.h, _stream(stream)), self.h)

    # ---- step -----------------------------------------------------------------------
    def forward(self, images, stream=None):
        check(LIB.seg_forward(self.h, _ptr(images), _stream(stream)), self.h)
        self.forward_count = getattr(self, "forward_count", 0) + 1

    def loss(self, px_labels=None, bbox_soft=None, tag_soft=None, decisions=None, stream=None):
        check(LIB.seg_loss(self.h, _ptr(px_labels), _ptr(bbox_soft), _ptr(tag_soft),
                           _ptr(decisions), _stream(stream)), self.h)

    def set_bn_inference(self, on: bool):
        """BN normalises with the moving statistics in later forwards (is_training=False,
        the reference's default unless --batch_norm_accumulate_statistics)."""
        check(LIB.seg_set_bn_inference(self.h, 1 if on else 0), self.h)
        self.bn_inference = bool(on)

    def _decision_args(self, cid_map, out, mean_probs=None, n=None):
        """(batch size, cid_map as a C array) after the checks the decision calls share: ``out`` a
        contiguous device int32 [n, Ho, Wo], ``mean_probs`` None or a contiguous device float32
        [n, H, W, C]. ``n``: the batch size when it is not the context's."""
        import torch
        n = self.batch_size if n is None else n
        _check_tensor(out, torch.int32, 3, n, "decisions buffer")
        if mean_probs is not None:
            _check_tensor(mean_probs, torch.float32, 4, n, "mean_probs")
        return n, (ctypes.c_int32 * len(cid_map))(*[int(v) for v in cid_map])

    def predict(self, cid_map, out, replace_voids=False, stream=None, order="eval"):
        """Decisions of the last forward mapped through ``cid_map`` (training -> eval/inference
        cids, -1 = void), optionally void-replaced, nearest-neighbour resized to out's
        [N, Ho, Wo] (device int32). ``order``: "eval" replaces voids at network resolution
        before the resize (the EVAL branch); "predict" resizes first -- l1 probabilities
        bilinearly (align_corners) -- and replaces voids on the resized probabilities (the
        PREDICT branch, define_estimator_hierarchical.py:227-231)."""
        if order not in ("eval", "predict"):
            raise ValueError(f"order must be 'eval' or 'predict', got {order!r}")
        _, m = self._decision_args(cid_map, out)
        rv = (2 if order == "predict" else 1) if replace_voids else 0
        check(LIB.seg_predict(self.h, m, len(cid_map), rv,
                              int(out.shape[1]), int(out.shape[2]), _ptr(out), _stream(stream)),
              self.h)

    def full_predictions(self, logits=None, probs=None, head_decisions=None, decisions=None,
                         stream=None):
        """The model's full-resolution predictions of the last forward at network resolution
        (hierarchical.py:84-130) written into the given device buffers (any may be None):
        logits / probs f32 [N, H, W, C] (C = c1 + c2 + c3, heads l1 | l2v | l2h),
        head_decisions int32 [N, H, W, 3], decisions int32 [N, H, W] (fused, common cids)."""
        import torch
        hw, ct = (self.cfg.height, self.cfg.width), (sum(self.head_widths),)
        for name, t, dt, tail in (("logits", logits, torch.float32, ct), ("probs", probs, torch.float32, ct),
                                  ("head_decisions", head_decisions, torch.int32, (3,)),
                                  ("decisions", decisions, torch.int32, ())):
            if t is not None:
                _check_tensor(t, dt, 3 + len(tail), self.batch_size, name, hw + tail)
        check(LIB.seg_full_predictions(self.h, _ptr(logits), _ptr(probs), _ptr(head_decisions),
                                       _ptr(decisions), _stream(stream)), self.h)

    def tta_decisions(self, entries, cid_map, out, replace_voids=False, mean_probs=None,
                      stream=None):
        """seg_tta_decisions: decisions from the probabilities averaged over ``entries``, a list
        of (logits, flip): logits a contiguous device f32 [N, h_low, w_low, ld] (ld >= c1 + c2 +
        c3 is the pixel stride) of one scale's forward, flip True when that forward saw the
        mirrored image. ``cid_map`` / ``out`` / ``replace_voids`` as in ``predict`` (mode
        "eval"; the "predict" order is not defined for averaged probabilities). ``mean_probs``:
        optional device f32 [N, H, W, c1 + c2 + c3] for the mean probabilities; needs out's
        size to be the network size. The context's own logits are not read."""
        import torch
        n, m = self._decision_args(cid_map, out, mean_probs)
        if len(entries) > TTA_MAX_ENTRIES:
            raise ValueError(f"{len(entries)} entries: at most {TTA_MAX_ENTRIES} "
                             "(scales x flips) per decision launch")
        arr = (TtaEntry * max(len(entries), 1))()
        for i, (lg, flip) in enumerate(entries):
            _check_tensor(lg, torch.float32, 4, n, f"entry {i}: logits")
            arr[i] = TtaEntry(lg.data_ptr(), int(lg.shape[1]), int(lg.shape[2]), int(lg.shape[3]),
                              int(flip))
        check(LIB.seg_tta_decisions(self.h, arr, len(entries), m, len(cid_map), int(replace_voids),
                                    int(out.shape[1]), int(out.shape[2]), _ptr(mean_probs),
                                    _ptr(out), _stream(stream)), self.h)

    def window_decisions(self, entries, ys, xs, flip, canvas_hw, cid_map, out,
                         replace_voids=False, mean_probs=None, stream=None):
        """seg_window_decisions: decisions from the probabilities averaged over the windows that
        cover each pixel of a canvas. ``entries``: contiguous device f32 [N, h_low, w_low, ld]
        tensors of one shape, the low-resolution logits of this context's forwards on the
        windows at origins ``ys`` x ``xs`` of the ``canvas_hw`` canvas, in entry order (rows of
        ys outermost, then xs, then with ``flip`` the unflipped entry followed by the mirrored
        one). ``cid_map`` / ``out`` / ``replace_voids`` as in ``tta_decisions``; the nearest
        resize to out's size starts from the canvas. ``mean_probs``: optional device f32
        [N, Hc, Wc, c1 + c2 + c3]; needs out's size to be the canvas size. The context's own
        logits are not read."""
        import torch
        n, m = self._decision_args(cid_map, out, mean_probs)
        ys, xs = [int(v) for v in ys], [int(v) for v in xs]
        want = len(ys) * len(xs) * (2 if flip else 1)
        if want > WIN_MAX_ENTRIES:
            raise ValueError(f"{len(ys)} x {len(xs)} windows{' with flip' if flip else ''} are "
                             f"{want} entries: at most {WIN_MAX_ENTRIES} per decision launch")
        if len(entries) != want or want == 0:
            raise ValueError(f"{len(entries)} entries for {len(ys)} x {len(xs)} windows"
                             f"{' with flip' if flip else ''}: expected {want} (at least 1)")
        shape = tuple(entries[0].shape)
        for i, lg in enumerate(entries):   # all of the first entry's shape
            _check_tensor(lg, torch.float32, 4, n, f"entry {i}: logits", shape[1:])
        ptrs = (_VP * want)(*[lg.data_ptr() for lg in entries])
        check(LIB.seg_window_decisions(self.h, ptrs, shape[1], shape[2], shape[3],
                                       (_INT * len(ys))(*ys), len(ys), (_INT * len(xs))(*xs), len(xs),
                                       int(bool(flip)), int(canvas_hw[0]), int(canvas_hw[1]), m,
                                       len(cid_map), int(replace_voids), int(out.shape[1]),
                                       int(out.shape[2]), _ptr(mean_probs), _ptr(out),
                                       _stream(stream)), self.h)

    def crf_decisions(self, probs, images, crf, cid_map, out, replace_voids=False, workspace=None,
                      probs_out=None, stream=None):
        """seg_crf_decisions: decisions from ``probs`` (contiguous device f32 [n, H, W, c1 + c2 +
        c3], per-head probabilities) after ``crf.iterations`` mean-field steps conditioned on
        ``images`` (contiguous device f32 [n, H, W, 3], the prepared batch at the same size).
        ``crf``: a ``CrfParams``. ``cid_map`` / ``out`` / ``replace_voids`` as in
        ``tta_decisions``; the nearest resize to out's size starts from H x W, the size of
        ``probs``, whatever the context's own size is. ``workspace``: a contiguous device buffer of
        at least ``crf_workspace_bytes(n, H, W, ct)`` bytes (needed when iterations >= 1; the
        caller owns it). ``probs_out``: optional device f32 of probs' shape for the refined
        probabilities Q^T."""
        import torch
        _check_tensor(probs, torch.float32, 4, None, "probs")
        n, H, W, ct = (int(v) for v in probs.shape)
        _check_tensor(images, torch.float32, 4, n, "images", (H, W, 3))
        _, m = self._decision_args(cid_map, out, n=n)
        if probs_out is not None:
            _check_tensor(probs_out, torch.float32, 4, n, "probs_out", (H, W, ct))
        if workspace is not None and not (workspace.is_cuda and workspace.is_contiguous()):
            raise ValueError("workspace must be a contiguous device buffer")
        ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
        check(LIB.seg_crf_decisions(self.h, _ptr(probs), _ptr(images), n, H, W, ctypes.byref(crf),
                                    _ptr(workspace), ws_bytes, m, len(cid_map), int(replace_voids),
                                    int(out.shape[1]), int(out.shape[2]), _ptr(probs_out), _ptr(out),
                                    _stream(stream)), self.h)

    def box_kinds(self):
        """seg_box_kinds: per weak class 0..13, 1 for a vehicle box, 2 for a human box, 0 for an
        inert one, under this context's head tables."""
        kinds = (ctypes.c_int32 * 14)()
        check(LIB.seg_box_kinds(self.h, kinds), self.h)
        return list(kinds)

    def upload_boxes(self, box_lists, size):
        """A ``BoxLists`` (items (cids, coords, src_size, resized_size, offset), no flip) on the
        device, for label maps of ``size`` = (H, W): the ``DeviceBoxLists`` the ``box_*`` calls take.
        One upload serves every call of a batch."""
        import torch
        from input_pipelines.weak_labels import pack_box_lists
        items = [tuple(im) for im in box_lists]
        if any(len(im) > 5 and int(im[5]) for im in items):
            raise ValueError("box labels are not defined for flipped box lists")
        boxes, cids, off, geom, counts = pack_box_lists([im[:5] for im in items], size)
        dev = torch.device(self.device)
        tb, tc, to, tg = (torch.as_tensor(x).to(dev) for x in (boxes, cids, off, geom))
        return DeviceBoxLists(tb, tc, to, tg, len(items), max(counts, default=0), int(off[-1]),
                              (int(size[0]), int(size[1])))

    def _boxes_for(self, boxes, n, H, W):
        b = boxes if isinstance(boxes, DeviceBoxLists) else self.upload_boxes(boxes, (H, W))
        if b.n != n or b.size != (H, W):
            raise ValueError(f"box lists of {b.n} images for {b.size[0]}x{b.size[1]} maps, the call "
                             f"has {n} images of {H}x{W}")
        return b

    def box_constrain(self, probs, boxes, probs_out, mask_out=None, stream=None):
        """seg_box_constrain: ``probs`` (contiguous device f32 [n, H, W, c1 + c2 + c3]) with every
        l2 head restricted to the channels the boxes covering the pixel allow, into ``probs_out``
        (same shape, not ``probs``). ``boxes``: a ``BoxLists`` or an ``upload_boxes`` result for
        H x W. ``mask_out``: optional device int16 [n, H, W], bit k = a box of class k covers the
        pixel. Returns the uploaded boxes."""
        import torch
        _check_tensor(probs, torch.float32, 4, None, "probs")
        n, H, W, ct = (int(v) for v in probs.shape)
        _check_tensor(probs_out, torch.float32, 4, n, "probs_out", (H, W, ct))
        if mask_out is not None:
            _check_tensor(mask_out, torch.int16, 3, n, "mask_out", (H, W))
        b = self._boxes_for(boxes, n, H, W)
        check(LIB.seg_box_constrain(self.h, _ptr(probs), n, H, W, _ptr(b.boxes), _ptr(b.cids),
                                    _ptr(b.box_off), _ptr(b.geom), b.max_boxes, _ptr(probs_out),
                                    _ptr(mask_out), _stream(stream)), self.h)
        return b

    def box_decisions(self, q, boxes, tau, labels_out, counts_out, conf_out=None, stream=None):
        """seg_box_decisions: labels in training cids (device int32 [n, H, W]) from ``q``
        (contiguous device f32 [n, H, W, c1 + c2 + c3], constrained and possibly refined
        probabilities), the fine class taken among the channels the covering boxes allow, the void
        cid for an unboxed vehicle / human pixel or an l1 confidence below ``tau``.
        ``counts_out``: device int32 [total boxes (at least 1), 2] = (area, hit) per box.
        ``conf_out``: optional device f32 [n, H, W]. Returns the uploaded boxes."""
        import torch
        _check_tensor(q, torch.float32, 4, None, "q")
        n, H, W, _ = (int(v) for v in q.shape)
        _check_tensor(labels_out, torch.int32, 3, n, "labels_out", (H, W))
        if conf_out is not None:
            _check_tensor(conf_out, torch.float32, 3, n, "conf_out", (H, W))
        b = self._boxes_for(boxes, n, H, W)
        _check_tensor(counts_out, torch.int32, 2, max(b.total, 1), "counts_out", (2,))
        check(LIB.seg_box_decisions(self.h, _ptr(q), n, H, W, _ptr(b.boxes), _ptr(b.cids),
                                    _ptr(b.box_off), _ptr(b.geom), b.max_boxes, float(tau),
                                    _ptr(labels_out), _ptr(conf_out), _ptr(counts_out),
                                    _stream(stream)), self.h)
        return b

    def box_finalize(self, labels, boxes, reject, out, stream=None):
        """seg_box_finalize: ``labels`` (device int32 [n, H, W]) nearest-neighbour resized
        (align_corners) to ``out`` (device int32 [n, Ho, Wo]), the void cid under every box whose
        entry of ``reject`` (device int32 [total boxes (at least 1)]) is nonzero. Returns the
        uploaded boxes."""
        import torch
        _check_tensor(labels, torch.int32, 3, None, "labels")
        n, H, W = (int(v) for v in labels.shape)
        _check_tensor(out, torch.int32, 3, n, "out")
        b = self._boxes_for(boxes, n, H, W)
        _check_tensor(reject, torch.int32, 1, max(b.total, 1), "reject")
        check(LIB.seg_box_finalize(self.h, _ptr(labels), n, H, W, _ptr(b.boxes), _ptr(b.cids),
                                   _ptr(b.box_off), _ptr(b.geom), b.max_boxes, _ptr(reject),
                                   int(out.shape[1]), int(out.shape[2]), _ptr(out),
                                   _stream(stream)), self.h)
        return b

    def backward(self, stream=None):
        check(LIB.seg_backward(self.h, _stream(stream)), self.h)

    def set_loss_scale(self, scale: float):
        """Gradient-seed multiplier (fp16 dynamic loss scaling; see seg_set_loss_scale)."""
        check(LIB.seg_set_loss_scale(self.h, float(scale)), self.h)
        self.loss_scale = float(scale)

    def found_inf(self):
        """Device int32 view of the last update's overflow flag (None unless loss scaling)."""
        p = ctypes.c_void_p()
        check(LIB.seg_found_inf(self.h, ctypes.byref(p)), self.h)
        return None if not p.value else _wrap_i32(p.value, (1,), self.device)

    def set_bn_sync(self, world=None, group=None, always=False):
        """Cross-replica batch norm (the reference's --cross_replica_norm, see seg_set_bn_sync):
        each BN layer's moments (forward) and gradient means (backward) are summed over
        `group` by torch.distributed.all_reduce (RCCL or gloo) ordered on the step's stream.
        world=None takes the group's size; a world of 1 turns synchronisation off unless
        `always` (then the one-replica group still runs every exchange: tests of the
        collective path on one GPU)."""
        import torch
        import torch.distributed as dist
        if world is None:
            world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if world <= 1 and not always:
            check(LIB.seg_set_bn_sync(self.h, SEG_ALLREDUCE_FN(), None, 1), self.h)
            self._sync_cb = None
            return
        dev = self.device

        def _exchange(user, buf, n, stream):   # called from inside seg_forward / seg_backward
            try:
                t = _wrap(buf, (int(n),), dev)
                s = (torch.cuda.ExternalStream(stream, device=dev) if stream
                     else torch.cuda.default_stream(dev))
                with torch.cuda.stream(s):
                    dist.all_reduce(t, group=group)
                return 0
            except Exception as e:  # reported through the failing seg_* call
                self.sync_error = e
                return 1
        cb = SEG_ALLREDUCE_FN(_exchange)
        check(LIB.seg_set_bn_sync(self.h, cb, None, int(world)), self.h)
        self._sync_cb = cb   # the C side holds the raw pointer: keep the thunk alive

    def grad_buckets(self):
        """[(lo, hi)] ranges of self.grads in the order the backward completes them."""
        n = LIB.seg_grad_buckets(self.h, 0, None, None)
        if n < 0:
            check(n, self.h)
        lo, hi = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        check(LIB.seg_grad_buckets(self.h, n, lo, hi) - n, self.h)
        return [(int(lo[i]), int(hi[i])) for i in range(n)]

    def wait_bucket(self, i, stream):
        """Make `stream` wait until the last seg_backward has written bucket i."""
        check(LIB.seg_stream_wait_bucket(self.h, i, _stream(stream)), self.h)

    def set_nesterov(self, on: bool):
        """MomentumOptimizer(use_nesterov=on) for the following updates."""
        check(LIB.seg_set_nesterov(self.h, 1 if on else 0), self.h)
        self.nesterov = bool(on)

    def set_defer_stem(self, on: bool):
        """Single-process training loops: update every other parameter beside the stem's weight
        gradient (the step's last kernel); gradients must not be read between backward() and
        apply_update() while this is on."""
        check(LIB.seg_set_defer_stem(self.h, 1 if on else 0), self.h)

    def set_premask(self, on):
        """seg_set_premask: pre-masked identity-unit gradients (default on; results unchanged)."""
        check(LIB.seg_set_premask(self.h, 1 if on else 0), self.h)

    def set_lbf(self, on):
        """seg_set_lbf: the linear BN-backward fold of the bottleneck conv3 layers (default on;
        off = the separate BN-backward apply pass, the fold's reference path in tests)."""
        check(LIB.seg_set_lbf(self.h, 1 if on else 0), self.h)

    def set_bootstrap(self, percentage: int):
        """seg_set_bootstrap: bootstrapped l1 loss over the hardest `percentage` % of the strong
        images' pixels (--bootstrapping_percentage); <= 0 turns it off, > 100 is an error."""
        check(LIB.seg_set_bootstrap(self.h, int(percentage)), self.h)
        self.bootstrap = int(percentage) if percentage > 0 else -1

    def counter(self, name: str) -> int:
        """seg_counter: a runtime counter since creation (e.g. "premask_launches")."""
        v = ctypes.c_int64()
        check(LIB.seg_counter(self.h, name.encode(), ctypes.byref(v)), self.h)
        return v.value

    def apply_update(self, lr, momentum=0.9, ema_decay_eff=0.0, grad_scale=1.0, stream=None):
        check(LIB.seg_apply_update(self.h, lr, momentum, ema_decay_eff, grad_scale,
                                   _stream(stream)), self.h)

    def outputs(self):
        """(losses[10], reg[1], low-res logits [N,Hl,Wl,ldl]) as torch views (device)."""
        import torch
        l, r, lg = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        ld, hl, wl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(LIB.seg_outputs(self.h, ctypes.byref(l), ctypes.byref(r), ctypes.byref(lg),
                              ctypes.byref(ld), ctypes.byref(hl), ctypes.byref(wl)), self.h)
        n = self.batch_size
        return (_wrap(l.value, (10,), self.device), _wrap(r.value, (1,), self.device),
                _wrap(lg.value, (n, hl.value, wl.value, ld.value), self.device))

    def confusion(self, labels, decisions, num_classes, out, stream=None):
        check(LIB.seg_confusion(self.h, _ptr(labels), _ptr(decisions), labels.numel(),
                                num_classes, _ptr(out), _stream(stream)), self.h)

    def boundary_distance(self, labels, num_classes, ignore, max_width, out=None, stream=None):
        """seg_boundary_distance: per pixel of ``labels`` (contiguous device int32 [n, H, W]) the
        squared distance to the nearest boundary pixel of its image, capped at ``max_width``^2 + 1
        (``max_width`` 1..64). A boundary pixel carries a counted label (0 <= l < ``num_classes``,
        l != ``ignore``; ``ignore`` -1 for none) and has a 4-neighbour with another counted label.
        ``out``: device int16 [n, H, W] holding the uint16 values (at most 4097: never negative),
        allocated when None. Returns ``out``."""
        import torch
        _check_tensor(labels, torch.int32, 3, None, "labels")
        n, H, W = (int(v) for v in labels.shape)
        if out is None:
            out = torch.empty((n, H, W), dtype=torch.int16, device=labels.device)
        _check_tensor(out, torch.int16, 3, n, "out", (H, W))
        check(LIB.seg_boundary_distance(self.h, _ptr(labels), n, H, W, int(num_classes), int(ignore),
                                        int(max_width), _ptr(out), _stream(stream)), self.h)
        return out

    def band_confusion(self, labels, decisions, num_classes, ignore, widths, out, stream=None):
        """seg_band_confusion: ``out`` (device int32 [K, num_classes, num_classes], overwritten) =
        the confusion matrices of ``labels`` against ``decisions`` (contiguous device int32
        [n, H, W], seg_confusion's acceptance rule) over the pixels within ``widths[k]`` pixels
        (Euclidean) of a boundary pixel of ``labels`` (``boundary_distance``). ``widths``: 1..8
        strictly increasing integers in 1..64. The workspace is kept on the context per (n, H, W),
        the way the CRF driver keeps its own."""
        import torch
        _check_tensor(labels, torch.int32, 3, None, "labels")
        n, H, W = (int(v) for v in labels.shape)
        _check_tensor(decisions, torch.int32, 3, n, "decisions", (H, W))
        widths = [int(w) for w in widths]
        nc = int(num_classes)
        _check_tensor(out, torch.int32, 3, len(widths), "out", (nc, nc))
        cache = self.__dict__.setdefault("_band_workspaces", {})
        if (n, H, W) not in cache:
            nbytes = band_confusion_workspace_bytes(n, H, W, max(len(widths), 1), nc)
            cache[(n, H, W)] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ws = cache[(n, H, W)]
        check(LIB.seg_band_confusion(self.h, _ptr(labels), _ptr(decisions), n, H, W, nc, int(ignore),
                                     (ctypes.c_int32 * len(widths))(*widths), len(widths), _ptr(ws),
                                     ws.numel(), _ptr(out), _stream(stream)), self.h)

    def debug_tensor(self, name: str):
        """Host copy (float32, [N,H,W,C]) of an internal tensor (parity tests only)."""
        import torch
        ptr = ctypes.c_void_p()
        dims = (ctypes.c_int * 4)()
        ld, dt = ctypes.c_int(), ctypes.c_int()
        check(LIB.seg_debug_tensor(self.h, name.encode(), ctypes.byref(ptr), dims, ctypes.byref(ld),
                                   ctypes.byref(dt)), self.h)
        n, hh, ww, c = list(dims)
        torch.cuda.synchronize()
        if dt.value == 0:
            t = _wrap(ptr.value, (n * hh * ww, ld.value), self.device)
        else:
            t = _wrap_u16(ptr.value, (n * hh * ww, ld.value), self.device, half=dt.value == 2)
        return t[:, :c].float().cpu().numpy().reshape(n, hh, ww, c)

    def debug_dims(self, name: str):
        """(N, H, W, C) of an internal tensor; a conv's input has them from seg_create on, its
        pointer only after the first forward (geometry tests read the dims without a step)."""
        dims = (ctypes.c_int * 4)()
        check(LIB.seg_debug_tensor(self.h, name.encode(), None, dims, None, None), self.h)
        return tuple(dims)

    def debug_device(self, name: str):
        """Zero-copy device view [N,H,W,C] (storage dtype, pixel stride ld) of an internal
        tensor: the full-size parity tests read 1024 x 2048 activations without a host copy."""
        import torch
        ptr = ctypes.c_void_p()
        dims = (ctypes.c_int * 4)()
        ld, dt = ctypes.c_int(), ctypes.c_int()
        check(LIB.seg_debug_tensor(self.h, name.encode(), ctypes.byref(ptr), dims, ctypes.byref(ld),
                                   ctypes.byref(dt)), self.h)
        n, hh, ww, c = list(dims)
        if dt.value == 0:
            t = _wrap(ptr.value, (n * hh * ww, ld.value), self.device)
        else:
            t = _wrap_u16(ptr.value, (n * hh * ww, ld.value), self.device, half=dt.value == 2)
        return t[:, :c].unflatten(0, (n, hh, ww))

    def profile(self, enable: bool):
        check(LIB.seg_profile(self.h, int(enable)), self.h)

    def profile_read(self, cls: int):
        ms, gf, mx = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int64()
        name = ctypes.create_string_buffer(256)
        check(LIB.seg_profile_read(self.h, cls, ctypes.byref(ms), ctypes.byref(gf), ctypes.byref(n),
                                   ctypes.byref(mx), name, 256), self.h)
        return dict(ms=ms.value, gflop=gf.value, launches=n.value, ms_max_layer=mx.value,
                    max_layer=name.value.decode())

    def profile_dump(self):
        """Per-launch records of the conv kernels: list of dicts."""
        buf = ctypes.create_string_buffer(1 << 22)
        check(LIB.seg_profile_dump(self.h, buf, len(buf)), self.h)
        rows = []
        for line in buf.value.decode().splitlines():
            f = line.split()
            rows.append(dict(cls=int(f[0]), name=f[1], ci=int(f[2]), co=int(f[3]), k=int(f[4]),
                             rate=int(f[5]), ho=int(f[6]), wo=int(f[7]), gflop=float(f[8]),
                             ms=float(f[9]), gbytes=float(f[10]) if len(f) > 10 else 0.0))
        return rows

    def close(self):
        if getattr(self, "h", None):
            LIB.seg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resize_images(x, h: int, w: int, flip: bool = False, stream=None):
    """seg_resize_images: contiguous device float32 [n, H, W, 3] -> [n, h, w, 3] by TF 1.12's
    legacy bilinear resize (align_corners = False) of the image, mirrored in x first when
    ``flip``. Equal sizes copy (or mirror) bit for bit."""
    import torch
    _check_tensor(x, torch.float32, 4, None, "images", (3,))
    out = torch.empty((x.shape[0], int(h), int(w), 3), dtype=torch.float32, device=x.device)
    check(LIB.seg_resize_images(_ptr(x), int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), int(h),
                                int(w), int(flip), _ptr(out), _stream(stream)))
    return out


def window_images(x, y0: int, x0: int, H: int, W: int, flip: bool = False, stream=None):
    """seg_window_images: the H x W window at (y0, x0) of a contiguous device float32 canvas
    [n, Hc, Wc, 3], mirrored in x when ``flip``: a bitwise copy [n, H, W, 3]."""
    import torch
    _check_tensor(x, torch.float32, 4, None, "images", (3,))
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"window size {H} x {W} must be positive")
    out = torch.empty((x.shape[0], int(H), int(W), 3), dtype=torch.float32, device=x.device)
    check(LIB.seg_window_images(_ptr(x), int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), int(y0),
                                int(x0), int(H), int(W), int(flip), _ptr(out), _stream(stream)))
    return out


def bootstrap_threshold(values, k: int, stream=None):
    """seg_op_bootstrap_threshold on a contiguous device float32 tensor of finite values >= +0:
    (rc, tau, n_ge) with tau the k-th largest entry and n_ge the count of entries >= tau; rc is
    the library's return code (-EINVAL for k outside 1..n), not raised."""
    tau, n_ge = ctypes.c_float(), ctypes.c_int64()
    rc = LIB.seg_op_bootstrap_threshold(_ptr(values), values.numel(), int(k), ctypes.byref(tau),
                                        ctypes.byref(n_ge), _stream(stream))
    return rc, tau.value, n_ge.value


def _wrap_u16(ptr: int, shape: Tuple[int, ...], device, half=False):
    """Zero-copy view of a bf16 (or fp16) device buffer (reinterpreted from int16)."""
    import torch

    class _CAI:
        pass
    o = _CAI()
    o.__cuda_array_interface__ = {"shape": shape, "typestr": "<i2", "data": (ptr, False),
                                  "version": 3, "strides": None}
    return torch.as_tensor(o, device=device).view(torch.float16 if half else torch.bfloat16)


def _wrap_i32(ptr: int, shape: Tuple[int, ...], device):
    import torch

    class _CAI:
        pass
    o = _CAI()
    o.__cuda_array_interface__ = {"shape": shape, "typestr": "<i4", "data": (ptr, False),
                                  "version": 3, "strides": None}
    return torch.as_tensor(o, device=device)


def _wrap(ptr: int, shape: Tuple[int, ...], device):
    """Zero-copy torch view of a context-owned fp32 device buffer."""
    import torch

    class _CAI:
        pass
    o = _CAI()
    o.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False),
                                  "version": 3, "strides": None}
    return torch.as_tensor(o, device=device)
