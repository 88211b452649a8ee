"""Parity at the benchmark's shapes (BASELINE config C2: R50 + ASPP, 1024 x 2048, 4 images per
GPU, bf16 storage / fp32 accumulation), through the production dispatch.

At these sizes every conv runs the kernels the bench times: the persistent ping-pong NT loop
(more 256 x 256 tiles than CUs, so each workgroup walks several tiles with the next tile's
DMA in flight during the epilogue), the non-persistent residual dgrad launches, the split-K
weight gradient with large pixel counts (op entry: ~2 waves of workgroups; in the step: the
side-stream sizing beside the dgrad -> BN chain), the v2 kernels for Co <= 128, the tap8
stem and the transposed-stride dgrad.

* ``test_conv_c2_layer`` — single layers through ``seg_op_conv_fwd / _dgrad / _wgrad``,
  every output element against the oracle's ``conv_tf`` on the CPU (float32 accumulation of
  the same bf16 / fp16 operands; the convolution of ``resnet50_extended_feature_extractor.py:
  25-30`` / ``hierarchical.py:59-64`` at the C2 layer shapes).
* ``test_step_layerwise_fullsize`` — one full training step (C2, C4, C5) of the native context, then every
  conv's forward output and weight gradient, and the whole backward chain of the data
  gradients (dgrad -> ReLU mask -> BN backward, residual and strided-subsample shortcuts,
  the ASPP transposes, the stem max-pool), against a float64 restatement fed the tensors the
  native step itself consumed (``oracle/conv_props.py``, pinned to ``conv_tf`` and autograd by
  ``tests/test_oracle.py``); plus the loss terms and fused decisions of the loss head against
  ``OracleNet.losses`` / ``head_predictions`` on the native low-resolution logits. The checker
  is ``tests/step_chain.py`` (shared with ``tests/test_gpu_odd_geometry.py``); its forward
  links (BN + ReLU, max-pool, unit outputs with their shortcuts, pyramid glue, each native
  16-bit tensor against the float64 restatement of the op that wrote it) are on here too.

Tolerances (written per check below):
* 16-bit outputs (forward y, data gradients of the op tests): per element
  |got - ref| <= 2u |ref| + 1e-3 rms(ref), u = 2^-8 (bf16) / 2^-11 (fp16) — one rounding of
  the fp32 accumulator plus summation-order noise; any missing tap, K-chunk or tile breaks it.
* fp32 weight gradients: per element |got - ref| <= 1e-3 |ref| + 1e-4 rms(ref), plus in the
  step 2^-24 sqrt(P) sum_p |dy x| (an fp32 sum over P pixels is off by ~sqrt(P) ulps of the
  absolute sum where the signed sum cancels; a missing 64-pixel K-step is ~20x that).
* BN-backward outputs of the step (dy of every conv): L2-relative 2e-2 over the tensor and
  5e-2 over every 256-pixel tile (bf16 dgrad outputs feed a cancelling formula: dh minus its
  mean and its x-hat projection).
"""
import math

import pytest
import torch

from oracle.tfseg import ConvSpec, SegConfig, conv_tf
from step_chain import ABI, TDT, ULP, _elementwise, step_chain

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------- single layers
C2_LAYERS = [
    # name, N, H, W, Ci, Co, k, stride, rate, explicit_pad
    ("block4_conv2_r4", 4, 128, 256, 512, 512, 3, 1, 4, False),
    ("block3_conv2_r2", 4, 128, 256, 256, 256, 3, 1, 2, False),
    ("block4_conv3_1x1_co2048", 4, 128, 256, 512, 2048, 1, 1, 1, False),
    ("block4_conv1_1x1_ci2048", 4, 128, 256, 2048, 512, 1, 1, 1, False),
    ("aspp_conv_r18", 4, 128, 256, 256, 256, 3, 1, 18, False),
    ("block1_conv2_s2", 4, 256, 512, 64, 64, 3, 2, 1, True),
    ("block2_conv1_co128", 4, 128, 256, 256, 128, 1, 1, 1, False),
    # the small-channel 3x3 patch kernel (conv_v2.hip conv_nt_patch_kernel): forward and the
    # stride-1 data gradient of block1 / block2 conv2
    ("block1_conv2_c64", 4, 256, 512, 64, 64, 3, 1, 1, False),
    ("block2_conv2_c128", 4, 128, 256, 128, 128, 3, 1, 1, False),
    ("l1_logits_co14", 4, 128, 256, 256, 14, 1, 1, 1, False),
]
LAYER_DTYPES = [(c, "bf16") for c in C2_LAYERS] + [(C2_LAYERS[0], "fp16"), (C2_LAYERS[2], "fp16"),
                                                    (C2_LAYERS[9], "fp16")]


def _operands(case, dtype, seed):
    _, N, H, W, Ci, Co, k, s, r, ep = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Ci, generator=g).to(TDT[dtype])
    w = (torch.randn(Co, k, k, Ci, generator=g) * math.sqrt(2.0 / (k * k * Ci))).to(TDT[dtype])
    return x, w


def _cpu_conv(x, w, spec):
    """oracle conv_tf in float32 on the CPU (NHWC in / out)."""
    return conv_tf(x.float().permute(0, 3, 1, 2), w.float(), spec).permute(0, 2, 3, 1)


@pytest.mark.parametrize("case,dtype", LAYER_DTYPES, ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_conv_c2_layer(cuda, case, dtype):
    from seg_hip import LIB, check
    name, N, H, W, Ci, Co, k, s, r, ep = case
    spec = ConvSpec(name, Ci, Co, k, s, r, explicit_pad=ep)
    x, w = _operands(case, dtype, 0)
    st = torch.cuda.current_stream().cuda_stream
    # ---- forward (+ the epilogue's BN partial statistics)
    ref = _cpu_conv(x, w, spec)
    Ho, Wo = ref.shape[1], ref.shape[2]
    M = N * Ho * Wo
    xd, wd = x.to(cuda), w.to(cuda)
    yd = torch.empty((N, Ho, Wo, Co), dtype=TDT[dtype], device=cuda)
    # BN partials: one per stat-rows block of the kernel the dispatcher picks (64 / 128 / 256)
    tr = LIB.seg_op_conv_stat_rows(ABI[dtype], N, H, W, Ci, Ci, Co, Co, k, s, r, int(ep))
    stats = torch.zeros(((M + tr - 1) // tr, Co, 2), dtype=torch.float32, device=cuda)
    check(LIB.seg_op_conv_fwd(ABI[dtype], xd.data_ptr(), N, H, W, Ci, Ci, wd.data_ptr(), Co, k, s, r,
                              int(ep), yd.data_ptr(), Co, stats.data_ptr(), st))
    torch.cuda.synchronize()
    refd = ref.to(cuda)
    _elementwise(yd, refd, 2 * ULP[dtype], 1e-3, f"{name} fwd")
    nt = (M + tr - 1) // tr
    sp = stats[:nt].double()
    cnt = torch.clamp(M - torch.arange(nt, device=cuda) * tr, max=tr).double()
    mean = sp[:, :, 0].sum(0) / M
    m2 = sp[:, :, 1].sum(0) + (cnt[:, None] * (sp[:, :, 0] / cnt[:, None] - mean) ** 2).sum(0)
    r64 = refd.double().reshape(-1, Co)
    sd = r64.std(0, unbiased=False)
    assert float(((mean - r64.mean(0)).abs() / sd).max()) < 1e-3, f"{name} BN mean"
    assert float(((m2 / M) / r64.var(0, unbiased=False) - 1).abs().max()) < 1e-3, f"{name} BN var"
    del yd, refd, r64, stats
    # ---- data gradient (the runtime passes the spatially flipped, transposed weights)
    g = torch.Generator().manual_seed(1)
    dy = torch.randn(N, Ho, Wo, Co, generator=g).to(TDT[dtype])
    xt = torch.zeros(N, Ci, H, W, requires_grad=True)
    conv_tf(xt, w.float(), spec).backward(dy.float().permute(0, 3, 1, 2))
    ref = xt.grad.permute(0, 2, 3, 1)
    wt = torch.flip(w, (1, 2)).permute(3, 1, 2, 0).contiguous()   # [Ci][k][k][Co]
    dyd, wtd = dy.to(cuda), wt.to(cuda)
    dx = torch.empty((N, H, W, Ci), dtype=TDT[dtype], device=cuda)
    check(LIB.seg_op_conv_dgrad(ABI[dtype], dyd.data_ptr(), N, Ho, Wo, Co, Co, wtd.data_ptr(), Ci, k,
                                s, r, int(ep), H, W, dx.data_ptr(), Ci, st))
    torch.cuda.synchronize()
    _elementwise(dx, ref.to(cuda), 2 * ULP[dtype], 1e-3, f"{name} dgrad")
    del dx, wtd
    # ---- weight gradient (split-K over the 131 k - 524 k pixels, fp32 slabs + reduce); the
    # runtime pads Co % 8 != 0 rows (the logits) itself: that one is covered by the step test
    if Co % 8:
        return
    wg = torch.zeros(Co, k, k, Ci, requires_grad=True)
    conv_tf(x.float().permute(0, 3, 1, 2), wg, spec).backward(dy.float().permute(0, 3, 1, 2))
    dw = torch.zeros((Co, k, k, Ci), dtype=torch.float32, device=cuda)
    ws = torch.empty(768 << 20, dtype=torch.uint8, device=cuda)
    check(LIB.seg_op_conv_wgrad(ABI[dtype], dyd.data_ptr(), N, Ho, Wo, Co, Co, xd.data_ptr(), H, W, Ci,
                                Ci, k, s, r, int(ep), dw.data_ptr(), ws.data_ptr(), ws.numel(), st))
    torch.cuda.synchronize()
    _elementwise(dw, wg.grad.to(cuda), 1e-3, 1e-4, f"{name} wgrad")


# ------------------------------------------------------------------------- one full C2 step
# the chain checker itself is tests/step_chain.py (shared with tests/test_gpu_odd_geometry.py)
# BASELINE configs at their per-GPU shape (1024 x 2048, 4 images): C2 as the bench runs it;
# C4 = R101 + pyramid with the 1:2:1 strong : bbox : tag mix in bf16 (covers C3's kernels and
# adds the weak-label loss head); C5 = the same mix in fp16 with fp32 master gradients under a
# loss scale of 4096 (the dynamic scaler settles at 8192 on these weights)
# C2-PSP = C2 with the reference's live pyramid module (_create_psp_module, hierarchical.py:
# 186-207; the shipped checkpoint uses it, README.md:31): at 1024 x 2048 the 3- and 6-grids pool
# 42 x 85 and 21 x 42 windows of the 128 x 256 map and drop the remainder rows and columns
FULL_CONFIGS = [
    ("C2", 50, "bf16", (4, 0, 0), "aspp"),
    ("C2-PSP", 50, "bf16", (4, 0, 0), "psp"),
    ("C4", 101, "bf16", (1, 2, 1), "aspp"),
    ("C5", 101, "fp16", (1, 2, 1), "aspp"),
]
FULL_LINKS = True   # the forward links of step_chain, at full size too


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,depth,dtype,mix,pyramid", FULL_CONFIGS, ids=[c[0] for c in FULL_CONFIGS])
def test_step_layerwise_fullsize(cuda, name, depth, dtype, mix, pyramid):
    npp, npb, npi = mix
    cfg = SegConfig(depth=depth, height=1024, width=2048, nb_pp=npp, nb_pb=npb, nb_pi=npi, pyramid=pyramid)
    rep = step_chain(cuda, cfg, dtype, param_seed=2, data_seed=17,
                     loss_scale=4096.0 if dtype == "fp16" else None, links=FULL_LINKS,
                     bn_tol=2e-2, tile_tol=5e-2)
    if pyramid == "psp":
        grids = rep["psp_grids"]
        assert grids[2] == (42, 85) and grids[3] == (21, 42)          # the dropped remainders
