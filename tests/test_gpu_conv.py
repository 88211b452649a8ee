"""Parity of the implicit-GEMM conv kernels (fwd / dgrad / wgrad, fp32, bf16 and fp16) against
the oracle's TF-semantics conv (torch CPU, float64). Tolerances: fp32 rel 1e-4 (exact-fp32
MFMA with a different summation order), bf16 rel 2e-2 and fp16 rel 3e-3 against a reference
fed the same rounded operands (fp32 accumulation on both sides; the output is rounded once).
Beside the L2-relative number, the forward, data-gradient and residual tests hold every element
to the derived bound of tests/conv_bounds.py (zero violations): the L2 number cannot see one
wave's worth of wrong elements in a multi-tile output (tests/test_conv_bounds.py)."""
import numpy as np
import pytest
import torch

from conv_bounds import violations
from oracle.tfseg import ConvSpec, conv_tf

pytestmark = pytest.mark.gpu

CASES = [
    # N, H, W, Ci, Co, k, stride, rate, explicit_pad
    (2, 13, 17, 64, 64, 3, 1, 2, False),      # dilated 3x3, ragged tiles
    (2, 16, 20, 128, 256, 3, 1, 4, False),    # rate 4
    (1, 11, 9, 256, 128, 1, 1, 1, False),     # 1x1
    (2, 18, 22, 64, 64, 3, 2, 1, True),       # conv2d_same stride 2
    (1, 37, 45, 3, 64, 7, 2, 1, True),        # stem (generic small-C path)
    (2, 9, 10, 256, 14, 1, 1, 1, False),      # logits (Co=14): skinny narrow-N / narrow-K
    (1, 37, 45, 256, 7, 1, 1, 1, False),      # l2 vehicle logits, ragged 128-row stats tiles
    (2, 9, 10, 256, 3, 1, 1, 1, False),       # l2 human logits
    (1, 6, 6, 1280, 256, 1, 1, 1, False),     # PSP final (C=1280)
    (2, 15, 21, 256, 512, 1, 1, 1, False),    # short K, wide N: 128-row tiles, 2 per CU
    (1, 20, 20, 128, 256, 1, 1, 1, False),    # ping-pong tile whose second wave row is ragged (16 rows)
    # small-channel 3x3 patch kernel (8 x 32 pixel tiles, input patch staged once per chunk)
    (2, 16, 64, 64, 64, 3, 1, 1, False),      # one 64-channel chunk, Co 64
    (1, 24, 96, 128, 128, 3, 1, 1, False),    # two chunks (second patch streamed), Co 128
    (1, 8, 32, 128, 64, 3, 1, 1, False),      # two chunks, Co 64 (its dgrad: one chunk, Co 128)
    # short-K dense 1x1 on the persistent ping-pong loop (several tiles per workgroup: the next
    # tile's prologue in flight during the epilogue); the dgrad of the same case is a short-K
    # problem too where Ci > 128
    (2, 16, 32, 256, 512, 1, 1, 1, False),    # K 256 -> 512: 4 x 2 tiles, one per workgroup
    (1, 16, 16, 64, 256, 1, 1, 1, False),     # K 64: one K-tile per tile
    (1, 128, 128, 256, 1024, 1, 1, 1, False), # 256 tiles
    (1, 96, 128, 128, 768, 1, 1, 1, False),  # 288 tiles: 2 or 1 per workgroup, K 128
    (2, 64, 128, 512, 1024, 1, 1, 1, False),  # K 512, 512 tiles; its dgrad K 1024 (ping-pong)
    # stride-2 conv2d_same (explicit padding): block2's strided unit runs the v2 128-channel tile
    # (its dgrad: the transposed gather, ST = 2), even and odd inputs, 64 and 128 channels; 256
    # channels reach the ping-pong kernel's ST = 2 instantiation (no output-stride-8 network
    # launches it, the op entries dispatch to it)
    (1, 18, 22, 128, 128, 3, 2, 1, True),
    (2, 17, 23, 64, 64, 3, 2, 1, True),
    (1, 19, 21, 128, 128, 3, 2, 1, True),
    (1, 18, 22, 256, 256, 3, 2, 1, True),
]


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _tensors(case, seed=0):
    N, H, W, Ci, Co, k, s, r, ep = case
    g = np.random.default_rng(seed)
    x = g.standard_normal((N, H, W, Ci)).astype(np.float32)
    w = (g.standard_normal((Co, k, k, Ci)) * np.sqrt(2.0 / (k * k * Ci))).astype(np.float32)
    return x, w


def _bf16_round(a):
    return torch.as_tensor(a).to(torch.bfloat16).to(torch.float32).numpy()


TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ABI = {"fp32": 0, "bf16": 1, "fp16": 2}
TOL = {"fp32": 1e-4, "bf16": 2e-2, "fp16": 3e-3}


def _round(a, dtype):
    return torch.as_tensor(a).to(TDT[dtype]).to(torch.float32).numpy()


def _geom(case):
    N, H, W, Ci, Co, k, s, r, ep = case
    spec = ConvSpec("t", Ci, Co, k, s, r, explicit_pad=ep)
    y = conv_tf(torch.zeros(1, Ci, H, W, dtype=torch.float64),
                torch.zeros(Co, k, k, Ci, dtype=torch.float64), spec)
    return spec, y.shape[2], y.shape[3]


def _ref_conv(x, w, spec):
    xt = torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)
    return conv_tf(xt, torch.as_tensor(w, dtype=torch.float64), spec).permute(0, 2, 3, 1).numpy()


def _ref_dgrad(case, w, g, spec):
    """float64 data gradient [N][H][W][Ci] of conv_tf for output gradient g [N][Ho][Wo][Co]"""
    N, H, W, Ci = case[:4]
    xt = torch.zeros((N, Ci, H, W), dtype=torch.float64, requires_grad=True)
    y = conv_tf(xt, torch.as_tensor(w, dtype=torch.float64), spec)
    y.backward(torch.as_tensor(g, dtype=torch.float64).permute(0, 3, 1, 2))
    return xt.grad.permute(0, 2, 3, 1).numpy()


def _assert_elementwise(dtype, got, ref, absprod, K, dg=None):
    """zero elements past the derived per-element bound (conv_bounds.gemm_bound)"""
    nbad, ratio = violations(dtype, got, ref, absprod, K, dg)
    print(f"per-element: {nbad} of {np.asarray(ref).size} past the bound, max err / bound {ratio:.3f}")
    assert nbad == 0, (nbad, ratio)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_conv_fwd(cuda, dtype, case):
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    x, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    tdt = TDT[dtype]
    if dtype != "fp32":
        x, w = _round(x, dtype), _round(w, dtype)
    ref = _ref_conv(x, w, spec)
    xd = torch.as_tensor(x).to(cuda, tdt).contiguous()
    wd = torch.as_tensor(w).to(cuda, tdt).contiguous()
    # narrow outputs (the logits) live in 16-channel pixels, as the runtime lays them out
    ldy = Co if Co % 8 == 0 else (Co + 15) // 16 * 16
    yd = torch.zeros((N, Ho, Wo, ldy), dtype=tdt, device=cuda)
    M = N * Ho * Wo
    # BN partials: one per stat-rows block of the kernel the dispatcher picks (64 / 128 / 256)
    tr = LIB.seg_op_conv_stat_rows(ABI[dtype], N, H, W, Ci, Ci, Co, Co, k, s, r, int(ep))
    stats = torch.zeros(((M + tr - 1) // tr, Co, 2), dtype=torch.float32, device=cuda)
    s_ = torch.cuda.current_stream().cuda_stream
    check(LIB.seg_op_conv_fwd(ABI[dtype], xd.data_ptr(), N, H, W, Ci, Ci,
                              wd.data_ptr(), Co, k, s, r, int(ep), yd.data_ptr(), ldy,
                              stats.data_ptr(), s_))
    torch.cuda.synchronize()
    y = yd[..., :Co].float().cpu().numpy()
    tol = TOL[dtype]
    assert _rel(y, ref) < tol
    _assert_elementwise(dtype, y, ref, _ref_conv(np.abs(x), np.abs(w), spec), k * k * Ci)
    # BN partial statistics: merge (sum, M2 about the tile mean) and compare
    nt = (M + tr - 1) // tr
    st = stats.cpu().numpy().astype(np.float64)[:nt]
    cnt = np.minimum(tr, M - np.arange(nt) * tr).astype(np.float64)
    mean = st[:, :, 0].sum(0) / M
    tile_mean = st[:, :, 0] / cnt[:, None]
    m2 = st[:, :, 1].sum(0) + (cnt[:, None] * (tile_mean - mean) ** 2).sum(0)
    # fp32: against the stored output; bf16: the statistics are taken from the fp32
    # accumulators (before the bf16 rounding of the stored y), so against the fp64 reference
    # (mean error measured in units of the channel's standard deviation: means are ~0 here)
    yr = (y if dtype == "fp32" else ref).reshape(-1, Co).astype(np.float64)
    sd = np.sqrt(yr.var(0))
    assert np.linalg.norm(mean - yr.mean(0)) / np.linalg.norm(sd) < (1e-5 if dtype == "fp32" else 1e-3)
    assert _rel(m2 / M, yr.var(0)) < 1e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", [c for c in CASES if c[3] != 3])
def test_conv_dgrad(cuda, dtype, case):
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    x, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    g = np.random.default_rng(1).standard_normal((N, Ho, Wo, Co)).astype(np.float32)
    tdt = TDT[dtype]
    if dtype != "fp32":
        w, g = _round(w, dtype), _round(g, dtype)
    xt = torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    y = conv_tf(xt, torch.as_tensor(w, dtype=torch.float64), spec)
    y.backward(torch.as_tensor(g, dtype=torch.float64).permute(0, 3, 1, 2))
    ref = xt.grad.permute(0, 2, 3, 1).numpy()
    wt = np.ascontiguousarray(np.flip(w, (1, 2)).transpose(3, 1, 2, 0))  # [Ci][k][k][Co] flipped
    # narrow gradients (of the logits) come in 16-channel pixels, as the runtime lays them out
    lddy = Co if Co % 8 == 0 else (Co + 15) // 16 * 16
    gp = np.zeros(g.shape[:3] + (lddy,), np.float32)
    gp[..., :Co] = g
    gd = torch.as_tensor(gp).to(cuda, tdt).contiguous()
    wtd = torch.as_tensor(wt).to(cuda, tdt).contiguous()
    dx = torch.zeros((N, H, W, Ci), dtype=tdt, device=cuda)
    check(LIB.seg_op_conv_dgrad(ABI[dtype], gd.data_ptr(), N, Ho, Wo, Co, lddy,
                                wtd.data_ptr(), Ci, k, s, r, int(ep), H, W, dx.data_ptr(), Ci,
                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = dx.float().cpu().numpy()
    assert _rel(got, ref) < TOL[dtype]
    # (a strided data gradient sums fewer than k * k * Co products: K is the kernel's loop length)
    _assert_elementwise(dtype, got, ref, _ref_dgrad(case, np.abs(w), np.abs(g), spec), k * k * Co)


# the identity units' data-gradient epilogue (seg_op_conv_dgrad_res): N, H, W, Co (= the
# forward conv's output channels: dy's), Ci (dx's), with residual, with the consumer's ReLU bits
RES_CASES = [
    (2, 16, 32, 256, 512, True, True),     # persistent residual launch (RQP): residual + mask (4 x 2 tiles)
    (2, 16, 32, 256, 512, True, False),    # residual only
    (1, 20, 20, 128, 256, True, True),     # ragged rows (400 pixels), K 128
    (1, 16, 16, 64, 256, False, True),     # mask only (the premasked dgrad without residual), K 64
    (2, 8, 16, 512, 2048, True, True),     # the block4 shape class: K 512 -> N 2048
    (1, 12, 20, 256, 128, True, False),    # Ci <= 128: the v2 kernel's residual epilogue
    # RQP with more tiles than CUs (506 tiles: blocks run two, the next tile's mask bytes and
    # K-tile 0 issued inside the epilogue), a ragged last row tile; K 192 = 3 K-tiles (odd: the
    # starting buffer alternates tile to tile) and K 256 (even)
    (4, 63, 257, 192, 512, True, True),
    (4, 63, 257, 256, 512, True, True),
    # ragged columns: Ci = 384 / 320 leave the last column tile half / three-quarters empty
    # (RQP reads past the row end into the next row or past the buffer, never stores there),
    # with ragged rows (640 pixels) and 3 K-tiles
    (2, 16, 32, 256, 384, True, True),
    (1, 16, 40, 192, 320, True, True),
    # the consumer's ReLU bits without a residual (one-tile launches), 506 tiles, ragged, K 192
    (4, 63, 257, 192, 512, False, True),
    # RQP without a mask, more tiles than CUs: the wait before residual half 1 is read counts the
    # operations issued after its DMA, and the next tile's 16 mask loads are among them only in a
    # masked launch (conv_pp.hip; vmcnt(32) waited for nothing here before the count followed the
    # mask). A lost race cannot be made to happen on demand, so these cases could not be made to
    # fail deterministically before the fix: the fix rests on the instruction count, the cases pin
    # the branch's values, element by element. Full tiles and a ragged last one, K 192 / 256
    (4, 63, 257, 192, 512, True, False),
    (4, 63, 257, 256, 512, True, False),
]
# fp32 (the generic kernel's residual epilogue): the small residual-only cases
RES_PARAMS = [pytest.param(c, d, id=f"case{i}-{d}") for d in ("bf16", "fp16") for i, c in enumerate(RES_CASES)]
RES_PARAMS += [pytest.param(c, "fp32", id=f"case{i}-fp32") for i, c in enumerate(RES_CASES)
               if c[5] and not c[6] and c[0] * c[1] * c[2] <= 1024]

SENTINEL = -777.0   # exact in bf16 / fp16 / fp32, not zero (masked-off outputs are zeros)


def _rows(cuda, a, ld, tdt, zero_to=0):
    """host [..][C] -> device [M][ld], ld >= C: the columns past C hold NaN (nothing may consume
    them), except a zero channel pad up to zero_to (the runtime's narrow 16-channel pixels)"""
    a = np.asarray(a, np.float32)
    a = a.reshape(-1, a.shape[-1])
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float32)
    buf[:, a.shape[1]:zero_to] = 0.0
    buf[:, :a.shape[1]] = torch.as_tensor(a)
    return buf.to(cuda, tdt).contiguous()


class _Guarded:
    """An [M][C] output inside a sentinel-filled device buffer [M + 2][ld] at channel offset off:
    everything outside [0:M, off:off + C] -- the row tails, the columns before off, the two guard
    rows after row M -- must be bitwise untouched by the launch."""

    def __init__(self, cuda, M, C, ld, tdt, off=0, init=None):
        assert off + C <= ld
        self.M, self.C, self.off = M, C, off
        self.buf = torch.full((M + 2, ld), SENTINEL, dtype=tdt, device=cuda)
        if init is not None:   # (a residual read in place)
            self.buf[:M, off:off + C] = torch.as_tensor(
                np.asarray(init, np.float32).reshape(M, C)).to(cuda, tdt)
        self.before = self.buf.clone()

    @property
    def ld(self):
        return self.buf.shape[1]

    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def result(self, shape):
        return self.buf[:self.M, self.off:self.off + self.C].float().cpu().numpy().reshape(shape)

    def assert_untouched(self, zero_pad_to=0):
        """zero_pad_to: columns [C, zero_pad_to) of the output's rows may have been zero-filled
        instead (the skinny narrow-output kernel completes a pixel's last 4-channel group with
        zeros, inside the runtime's 16-channel pixels: skinny.hip)"""
        ity = torch.int16 if self.buf.element_size() == 2 else torch.int32
        changed = self.buf.view(ity) != self.before.view(ity)
        changed[:self.M, self.off:self.off + self.C] = False
        if zero_pad_to > self.C:
            pad = slice(self.off + self.C, self.off + zero_pad_to)
            changed[:self.M, pad] &= self.buf[:self.M, pad] != 0
        bad = torch.nonzero(changed)
        assert bad.numel() == 0, f"{bad.shape[0]} elements written outside the output, first {bad[0].tolist()}"


def _out_layout(layout, C):
    """(ld, channel offset) of an output of C channels: 'exact' ld == C; 'pad' ld = C + 64;
    'slice' a concat-like slice, C channels at offset 256 of a 1280-wide row"""
    return {"exact": (C, 0), "pad": (C + 64, 0), "slice": (1280, 256)}[layout]


def _dgrad_res_problem(dtype, case):
    N, H, W, Co, Ci, with_r, with_m = case
    g = np.random.default_rng(7)
    dy = _round(g.standard_normal((N, H, W, Co)).astype(np.float32), dtype)
    w = _round((g.standard_normal((Co, Ci)) * np.sqrt(2.0 / Ci)).astype(np.float32), dtype)
    res = _round(g.standard_normal((N, H, W, Ci)).astype(np.float32), dtype) if with_r else None
    bits = g.integers(0, 256, size=(N, H, W, Ci // 8), dtype=np.uint8) if with_m else None
    dg = (dy.reshape(-1, Co).astype(np.float64) @ w.astype(np.float64)).reshape(N, H, W, Ci)
    absprod = (np.abs(dy).reshape(-1, Co).astype(np.float64) @ np.abs(w).astype(np.float64)).reshape(N, H, W, Ci)
    ref = dg
    if with_r:   # the exact sum: one rounding (RQP) and two (v2) are both within the bound
        ref = dg + res
    keep = np.ones((N, H, W, Ci), bool)
    if with_m:
        keep = ((bits[..., :, None] >> np.arange(8)) & 1).astype(bool).reshape(N, H, W, Ci)
    return dy, w, res, bits, dg, absprod, ref, keep


def _run_dgrad_res(cuda, dtype, case, layout):
    """the launches of test_conv_dgrad_residual_masked at an output / operand layout; returns
    the checked outputs (separate residual buffer first, then the residual read in place)"""
    from seg_hip import LIB, check
    N, H, W, Co, Ci, with_r, with_m = case
    M = N * H * W
    dy, w, res, bits, dg, absprod, ref, keep = _dgrad_res_problem(dtype, case)
    tdt = TDT[dtype]
    st = torch.cuda.current_stream().cuda_stream
    exact = layout == "exact"
    lddy = Co if exact else Co + 64
    dyd = _rows(cuda, dy, lddy, tdt)
    wtd = torch.as_tensor(np.ascontiguousarray(w.T)).to(cuda, tdt).contiguous()   # [Ci][Co]
    md = torch.as_tensor(bits).to(cuda).contiguous() if with_m else None
    lddx, off = _out_layout(layout, Ci)
    outs = []
    for alias in ((False, True) if with_r else (False,)):
        if alias:
            dx = _Guarded(cuda, M, Ci, lddx, tdt, off, init=res)
            rptr, ldr = dx.ptr(), lddx
        else:
            dx = _Guarded(cuda, M, Ci, lddx, tdt, off)
            # the residual's row stride differs from the output's unless it is the output
            ldr = Ci if exact else Ci + 128
            rd = _rows(cuda, res, ldr, tdt) if with_r else None
            rptr = rd.data_ptr() if with_r else None
        check(LIB.seg_op_conv_dgrad_res(ABI[dtype], dyd.data_ptr(), N, H, W, Co, lddy, wtd.data_ptr(), Ci,
                                        dx.ptr(), lddx, rptr, ldr,
                                        md.data_ptr() if md is not None else None, st))
        torch.cuda.synchronize()
        dx.assert_untouched()
        outs.append(dx.result((N, H, W, Ci)))
    for got in outs:
        assert np.all(got[~keep] == 0.0)
        assert _rel(got[keep], ref[keep]) < TOL[dtype]
        _assert_elementwise(dtype, got[keep], ref[keep], absprod[keep], Co, dg[keep])
    if len(outs) == 2:
        assert np.array_equal(outs[0], outs[1])
    return outs


@pytest.mark.parametrize("case,dtype", RES_PARAMS)
def test_conv_dgrad_residual_masked(cuda, dtype, case):
    """dx = round(dgrad(dy) + r) (RQP: one rounding; the v2 kernel's epilogue rounds the data
    gradient first), stored with the outputs whose ReLU bit is 0 set to zero (pre-masked identity-unit gradients, staged residuals -- the identity units'
    conv1 data gradient), against a float64 restatement on the same 16-bit operands: kept
    elements at the 16-bit bound of the other op tests (L2-relative) and each within the derived
    per-element bound (conv_bounds), masked-off elements exactly
    zero, the residual read in place (r aliasing dx) bitwise the same as from another buffer.
    fp32 (residual only): the generic kernel's epilogue."""
    _run_dgrad_res(cuda, dtype, case, "exact")


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_conv_wgrad(cuda, dtype, case):
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    # Co % 8 != 0 (the logits convs: 14 / 7 / 3 classes): the runtime pads the gradient's
    # channels and the weight-gradient rows to a multiple of 16 with zeros (net_layers.cpp conv_wgrad,
    # co_pad); the padded rows must come out zero
    co_pad = Co if Co % 8 == 0 else (Co + 15) // 16 * 16
    x, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    g = np.random.default_rng(2).standard_normal((N, Ho, Wo, Co)).astype(np.float32)
    tdt = TDT[dtype]
    if dtype != "fp32":
        x, g = _round(x, dtype), _round(g, dtype)
    wt = torch.as_tensor(w, dtype=torch.float64).requires_grad_(True)
    y = conv_tf(torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), wt, spec)
    y.backward(torch.as_tensor(g, dtype=torch.float64).permute(0, 3, 1, 2))
    ref = wt.grad.numpy()
    xd = torch.as_tensor(x).to(cuda, tdt).contiguous()
    gp = np.zeros((N, Ho, Wo, co_pad), np.float32)
    gp[..., :Co] = g
    gd = torch.as_tensor(gp).to(cuda, tdt).contiguous()
    dw = torch.full((co_pad, k, k, Ci), float("nan"), dtype=torch.float32, device=cuda)
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=cuda)
    check(LIB.seg_op_conv_wgrad(ABI[dtype], gd.data_ptr(), N, Ho, Wo, co_pad, co_pad,
                                xd.data_ptr(), H, W, Ci, Ci, k, s, r, int(ep), dw.data_ptr(),
                                ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    dwh = dw.cpu().numpy()
    assert _rel(dwh[:Co], ref) < TOL[dtype]
    assert np.all(dwh[Co:] == 0.0)


# small-channel 3x3 stride-1 weight gradient on input patches (wgrad_patch.hip): 64-pixel row
# strips, 64-channel co / ci blocks, dilation <= 4, padding rows and columns at every border
WGRAD_PATCH_CASES = [
    (1, 8, 128, 128, 128, 3, 1, 1, False),    # 2 x 2 channel blocks, two strips per row
    (2, 6, 64, 64, 128, 3, 1, 2, False),      # rate 2, Co 128 / Ci 64
    (1, 5, 64, 128, 64, 3, 1, 4, False),      # rate 4 (widest patch), Ci 128 / Co 64
    (3, 1, 192, 64, 64, 3, 1, 1, False),      # one output row per image (all taps padded)
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", WGRAD_PATCH_CASES)
def test_conv_wgrad_patch(cuda, dtype, case):
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    x, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    assert (Ho, Wo) == (H, W) and Wo % 64 == 0
    g = _round(np.random.default_rng(5).standard_normal((N, Ho, Wo, Co)).astype(np.float32), dtype)
    x = _round(x, dtype)
    wt = torch.as_tensor(w, dtype=torch.float64).requires_grad_(True)
    y = conv_tf(torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), wt, spec)
    y.backward(torch.as_tensor(g, dtype=torch.float64).permute(0, 3, 1, 2))
    ref = wt.grad.numpy()
    xd = torch.as_tensor(x).to(cuda, TDT[dtype]).contiguous()
    gd = torch.as_tensor(g).to(cuda, TDT[dtype]).contiguous()
    dw = torch.zeros((Co, k, k, Ci), dtype=torch.float32, device=cuda)
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=cuda)
    check(LIB.seg_op_conv_wgrad(ABI[dtype], gd.data_ptr(), N, Ho, Wo, Co, Co,
                                xd.data_ptr(), H, W, Ci, Ci, k, s, r, int(ep), dw.data_ptr(),
                                ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _rel(dw.cpu().numpy(), ref) < TOL[dtype]


WGRAD_CFG_CASES = [
    # case (N, H, W, Ci, Co, k, stride, rate, explicit_pad), bm, bn, splits
    ((1, 8, 72, 256, 256, 3, 1, 2, False), 256, 256, 3),   # ping-pong, Wo >= 64 (row carries)
    ((2, 13, 17, 128, 256, 3, 1, 2, False), 256, 256, 2),  # ping-pong, Wo < 64, ragged columns
    ((1, 9, 70, 64, 320, 1, 1, 1, False), 256, 256, 4),    # ragged co tile, Ncol < 256
    ((2, 18, 132, 64, 256, 3, 2, 1, True), 256, 256, 5),   # stride-2 conv2d_same gather
    ((1, 6, 66, 256, 256, 3, 1, 4, False), 256, 256, 64),  # splits with no pixels (zero slabs)
    ((2, 13, 17, 128, 256, 3, 1, 2, False), 128, 256, 3),  # v2 configurations
    ((1, 8, 72, 256, 256, 1, 1, 1, False), 64, 128, 2),
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case,bm,bn,splits", WGRAD_CFG_CASES)
def test_conv_wgrad_cfg(cuda, case, bm, bn, splits, dtype):
    """bf16 weight gradient at an explicit tile / split configuration (every kernel the
    runtime can pick, reached at test sizes), vs float64 on the same bf16 operands."""
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    x, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    g = _round(np.random.default_rng(3).standard_normal((N, Ho, Wo, Co)).astype(np.float32), dtype)
    x = _round(x, dtype)
    wt = torch.as_tensor(w, dtype=torch.float64).requires_grad_(True)
    y = conv_tf(torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), wt, spec)
    y.backward(torch.as_tensor(g, dtype=torch.float64).permute(0, 3, 1, 2))
    ref = wt.grad.numpy()
    xd = torch.as_tensor(x).to(cuda, TDT[dtype]).contiguous()
    gd = torch.as_tensor(g).to(cuda, TDT[dtype]).contiguous()
    dw = torch.zeros((Co, k, k, Ci), dtype=torch.float32, device=cuda)
    ws = torch.full((splits * Co * k * k * Ci,), float("nan"), dtype=torch.float32, device=cuda)
    check(LIB.seg_op_conv_wgrad_cfg(ABI[dtype], gd.data_ptr(), N, Ho, Wo, Co, Co, xd.data_ptr(), H, W, Ci,
                                    Ci, k, s, r, int(ep), dw.data_ptr(), ws.data_ptr(),
                                    ws.numel() * 4, bm, bn, splits,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _rel(dw.cpu().numpy(), ref) < TOL[dtype]


# ---- leading dimensions and guard bands -------------------------------------------------
# The runtime's tensors are often slices of wider rows (the pyramid concat: ld = 5 x
# feature_dims). Every operand here has ld > its channel count (inputs C + 64, the tail NaN;
# outputs Co + 64, or Co = 256 at channel offset 256 of a 1280-wide row), two guard rows follow
# row M of every output, and the outputs are prefilled with a sentinel: a store past Co or past
# row M, invisible with exactly sized ld == C buffers, changes a guard element.
LD_CASES = [
    # N, H, W, Ci, Co, k, stride, rate, explicit_pad
    (2, 16, 32, 256, 384, 1, 1, 1, False),    # ragged columns (its dgrad: Co 256)
    (1, 16, 40, 192, 320, 1, 1, 1, False),    # ragged columns and rows, 3 K-tiles
    (1, 20, 20, 128, 256, 1, 1, 1, False),    # ragged second wave row
    (2, 13, 17, 64, 64, 3, 1, 2, False),      # dilated 3x3, v2 64-channel tile
    (2, 16, 20, 128, 256, 3, 1, 4, False),    # rate 4, ping-pong ST = 1
    (2, 9, 10, 256, 14, 1, 1, 1, False),      # skinny
]


def _ld_params(out_channels):
    """(case, layout): 'pad' for every case, 'slice' where the output has 256 channels"""
    return [(c, "pad") for c in LD_CASES] + [(c, "slice") for c in LD_CASES if out_channels(c) == 256]


def _pad16(C):   # narrow tensors (the logits and their gradients) live in 16-channel pixels
    return C if C % 8 == 0 else (C + 15) // 16 * 16


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case,layout", _ld_params(lambda c: c[4]))
def test_conv_fwd_ld(cuda, dtype, case, layout):
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    x, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    tdt = TDT[dtype]
    if dtype != "fp32":
        x, w = _round(x, dtype), _round(w, dtype)
    ref = _ref_conv(x, w, spec)
    xd = _rows(cuda, x, Ci + 64, tdt)
    wd = torch.as_tensor(w).to(cuda, tdt).contiguous()
    M = N * Ho * Wo
    ldy, off = _out_layout(layout, _pad16(Co))
    yd = _Guarded(cuda, M, Co, ldy, tdt, off)
    check(LIB.seg_op_conv_fwd(ABI[dtype], xd.data_ptr(), N, H, W, Ci, Ci + 64,
                              wd.data_ptr(), Co, k, s, r, int(ep), yd.ptr(), ldy,
                              None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    yd.assert_untouched(zero_pad_to=(Co + 3) // 4 * 4)
    y = yd.result(ref.shape)
    assert _rel(y, ref) < TOL[dtype]
    _assert_elementwise(dtype, y, ref, _ref_conv(np.abs(x), np.abs(w), spec), k * k * Ci)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case,layout", _ld_params(lambda c: c[3]))
def test_conv_dgrad_ld(cuda, dtype, case, layout):
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    _, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    g = np.random.default_rng(1).standard_normal((N, Ho, Wo, Co)).astype(np.float32)
    tdt = TDT[dtype]
    if dtype != "fp32":
        w, g = _round(w, dtype), _round(g, dtype)
    ref = _ref_dgrad(case, w, g, spec)
    wt = np.ascontiguousarray(np.flip(w, (1, 2)).transpose(3, 1, 2, 0))  # [Ci][k][k][Co] flipped
    lddy = _pad16(Co) + 64
    gd = _rows(cuda, g, lddy, tdt, zero_to=_pad16(Co))
    wtd = torch.as_tensor(wt).to(cuda, tdt).contiguous()
    lddx, off = _out_layout(layout, Ci)
    dx = _Guarded(cuda, N * H * W, Ci, lddx, tdt, off)
    check(LIB.seg_op_conv_dgrad(ABI[dtype], gd.data_ptr(), N, Ho, Wo, Co, lddy,
                                wtd.data_ptr(), Ci, k, s, r, int(ep), H, W, dx.ptr(), lddx,
                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    dx.assert_untouched()
    got = dx.result(ref.shape)
    assert _rel(got, ref) < TOL[dtype]
    _assert_elementwise(dtype, got, ref, _ref_dgrad(case, np.abs(w), np.abs(g), spec), k * k * Co)


# N, H, W, Co (dy's), Ci (dx's), with residual, with mask: the dense 1 x 1 shapes of LD_CASES
LD_RES_CASES = [
    (2, 16, 32, 256, 384, True, True),
    (1, 16, 40, 192, 320, True, True),     # ragged columns under RQP
    (1, 16, 40, 192, 320, True, False),
    (1, 20, 20, 128, 256, True, True),
    (1, 20, 20, 128, 256, False, True),
    (1, 12, 20, 256, 128, True, False),    # the v2 kernel's residual epilogue
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case,layout", [(c, "pad") for c in LD_RES_CASES] +
                         [(c, "slice") for c in LD_RES_CASES if c[4] == 256])
def test_conv_dgrad_residual_masked_ld(cuda, dtype, case, layout):
    """test_conv_dgrad_residual_masked with every ld > the channel count (the residual's differs
    from the output's except where it is the output) and guard bands round the output"""
    _run_dgrad_res(cuda, dtype, case, layout)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_conv_dgrad_residual_unaligned_ldr(cuda, dtype):
    """A residual whose row stride is no multiple of 8 elements (ldr = Ci + 4): the 16-byte
    residual reads of the v2 / ping-pong epilogues and the 16-byte LDS-DMA pieces of RQP would
    read shifted rows. The kernel selection (csrc/conv_select.cpp) turns such a launch away from
    every 16-bit tile kernel (it runs on the generic one), so the result is correct per the
    bound; a negative errno would be acceptable too -- shifted data never."""
    from seg_hip import LIB
    case = (2, 16, 32, 256, 512, True, False)
    N, H, W, Co, Ci, _, _ = case
    M = N * H * W
    dy, w, res, _, dg, absprod, ref, _ = _dgrad_res_problem(dtype, case)
    tdt = TDT[dtype]
    dyd = _rows(cuda, dy, Co, tdt)
    wtd = torch.as_tensor(np.ascontiguousarray(w.T)).to(cuda, tdt).contiguous()
    rd = _rows(cuda, res, Ci + 4, tdt)
    dx = _Guarded(cuda, M, Ci, Ci, tdt)
    rc = LIB.seg_op_conv_dgrad_res(ABI[dtype], dyd.data_ptr(), N, H, W, Co, Co, wtd.data_ptr(), Ci,
                                   dx.ptr(), Ci, rd.data_ptr(), Ci + 4, None,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dx.assert_untouched()
    if rc == 0:
        got = dx.result(ref.shape)
        assert _rel(got, ref) < TOL[dtype]
        _assert_elementwise(dtype, got, ref, absprod, Co, dg)
    else:
        assert rc < 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", LD_CASES)
def test_conv_wgrad_ld(cuda, dtype, case):
    """weight gradient with padded operand rows (x: Ci + 64, dy: Co + 64); dw is dense
    [Co][k][k][Ci] fp32, followed here by two guard rows"""
    from seg_hip import LIB, check
    N, H, W, Ci, Co, k, s, r, ep = case
    co_pad = _pad16(Co)
    x, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    g = np.random.default_rng(2).standard_normal((N, Ho, Wo, Co)).astype(np.float32)
    tdt = TDT[dtype]
    if dtype != "fp32":
        x, g = _round(x, dtype), _round(g, dtype)
    wt = torch.as_tensor(w, dtype=torch.float64).requires_grad_(True)
    y = conv_tf(torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), wt, spec)
    y.backward(torch.as_tensor(g, dtype=torch.float64).permute(0, 3, 1, 2))
    ref = wt.grad.numpy()
    xd = _rows(cuda, x, Ci + 64, tdt)
    gd = _rows(cuda, g, co_pad + 64, tdt, zero_to=co_pad)
    dw = _Guarded(cuda, co_pad, k * k * Ci, k * k * Ci, torch.float32)
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=cuda)
    check(LIB.seg_op_conv_wgrad(ABI[dtype], gd.data_ptr(), N, Ho, Wo, co_pad, co_pad + 64,
                                xd.data_ptr(), H, W, Ci, Ci + 64, k, s, r, int(ep), dw.ptr(),
                                ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    dw.assert_untouched()
    dwh = dw.result((co_pad, k, k, Ci))
    assert _rel(dwh[:Co], ref) < TOL[dtype]
    assert np.all(dwh[Co:] == 0.0)


# ---- the fused data-gradient variants the runtime launches (seg_op_conv_dgrad_fused) -----
def _keep_of(bits, shape):
    return ((bits[..., :, None] >> np.arange(8)) & 1).astype(bool).reshape(shape)


def _assert_fused(dtype, got, ref, absprod, K, dg, keep):
    assert np.all(got[~keep] == 0.0)
    assert _rel(got[keep], ref[keep]) < TOL[dtype]
    _assert_elementwise(dtype, got[keep], ref[keep], absprod[keep], K, dg[keep])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,with_m", [((2, 16, 32, 256, 512), False), ((2, 16, 32, 256, 512), True),
                                          ((4, 63, 257, 192, 512), False)])
def test_conv_dgrad_two_residuals_aliased(cuda, dtype, shape, with_m):
    """dx = dgrad(dy) + r1 + r2 with r1 read in place (r1 aliasing dx): the identity units'
    conv1 data gradient into a gradient that already holds the shortcut's
    (conv_dgrad(S, u.c1, dx, &dx, &dres)); one tile per workgroup on the ping-pong kernel, the
    residuals read in the staged layout. Bitwise the same as with r1 in a buffer of its own."""
    from seg_hip import LIB, check
    N, H, W, Co, Ci = shape
    M = N * H * W
    g = np.random.default_rng(17)
    dy = _round(g.standard_normal((M, Co)).astype(np.float32), dtype)
    w = _round((g.standard_normal((Co, Ci)) * np.sqrt(2.0 / Ci)).astype(np.float32), dtype)
    r1 = _round(g.standard_normal((M, Ci)).astype(np.float32), dtype)
    r2 = _round(g.standard_normal((M, Ci)).astype(np.float32), dtype)
    bits = g.integers(0, 256, size=(M, Ci // 8), dtype=np.uint8) if with_m else None
    keep = _keep_of(bits, (M, Ci)) if with_m else np.ones((M, Ci), bool)
    dg = dy.astype(np.float64) @ w.astype(np.float64)
    absprod = np.abs(dy).astype(np.float64) @ np.abs(w).astype(np.float64)
    ref = dg + r1 + r2
    tdt = TDT[dtype]
    dyd = _rows(cuda, dy, Co, tdt)
    wtd = torch.as_tensor(np.ascontiguousarray(w.T)).to(cuda, tdt).contiguous()   # [Ci][Co]
    r2d = _rows(cuda, r2, Ci, tdt)
    md = torch.as_tensor(bits).to(cuda).contiguous() if with_m else None
    outs = []
    for alias in (False, True):
        dx = _Guarded(cuda, M, Ci, Ci, tdt, init=r1 if alias else None)
        r1d = None if alias else _rows(cuda, r1, Ci, tdt)
        check(LIB.seg_op_conv_dgrad_fused(ABI[dtype], dyd.data_ptr(), N, H, W, Co, Co, wtd.data_ptr(), Ci,
                                          1, 1, dx.ptr(), Ci, dx.ptr() if alias else r1d.data_ptr(), Ci,
                                          r2d.data_ptr(), Ci, None, 0, 0, None,
                                          md.data_ptr() if with_m else None,
                                          torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        dx.assert_untouched()
        outs.append(dx.result((M, Ci)))
        _assert_fused(dtype, outs[-1], ref, absprod, Co, dg, keep)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("Ci,with_m", [(512, False), (512, True), (128, False)])
def test_conv_dgrad_dual(cuda, dtype, Ci, with_m):
    """dx = dy . wt + dy2 . wt2 in one K-concatenated launch (a projection unit's conv1 and
    shortcut data gradients; the folded conv3 launches): Ci 512 on the ping-pong kernel (ST = 4),
    with and without the consumer's ReLU bits, Ci 128 on the v2 kernel (no masked launch exists
    there: the plan of such a request is invalid, csrc/conv_select.cpp); 630 pixels: two full
    row tiles and a ragged one; dy and dy2 with different row strides."""
    from seg_hip import LIB, check
    N, H, W, Co, Co2 = 2, 15, 21, 256, 256
    M = N * H * W
    g = np.random.default_rng(23)
    dy = _round(g.standard_normal((M, Co)).astype(np.float32), dtype)
    dy2 = _round(g.standard_normal((M, Co2)).astype(np.float32), dtype)
    w = _round((g.standard_normal((Co, Ci)) * np.sqrt(1.0 / Co)).astype(np.float32), dtype)
    w2 = _round((g.standard_normal((Co2, Ci)) * np.sqrt(1.0 / Co2)).astype(np.float32), dtype)
    bits = g.integers(0, 256, size=(M, Ci // 8), dtype=np.uint8) if with_m else None
    keep = _keep_of(bits, (M, Ci)) if with_m else np.ones((M, Ci), bool)
    f = lambda a: np.asarray(a, np.float64)
    ref = f(dy) @ f(w) + f(dy2) @ f(w2)
    absprod = np.abs(f(dy)) @ np.abs(f(w)) + np.abs(f(dy2)) @ np.abs(f(w2))
    tdt = TDT[dtype]
    dyd, dy2d = _rows(cuda, dy, Co, tdt), _rows(cuda, dy2, Co2 + 64, tdt)
    wtd = torch.as_tensor(np.ascontiguousarray(w.T)).to(cuda, tdt).contiguous()
    wt2d = torch.as_tensor(np.ascontiguousarray(w2.T)).to(cuda, tdt).contiguous()
    md = torch.as_tensor(bits).to(cuda).contiguous() if with_m else None
    dx = _Guarded(cuda, M, Ci, Ci + 64, tdt)
    check(LIB.seg_op_conv_dgrad_fused(ABI[dtype], dyd.data_ptr(), N, H, W, Co, Co, wtd.data_ptr(), Ci,
                                      1, 1, dx.ptr(), Ci + 64, None, 0, None, 0,
                                      dy2d.data_ptr(), Co2, Co2 + 64, wt2d.data_ptr(),
                                      md.data_ptr() if with_m else None,
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    dx.assert_untouched()
    _assert_fused(dtype, dx.result((M, Ci)), ref, absprod, Co + Co2, ref, keep)


def test_conv_dgrad_fused_rejects_what_the_runtime_never_launches(cuda):
    from seg_hip import LIB
    import errno
    t = torch.zeros(1 << 16, dtype=torch.bfloat16, device=cuda)
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream

    def call(dtype=1, k=1, rate=1, Ci=256, r1=None, r2=None, dy2=None, wt2=None, omask=None):
        return LIB.seg_op_conv_dgrad_fused(dtype, p, 1, 4, 4, 64, 64, p, Ci, k, rate, p, Ci, r1, Ci, r2, Ci,
                                           dy2, 64, 64, wt2, omask, st)
    assert call(dy2=p, wt2=p, r1=p) == -errno.EINVAL     # a dual GEMM with a residual
    assert call(dy2=p, wt2=p, k=3) == -errno.EINVAL      # a dual 3 x 3
    assert call(dy2=p, wt2=p, dtype=0) == -errno.EINVAL  # a dual fp32
    assert call(dy2=p) == -errno.EINVAL                  # dy2 without weights
    assert call(r2=p) == -errno.EINVAL                   # a second residual without a first
    assert call(k=5) == -errno.EINVAL
    assert call(k=1, rate=2) == -errno.EINVAL
    assert call(Ci=128, omask=p) == -errno.EINVAL        # no masked launch at Ci <= 128
    assert call(k=3, omask=p) == -errno.EINVAL           # nor for a 3 x 3
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_conv_dgrad_dilated_residual_in_place(cuda, dtype):
    """A 3 x 3 rate-6 data gradient, 256 -> 256, added in place to the gradient its output
    already holds (r1 aliasing dx): the ASPP branches' accumulation into the pyramid input's
    gradient. 960 pixels; bitwise the same as with the residual in a buffer of its own."""
    from seg_hip import LIB, check
    case = (1, 24, 40, 256, 256, 3, 1, 6, False)
    N, H, W, Ci, Co, k, s, r, ep = case
    M = N * H * W
    _, w = _tensors(case)
    spec, Ho, Wo = _geom(case)
    assert (Ho, Wo) == (H, W)
    g = np.random.default_rng(29)
    dy = _round(g.standard_normal((N, H, W, Co)).astype(np.float32), dtype)
    res = _round(g.standard_normal((N, H, W, Ci)).astype(np.float32), dtype)
    w = _round(w, dtype)
    dg = _ref_dgrad(case, w, dy, spec)
    absprod = _ref_dgrad(case, np.abs(w), np.abs(dy), spec)
    ref = dg + res
    wt = np.ascontiguousarray(np.flip(w, (1, 2)).transpose(3, 1, 2, 0))  # [Ci][k][k][Co] flipped
    tdt = TDT[dtype]
    dyd = _rows(cuda, dy, Co, tdt)
    wtd = torch.as_tensor(wt).to(cuda, tdt).contiguous()
    outs = []
    for alias in (False, True):
        dx = _Guarded(cuda, M, Ci, Ci, tdt, init=res if alias else None)
        rd = None if alias else _rows(cuda, res, Ci, tdt)
        check(LIB.seg_op_conv_dgrad_fused(ABI[dtype], dyd.data_ptr(), N, H, W, Co, Co, wtd.data_ptr(), Ci,
                                          k, r, dx.ptr(), Ci, dx.ptr() if alias else rd.data_ptr(), Ci,
                                          None, 0, None, 0, 0, None, None,
                                          torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        dx.assert_untouched()
        outs.append(dx.result(ref.shape))
        _assert_fused(dtype, outs[-1], ref, absprod, k * k * Co, dg, np.ones(ref.shape, bool))
    assert np.array_equal(outs[0], outs[1])
