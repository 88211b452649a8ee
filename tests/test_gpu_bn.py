"""The batch-norm kernels (csrc/bn.hip) one launch at a time through the seg_op_bn_* entries,
each against the float64 reference of tests/bn_refs.py on exactly what the kernel read, per
element with zero violations (the bounds and their derivation: bn_refs.py; that the checkers
discriminate: test_bn_refs.py). Inputs are well conditioned: y ~ N(m_c, s_c), dz ~ N(0.1, 1),
mean / invstd from the float64 moments of y; the gate bits of the backward are the ones the native
apply of the same case wrote. Every reduce + finalize runs twice and must repeat bit for bit.
Each line "MARGIN op dtype check ratio" is a worst err / bound (profiles/bn_op_margins.txt)."""
import ctypes
import errno

import numpy as np
import pytest
import torch

import bn_refs as R

pytestmark = pytest.mark.gpu

ABI = {"fp32": 0, "bf16": 1, "fp16": 2}
ESZ = {"fp32": 4, "bf16": 2, "fp16": 2}
POISON = 0x7F   # every byte: a NaN in bf16 / fp16 / fp32, and a mask byte no apply writes by chance


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """device buffers of one case (kept alive), with the address arithmetic of strided views"""

    def __init__(self, cuda):
        self.cuda, self.keep = cuda, []

    def put(self, a, dtype="fp32", ld=None, off=0):
        """float32 values [M][C] stored as `dtype` in rows of ld elements at column off (the rest
        poisoned). Returns (address of element [0][off], backing tensor)."""
        a = np.asarray(a, np.float32)
        if a.ndim == 1 or ld is None:
            t = torch.from_numpy(np.ascontiguousarray(a)).to(self.cuda, R.TDT[dtype])
            self.keep.append(t)
            return t.data_ptr(), t
        M, C = a.shape
        t = self.poisoned((M, ld), dtype)
        t[:, off:off + C] = torch.from_numpy(a).to(self.cuda, R.TDT[dtype])
        return t.data_ptr() + off * ESZ[dtype], t

    def poisoned(self, shape, dtype="fp32"):
        n = int(np.prod(shape)) * (1 if dtype == "u8" else ESZ[dtype])
        raw = torch.full((max(n, 1),), POISON, dtype=torch.uint8, device=self.cuda)
        t = raw[:n].view(torch.uint8 if dtype == "u8" else R.TDT[dtype]).reshape(shape)
        self.keep.append(raw)
        return t


def _host(t):
    return t.float().cpu().numpy() if t.dtype != torch.uint8 else t.cpu().numpy()


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == POISON).all())


def _record(op, dtype, res):
    for name, (nbad, ratio) in res.items():
        print(f"MARGIN {op} {dtype} {name} {ratio:.4f}")
    bad = {k: v for k, v in res.items() if v[0] and not k.startswith("k_")}
    assert not bad, (op, dtype, bad)


# ---- forward apply --------------------------------------------------------------------------
def _apply(cuda, dtype, a, M, C, relu, out_f32, mode="none", want_bits=False, ld=None, off=0,
           sub=None, other=None, res_vals=None):
    """one seg_op_bn_apply; returns (rc, out float32 [M][C], bits or None, out tensor, mask tensor)"""
    from seg_hip import LIB, BnApplyArgs
    d = Dev(cuda)
    out_dtype = "fp32" if out_f32 else dtype
    ldv = ld or C
    args = BnApplyArgs()
    args.y, _ = d.put(a["y"], dtype, ld, off)
    args.ldy, args.M, args.C, args.relu = ldv, M, C, int(relu)
    args.mean, _ = d.put(a["mean"])
    args.scale, _ = d.put(a["scale"])
    args.beta, _ = d.put(a["beta"])
    if mode == "plain":
        args.res, _ = d.put(a["r"], dtype, ld, 0)
        args.ldres, args.rs = ldv, 1
    elif mode == "sub":
        rs, Ho, Wo, Hr, Wr = sub
        args.res, _ = d.put(res_vals, dtype)
        args.ldres, args.rs, args.Ho, args.Wo, args.Hr, args.Wr = C, rs, Ho, Wo, Hr, Wr
    elif mode == "bn2":
        args.y2, _ = d.put(other["y"], dtype)
        args.ldy2 = C
        args.mean2, _ = d.put(other["mean"])
        args.scale2, _ = d.put(other["scale"])
        args.beta2, _ = d.put(other["beta"])
    out = d.poisoned((M, ldv), out_dtype)
    args.out, args.ldo = out.data_ptr() + off * ESZ[out_dtype], ldv
    mask = d.poisoned((M, max(C // 8, 1)), "u8") if want_bits else None
    args.mask = mask.data_ptr() if want_bits else None
    rc = LIB.seg_op_bn_apply(ABI[dtype], int(out_f32), ctypes.byref(args), _stream())
    torch.cuda.synchronize()
    got = _host(out)
    if ld:   # nothing outside the layer's columns is written
        keep = torch.ones(ldv, dtype=torch.bool)
        keep[off:off + C] = False
        assert _untouched(out[:, keep.to(out.device)])
    return rc, got[:, off:off + C], (_host(mask) if want_bits else None), out, mask


def _apply_kw(a, mode, sub=None, other=None, res_vals=None):
    if mode == "plain":
        return dict(res=a["r"])
    if mode == "sub":
        return dict(res=res_vals, sub=sub)
    if mode == "bn2":
        return dict(y2=other["y"], bn2=(other["mean"], other["scale"], other["beta"]))
    return {}


SUBS = [(2, 5, 7, 9, 13), (2, 5, 7, 10, 14)]   # rs, Ho, Wo, Hr, Wr at N = 2: odd and even grids


@pytest.mark.parametrize("out_f32", [False, True], ids=["out16", "out32"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("mode", ["none", "plain", "sub", "bn2"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_apply_variants(cuda, dtype, mode, relu, out_f32):
    """every residual mode x ReLU x output type, with and without the bits"""
    C = 128
    M = 70 if mode == "sub" else 391
    a = R.layer_inputs(M, C, dtype, seed=11)
    other = R.layer_inputs(M, C, dtype, seed=12)
    if dtype == "fp32" and not out_f32:   # no fp32 -> 16-bit instantiation: refused, nothing written
        rc, _, _, out, _ = _apply(cuda, dtype, a, M, C, relu, out_f32)
        assert rc == -errno.EINVAL and _untouched(out)
        return
    out_dtype = "fp32" if out_f32 else dtype
    for sub in (SUBS if mode == "sub" else [None]):
        res_vals = None
        if sub:
            g = np.random.default_rng(13)
            res_vals = R.round_to(g.standard_normal((2 * sub[3] * sub[4], C)).astype(np.float32), dtype)
        kw = _apply_kw(a, mode, sub, other, res_vals)
        ref, bound = R.apply_ref(a["y"], a["mean"], a["scale"], a["beta"], relu, out_dtype, **kw)
        rc, got, bits, _, _ = _apply(cuda, dtype, a, M, C, relu, out_f32, mode, want_bits=relu, sub=sub,
                                     other=other, res_vals=res_vals)
        assert rc == 0
        _record(f"apply_{mode}", f"{dtype}>{out_dtype}", R.apply_check(got, bits, ref, bound))
        if relu:   # the same launch without the bits stores the same output
            rc, got2, _, _, _ = _apply(cuda, dtype, a, M, C, relu, out_f32, mode, sub=sub, other=other,
                                       res_vals=res_vals)
            assert rc == 0 and np.array_equal(got, got2)


# M, C and the reason each size is there
SIZES = [
    (1, 256),      # PSP grid-1, one image
    (4, 256),      # ASPP image pool
    (65, 64),      # rb 2, 33 + 32 rows, 32 row lanes, guarded tail groups only
    (391, 128),    # ragged full and tail groups
    (1000, 24),    # C/8 = 3: 85 row lanes, one idle thread
    (777, 320),    # C/8 = 40: 16 idle threads
    (300, 2048),   # C/8 = 256: the >= / > boundary in row_lane, grid8 and the launchers
    (130, 2056),   # C/8 = 257: blockIdx.y = 1 with one active lane
]
BIG_APPLY = (8200, 2048)    # past grid8's 2,048 x 4 rows: the grid-stride pass runs (16-bit only)
BIG_REDUCE = (66000, 64)    # the 1,024 row-block cap with rows_per = 65
NARROW = [(333, 14), (333, 7), (333, 3)]   # ld = 16: the scalar kernels and their 32-bit index path
ALL = ["bf16", "fp16", "fp32"]
APPLY_CASES = [(t, M, C) for t in ALL for M, C in SIZES] + [(t,) + BIG_APPLY for t in ALL[:2]]
BWD_CASES = APPLY_CASES + [(t,) + BIG_REDUCE for t in ALL]


@pytest.mark.parametrize("dtype,M,C", APPLY_CASES)
def test_apply_sizes(cuda, dtype, M, C):
    """BN + plain residual + ReLU with bits at every size that takes another path"""
    a = R.layer_inputs(M, C, dtype, seed=M + C)
    out_f32 = dtype == "fp32"
    ref, bound = R.apply_ref(a["y"], a["mean"], a["scale"], a["beta"], True, dtype, res=a["r"])
    rc, got, bits, _, _ = _apply(cuda, dtype, a, M, C, True, out_f32, "plain", want_bits=True)
    assert rc == 0
    _record("apply_sizes", dtype, R.apply_check(got, bits, ref, bound))


@pytest.mark.parametrize("out_f32", [False, True], ids=["out16", "out32"])
@pytest.mark.parametrize("M,C", NARROW)
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_apply_narrow(cuda, dtype, M, C, out_f32):
    """the logits layers: C = 14 / 7 / 3 in 16-channel pixels, the scalar kernel; bits refused"""
    a = R.layer_inputs(M, C, dtype, seed=M + C)
    if dtype == "fp32" and not out_f32:
        rc, _, _, out, _ = _apply(cuda, dtype, a, M, C, True, out_f32, ld=16)
        assert rc == -errno.EINVAL and _untouched(out)
        return
    out_dtype = "fp32" if out_f32 else dtype
    for mode in ("none", "plain"):
        ref, bound = R.apply_ref(a["y"], a["mean"], a["scale"], a["beta"], True, out_dtype, **_apply_kw(a, mode))
        rc, got, _, _, _ = _apply(cuda, dtype, a, M, C, True, out_f32, mode, ld=16)
        assert rc == 0
        _record("apply_narrow", f"{dtype}>{out_dtype}", R.apply_check(got, None, ref, bound))
    from seg_hip import LIB
    rc, _, _, out, mask = _apply(cuda, dtype, a, M, C, True, out_f32, want_bits=True, ld=16)
    assert rc == -errno.EINVAL and b"8-wide" in LIB.seg_last_error(None)
    assert _untouched(out) and _untouched(mask)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_apply_in_a_concat(cuda, dtype):
    """y and the output as 256 channels at offset 256 of a 1,280-wide concat"""
    M, C = 391, 256
    a = R.layer_inputs(M, C, dtype, seed=21)
    ref, bound = R.apply_ref(a["y"], a["mean"], a["scale"], a["beta"], True, dtype)
    rc, got, bits, _, _ = _apply(cuda, dtype, a, M, C, True, dtype == "fp32", want_bits=True, ld=1280, off=256)
    assert rc == 0
    _record("apply_concat", dtype, R.apply_check(got, bits, ref, bound))


# ---- backward -------------------------------------------------------------------------------
def _native_bits(cuda, dtype, a, M, C):
    """the ReLU bits the native apply of this case writes (BN + residual r + ReLU)"""
    rc, _, bits, _, _ = _apply(cuda, dtype, a, M, C, True, dtype == "fp32", "plain", want_bits=True)
    assert rc == 0
    return bits


class Bwd:
    """one layer's device buffers and seg_bn_bwd_args"""

    def __init__(self, cuda, dtype, a, M, C, kw, dz_f32=False, want_dy=True, want_dyhat=False,
                 want_cs=False, ld=None, lddz=None, dzoff=0, ldy=None, grads=True):
        from seg_hip import LIB, BnBwdArgs
        self.d = d = Dev(cuda)
        self.dtype, self.M, self.C, self.ld = dtype, M, C, ld or C
        zt = "fp32" if dz_f32 else dtype
        self.rb = LIB.seg_op_bn_rowblocks(M, C)
        assert self.rb == R.bn_rowblocks(M)
        g = self.args = BnBwdArgs()
        g.dz, _ = d.put(a["dz"], zt, lddz, dzoff)
        g.lddz = lddz or C
        if kw.get("z") is not None:
            g.z, _ = d.put(kw["z"], zt)
            g.ldz = C
        if kw.get("mask") is not None:
            t = torch.from_numpy(np.ascontiguousarray(kw["mask"])).to(cuda)
            d.keep.append(t)
            g.mask = t.data_ptr()
        g.y, _ = d.put(a["y"], dtype, ldy)
        g.ldy, g.M, g.C = ldy or C, M, C
        g.mean, _ = d.put(a["mean"])
        g.invstd, _ = d.put(a["invstd"])
        g.scale, _ = d.put(a["scale"])
        self.sdy, self.sdyx = d.poisoned((C,)), d.poisoned((C,))
        g.sdy, g.sdyx = self.sdy.data_ptr(), self.sdyx.data_ptr()
        self.dy = d.poisoned((M, self.ld), dtype) if want_dy else None
        if want_dy:
            g.dy, g.lddy = self.dy.data_ptr(), self.ld
        self.dyhat = d.poisoned((M, C), dtype) if want_dyhat else None
        if want_dyhat:
            g.dyhat, g.lddyhat = self.dyhat.data_ptr(), C
        for name in ("dzscale", "dshift"):
            if kw.get(name) is not None:
                setattr(g, name, d.put(kw[name])[0])
        if kw.get("beta") is not None:
            g.beta, _ = d.put(kw["beta"])
        self.cs = d.poisoned((self.rb, C)) if want_cs else None
        if want_cs:
            g.cs_part = self.cs.data_ptr()
        self.part = d.poisoned((self.rb, C, 2))
        g.part = self.part.data_ptr()
        self.dgamma = d.poisoned((C,)) if grads else None
        self.dbeta = d.poisoned((C,)) if grads else None
        if grads:
            g.dgamma, g.dbeta = self.dgamma.data_ptr(), self.dbeta.data_ptr()

    def outputs(self):
        return [t for t in (self.sdy, self.sdyx, self.dy, self.dyhat, self.cs, self.part, self.dgamma,
                            self.dbeta) if t is not None]

    def sums(self):
        out = {"sdy": _host(self.sdy), "sdyx": _host(self.sdyx), "part": _host(self.part)}
        if self.dgamma is not None:
            out.update(dgamma=_host(self.dgamma), dbeta=_host(self.dbeta))
        if self.cs is not None:
            out["cs_part"] = _host(self.cs)
        return out


def _run_bwd(b, dz_f32=False, frozen=False, reduce_only=False):
    from seg_hip import LIB
    rc = LIB.seg_op_bn_backward(ABI[b.dtype], int(dz_f32), int(frozen), int(reduce_only),
                                ctypes.byref(b.args), _stream())
    torch.cuda.synchronize()
    return rc


def _bitwise_equal(x, y):
    return all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in x)


def _check_layer(op, b, a, kw, frozen=False, reduce_only=False):
    """sums, stored dyhat and dy of one native backward against float64"""
    ref = R.bwd_ref(a["dz"], a["y"], a["mean"], a["invstd"], b.dtype, scale=a["scale"], **kw)
    got = b.sums()
    res = R.bwd_sums_check(got, ref, frozen)
    if b.dyhat is not None:
        res.update(R.dyhat_check(_host(b.dyhat), ref))
    if not reduce_only:
        dy = _host(b.dy)
        if b.ld != b.C:
            assert _untouched(b.dy[:, b.C:])
        res.update(R.dy_check(dy[:, :b.C], ref, a["scale"], got["sdy"], got["sdyx"], b.dtype)[0])
    _record(op, b.dtype, res)
    return got


def _variant_kw(cuda, dtype, a, M, C, variant):
    g = np.random.default_rng(31)
    kw = {}
    if "z" in variant:
        kw["z"] = a["r"]
    if "bits" in variant:
        kw["mask"] = _native_bits(cuda, dtype, a, M, C)
    if "dzscale" in variant:
        kw["dzscale"] = g.uniform(0.5, 1.5, C).astype(np.float32)
    if "dshift" in variant:
        kw["dshift"] = g.uniform(-0.2, 0.2, C).astype(np.float32)
    if "cs" in variant:
        kw["beta"] = a["beta"]
    return kw


# one case per row of the plan table (batch norm; bits + dzscale, with and without
# dyhat: test_group_norm_apply_gate): (id, variant, dyhat, reduce_only, frozen)
BRANCHES = [
    ("ungated", (), False, False, False),
    ("z", ("z",), False, False, False),
    ("bits", ("bits",), False, False, False),
    ("dzscale", ("dzscale",), False, False, False),
    ("z+dzscale", ("z", "dzscale"), False, False, False),
    ("bits+dshift", ("bits", "dshift"), False, False, False),
    ("bits+dshift+dyhat,reduce_only", ("bits", "dshift"), True, True, False),
    ("bits+dshift+cs,reduce_only", ("bits", "dshift", "cs"), False, True, False),
    ("bits+dyhat,reduce_only", ("bits",), True, True, False),
    ("dyhat", (), True, False, False),
    ("z+dyhat", ("z",), True, False, False),
    ("bits+dyhat", ("bits",), True, False, False),
    ("z+dzscale+dyhat", ("z", "dzscale"), True, False, False),
    ("dzscale+dyhat", ("dzscale",), True, False, False),
    ("frozen", ("bits",), False, False, True),
]


@pytest.mark.parametrize("branch", BRANCHES, ids=[b[0] for b in BRANCHES])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_backward_branches(cuda, dtype, branch):
    name, variant, dyhat, reduce_only, frozen = branch
    M, C = 391, 128
    a = R.layer_inputs(M, C, dtype, seed=41)
    kw = _variant_kw(cuda, dtype, a, M, C, variant)
    cs = "cs" in variant

    def build():
        return Bwd(cuda, dtype, a, M, C, kw, want_dy=not reduce_only, want_dyhat=dyhat, want_cs=cs)

    b = build()
    if cs and dtype == "fp32":   # no fp32 instantiation of the column sums: refused, nothing written
        assert _run_bwd(b, reduce_only=True) == -errno.EINVAL
        assert all(_untouched(t) for t in b.outputs())
        return
    assert _run_bwd(b, frozen=frozen, reduce_only=reduce_only) == 0
    got = _check_layer(f"bwd_{name}", b, a, kw, frozen, reduce_only)
    if frozen:
        assert not got["sdy"].any() and not got["sdyx"].any()
        live = build()
        assert _run_bwd(live) == 0
        assert _bitwise_equal({k: got[k] for k in ("dgamma", "dbeta")}, live.sums())
    again = build()   # determinism: the same launches on fresh buffers, bit for bit
    assert _run_bwd(again, frozen=frozen, reduce_only=reduce_only) == 0
    assert _bitwise_equal(got, again.sums())


def test_group_norm_apply_gate(cuda):
    """bits + dzscale with and without dyhat, the group-norm apply: with the bits the reduce drops
    dzscale (group norm passes gamma to the apply alone), so the sums are those of the gated dz
    and the apply's dy carries dzscale; dyhat is stored before it"""
    for dtype, dyhat in [(t, h) for t in ("bf16", "fp16", "fp32") for h in (True, False)]:
        M, C = 391, 128
        a = R.layer_inputs(M, C, dtype, seed=43)
        kw = _variant_kw(cuda, dtype, a, M, C, ("bits", "dzscale"))
        b = Bwd(cuda, dtype, a, M, C, kw, want_dyhat=dyhat)
        assert _run_bwd(b) == 0
        ref_sums = R.bwd_ref(a["dz"], a["y"], a["mean"], a["invstd"], dtype, mask=kw["mask"])
        ref = R.bwd_ref(a["dz"], a["y"], a["mean"], a["invstd"], dtype, **kw)
        got = b.sums()
        res = R.bwd_sums_check(got, ref_sums)
        if dyhat:
            res.update(R.dyhat_check(_host(b.dyhat), ref))
        res.update(R.dy_check(_host(b.dy), ref, a["scale"], got["sdy"], got["sdyx"], dtype)[0])
        _record("bwd_bits+dzscale" + ("+dyhat" if dyhat else ""), dtype, res)


@pytest.mark.parametrize("dtype,M,C", BWD_CASES)
def test_backward_sizes(cuda, dtype, M, C):
    """the bits-gated backward at every size that takes another path; the 1,024-block row runs
    reduce + finalize only, the grid-stride row runs in 16-bit"""
    reduce_only = (M, C) == BIG_REDUCE
    a = R.layer_inputs(M, C, dtype, seed=M + C)
    kw = {"mask": _native_bits(cuda, dtype, a, M, C)}
    b = Bwd(cuda, dtype, a, M, C, kw, want_dy=not reduce_only)
    assert _run_bwd(b, reduce_only=reduce_only) == 0
    got = _check_layer("bwd_sizes", b, a, kw, reduce_only=reduce_only)
    again = Bwd(cuda, dtype, a, M, C, kw, want_dy=False)   # the reduce + finalize repeat bit for bit
    assert _run_bwd(again, reduce_only=True) == 0
    assert _bitwise_equal(got, again.sums())


@pytest.mark.parametrize("variant", [(), ("z",), ("dzscale",), ("z", "dzscale")],
                         ids=["ungated", "z", "dzscale", "z+dzscale"])
@pytest.mark.parametrize("M,C", NARROW)
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_backward_narrow(cuda, dtype, M, C, variant):
    """the logits layers' scalar kernels: fp32 dz in 16-channel pixels over a 16-bit y"""
    dz_f32 = dtype != "fp32"
    a = R.layer_inputs(M, C, dtype, seed=M + C, dz_dtype="fp32")
    kw = _variant_kw(cuda, dtype, a, M, C, variant)   # (z has dz's type: y's grid is exact in it)
    b = Bwd(cuda, dtype, a, M, C, kw, dz_f32=dz_f32, want_dyhat=True, ld=16, lddz=16, ldy=16)
    assert _run_bwd(b, dz_f32=dz_f32) == 0
    got = _check_layer("bwd_narrow", b, a, kw)
    again = Bwd(cuda, dtype, a, M, C, kw, dz_f32=dz_f32, want_dyhat=True, ld=16, lddz=16, ldy=16)
    assert _run_bwd(again, dz_f32=dz_f32) == 0 and _bitwise_equal(got, again.sums())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_backward_fp32_dz_over_16_bit_y(cuda, dtype):
    """the 8-wide kernels with an fp32 dz (and z) over a 16-bit y; dyhat is one rounding of dz"""
    M, C = 391, 128
    a = R.layer_inputs(M, C, dtype, seed=47, dz_dtype="fp32")
    for variant in ((), ("z",), ("dzscale",)):
        kw = _variant_kw(cuda, dtype, a, M, C, variant)
        b = Bwd(cuda, dtype, a, M, C, kw, dz_f32=True, want_dyhat=True)
        assert _run_bwd(b, dz_f32=True) == 0
        _check_layer("bwd_fp32dz_" + ("+".join(variant) or "ungated"), b, a, kw)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_backward_strided(cuda, dtype):
    """dz read from 256 channels at offset 256 of a 1,280-wide concat; dy in rows wider than C"""
    M, C = 391, 256
    a = R.layer_inputs(M, C, dtype, seed=51)
    kw = {"mask": _native_bits(cuda, dtype, a, M, C)}
    b = Bwd(cuda, dtype, a, M, C, kw, ld=C + 64, lddz=1280, dzoff=256)
    assert _run_bwd(b) == 0
    _check_layer("bwd_strided", b, a, kw)


def _dual(cuda, dtype, M, C, second_only):
    from seg_hip import LIB
    a = R.layer_inputs(M, C, dtype, seed=61)
    a2 = R.layer_inputs(M, C, dtype, seed=62)
    kw = {"mask": _native_bits(cuda, dtype, a, M, C)}
    if second_only:   # dz arrives gated
        a = dict(a, dz=np.where(R.unpack_bits(kw["mask"], C), a["dz"], np.float32(0)))
    a2 = dict(a2, dz=a["dz"])
    b = Bwd(cuda, dtype, a, M, C, kw, want_dy=not second_only)
    b2 = Bwd(cuda, dtype, a2, M, C, {})
    rc = LIB.seg_op_bn_backward_dual(ABI[dtype], 0, int(second_only), ctypes.byref(b.args),
                                     ctypes.byref(b2.args), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    tag = "dual_second_only" if second_only else "dual"
    got = _check_layer(tag + "_first", b, a, kw, reduce_only=second_only)
    # the second layer: gated by the first's bits in the dual launches; alone (second_only) the
    # apply is ungated, which is the same thing on a dz that arrived gated
    got2 = _check_layer(tag + "_second", b2, a2, kw)
    # and against two single-layer runs of the same inputs: each pair of outputs within the bounds
    # of one float64 reference, i.e. within twice the bound of each other
    s = Bwd(cuda, dtype, a, M, C, kw)
    s2 = Bwd(cuda, dtype, a2, M, C, kw)
    assert _run_bwd(s) == 0 and _run_bwd(s2) == 0
    for one, ain, single, dual_got in ((1, a, s, got), (2, a2, s2, got2)):
        ref = R.bwd_ref(ain["dz"], ain["y"], ain["mean"], ain["invstd"], dtype, **kw)
        sg = _check_layer(f"{tag}_single{one}", single, ain, kw)
        for k, sref, sabs in (("dbeta", "s1", "s1_abs"), ("dgamma", "s2", "s2_abs")):
            assert R.violations(dual_got[k], sg[k], 2 * R.sum_bound(ref[sref], ref[sabs], M))[0] == 0
    again = Bwd(cuda, dtype, a, M, C, kw, want_dy=not second_only)
    again2 = Bwd(cuda, dtype, a2, M, C, {})
    assert LIB.seg_op_bn_backward_dual(ABI[dtype], 0, int(second_only), ctypes.byref(again.args),
                                       ctypes.byref(again2.args), _stream()) == 0
    torch.cuda.synchronize()
    assert _bitwise_equal(got, again.sums()) and _bitwise_equal(got2, again2.sums())


@pytest.mark.parametrize("second_only", [False, True], ids=["both", "second_only"])
@pytest.mark.parametrize("M,C", [(391, 128), (65, 64), (130, 2056)])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_backward_dual(cuda, dtype, M, C, second_only):
    _dual(cuda, dtype, M, C, second_only)


def test_backward_refusals(cuda):
    """what the launchers refuse is refused up front: -EINVAL, a text, nothing written"""
    from seg_hip import LIB
    M = 333
    for dtype in ("bf16", "fp32"):
        a14 = R.layer_inputs(M, 14, dtype, seed=71)
        a = R.layer_inputs(M, 128, dtype, seed=72)
        bits = R.pack_bits(a["r"] > 0)
        shift = np.full(128, 0.1, np.float32)
        cases = [
            # bits with a layout that is not 8-wide (C = 14 in 16-channel pixels)
            (Bwd(cuda, dtype, a14, M, 14, {"mask": np.zeros((M, 2), np.uint8)}, ld=16, lddz=16), False),
            # dshift without the bits
            (Bwd(cuda, dtype, a, M, 128, {"dshift": shift}), False),
            (Bwd(cuda, dtype, a, M, 128, {"dshift": shift, "z": a["r"]}), False),
            # dshift with an apply-side dyhat, with dzscale
            (Bwd(cuda, dtype, a, M, 128, {"dshift": shift, "mask": bits}, want_dyhat=True), False),
            (Bwd(cuda, dtype, a, M, 128, {"dshift": shift, "mask": bits, "dzscale": shift}), False),
            # cs_part without dshift
            (Bwd(cuda, dtype, a, M, 128, {"mask": bits, "beta": a["beta"]}, want_cs=True, want_dy=False), True),
            # both gates
            (Bwd(cuda, dtype, a, M, 128, {"mask": bits, "z": a["r"]}), False),
        ]
        if dtype == "fp32":   # cs_part in fp32
            cases.append((Bwd(cuda, dtype, a, M, 128, {"mask": bits, "dshift": shift, "beta": a["beta"]},
                              want_cs=True, want_dy=False), True))
        for i, (b, reduce_only) in enumerate(cases):
            assert _run_bwd(b, reduce_only=reduce_only) == -errno.EINVAL, (dtype, i)
            assert len(LIB.seg_last_error(None)) > len(b"seg_op_bn_backward: "), (dtype, i)
            assert all(_untouched(t) for t in b.outputs()), (dtype, i)
        # the dual launches take the bits and 8-wide layouts only
        b, b2 = Bwd(cuda, dtype, a, M, 128, {"z": a["r"]}), Bwd(cuda, dtype, a, M, 128, {})
        assert LIB.seg_op_bn_backward_dual(ABI[dtype], 0, 0, ctypes.byref(b.args), ctypes.byref(b2.args),
                                           _stream()) == -errno.EINVAL
        torch.cuda.synchronize()
        assert all(_untouched(t) for t in b.outputs() + b2.outputs())


# ---- forward statistics ---------------------------------------------------------------------
def _finalize(cuda, part, M, C, tile_rows, gamma, pack):
    from seg_hip import LIB
    d = Dev(cuda)
    pp, _ = d.put(np.array(part).reshape(-1))
    gp, _ = d.put(gamma)
    outs = {k: d.poisoned((C,)) for k in ("mean", "invstd", "scale", "var_unb")}
    pk = d.poisoned((2 * C,)) if pack else None
    rc = LIB.seg_op_bn_stats_finalize(pp, M, C, tile_rows, gp, outs["mean"].data_ptr(),
                                      outs["invstd"].data_ptr(), outs["scale"].data_ptr(),
                                      outs["var_unb"].data_ptr(), pk.data_ptr() if pack else None, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = {k: _host(v) for k, v in outs.items()}
    got["pack"] = _host(pk) if pack else None
    return got


@pytest.mark.parametrize("pack", [False, True], ids=["nopack", "pack"])
@pytest.mark.parametrize("case", R.STATS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_stats_finalize(cuda, case, pack):
    M, C, tile_rows, kind = case
    k_mean, k_var, worst = R.stats_k()
    part, gamma = R.stats_case(case)
    got = _finalize(cuda, part, M, C, tile_rows, gamma, pack)
    res = R.stats_check(got, part, M, tile_rows, gamma, k_mean, k_var)
    print(f"MARGIN stats fp32 k_mean_restatement {worst['k_mean']:.4f}")
    print(f"MARGIN stats fp32 k_var_restatement {worst['k_var']:.4f}")
    _record("stats", "fp32", res)
    if kind == "typical":   # the constant channel: var = 0 exactly
        assert got["var_unb"][0] == 0 and got["mean"][0] == 1.5
        assert got["invstd"][0] == pytest.approx(R.BN_EPS ** -0.5, rel=1e-6)
    again = _finalize(cuda, part, M, C, tile_rows, gamma, pack)
    assert _bitwise_equal({k: v for k, v in got.items() if v is not None},
                          {k: v for k, v in again.items() if v is not None})


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_stats_finalize_of_a_native_conv(cuda, dtype):
    """The partials seg_op_conv_fwd writes for (1, 37, 45, 256 -> 64, 1 x 1), finalized: against
    the exact merge of those partials to the finalize's own bound, and against the float64 moments
    of the reference conv. The second target differs from the first by the conv's own fp32
    accumulation (the statistics are taken from the accumulators): per element at most
    d = K 2^-23 |x| |w| (conv_bounds), plus the fp32 tile sums of tile_rows values, T e of the
    sums of their magnitudes; so |mean - ref| <= mean(d) + T e mean|y| + the finalize's bound and
    |var - ref| <= 2 sqrt(var mean(d^2)) + mean(d^2) + 2 T e (var + mean^2) + the finalize's."""
    from oracle.tfseg import ConvSpec, conv_tf
    from seg_hip import LIB, check
    N, H, W, Ci, Co = 1, 37, 45, 256, 64
    M = N * H * W
    g = np.random.default_rng(0)
    x = R.round_to(g.standard_normal((N, H, W, Ci)).astype(np.float32), dtype)
    w = R.round_to((g.standard_normal((Co, 1, 1, Ci)) * np.sqrt(2.0 / Ci)).astype(np.float32), dtype)
    spec = ConvSpec("t", Ci, Co, 1, 1, 1, explicit_pad=False)

    def conv64(xa, wa):
        xt = torch.as_tensor(xa, dtype=torch.float64).permute(0, 3, 1, 2)
        return conv_tf(xt, torch.as_tensor(wa, dtype=torch.float64), spec).permute(0, 2, 3, 1).numpy().reshape(M, Co)

    y64 = conv64(x, w)
    dlt = Ci * 2.0 ** -23 * conv64(np.abs(x), np.abs(w))
    tr = LIB.seg_op_conv_stat_rows(ABI[dtype], N, H, W, Ci, Ci, Co, Co, 1, 1, 1, 0)
    nt = -(-M // tr)
    xd = torch.from_numpy(x).to(cuda, R.TDT[dtype])
    wd = torch.from_numpy(w).to(cuda, R.TDT[dtype])
    yd = torch.zeros((M, Co), dtype=R.TDT[dtype], device=cuda)
    stats = torch.zeros((nt, Co, 2), dtype=torch.float32, device=cuda)
    check(LIB.seg_op_conv_fwd(ABI[dtype], xd.data_ptr(), N, H, W, Ci, Ci, wd.data_ptr(), Co, 1, 1, 1, 0,
                              yd.data_ptr(), Co, stats.data_ptr(), _stream()))
    torch.cuda.synchronize()
    part = stats.cpu().numpy()
    gamma = R.channel_params(Co, 5)[2]
    k_mean, k_var, _ = R.stats_k()
    got = _finalize(cuda, part, M, Co, tr, gamma, True)
    res = R.stats_check(got, part, M, tr, gamma, k_mean, k_var)
    _record("stats_conv", dtype, res)
    ex = R.stats_exact(part, M, tr)
    mean, var = y64.mean(0), y64.var(0)
    d2 = (dlt ** 2).mean(0)
    mean_b = dlt.mean(0) + tr * R.E * np.abs(y64).mean(0) + k_mean * R.E * (np.abs(ex["mean"]) + ex["A_abs"])
    var_b = 2 * np.sqrt(var * d2) + d2 + 2 * tr * R.E * (var + mean ** 2) + k_var * R.E * ex["B_over_N"]
    bessel = M / (M - 1.0)
    _record("stats_conv_moments", dtype, {"mean": R.violations(got["mean"], mean, mean_b),
                                          "var_unb": R.violations(got["var_unb"], var * bessel, bessel * var_b + 2 * R.E * var)})
