"""One native 16-bit training step checked link by link against float64 restatements (a plain
helper module, like ``tests/conv_bounds.py``).

``step_chain`` runs one step of the native context (forward, loss head, backward) and then
checks, each on the tensors the native step itself consumed:

* every conv's forward output and weight gradient (``oracle/conv_props.py``);
* the whole backward chain of the data gradients: dgrad -> ReLU mask -> BN backward, residual,
  strided-subsample and projection shortcuts, the ASPP / PSP transposes, the stem max-pool;
* with ``links=True`` the forward glue between the convs: the stem BN + ReLU and its 3x3 / 2
  SAME max-pool, BN + ReLU inside every bottleneck, every unit output relu(bn(y3) + shortcut)
  (projection, identity, identity read at stride 2), decrease_fdims, the pyramid branches and
  the pyramid's output into the adaptation units;
* the loss terms, counts and fused decisions against ``OracleNet`` on the native logits.

Tolerances:
* 16-bit tensors that are one rounding of an fp32 value (forward y, every forward link): per
  element |got - ref| <= 2u |ref| + 1e-3 rms(ref), u = 2^-8 (bf16) / 2^-11 (fp16), no violation.
* fp32 weight gradients: per element |got - ref| <= 1e-3 |ref| + 1e-4 rms(ref) +
  2^-24 sqrt(P) sum_p |dy x|.
* BN-backward outputs (dy of every conv): L2-relative ``bn_tol`` over the tensor and, where
  ``tile_tol`` is given, ``tile_tol`` over every 256-pixel tile. With ``few_sample_gap`` a
  pyramid branch normalised over fewer than 64 samples per channel is held to
  max(bn_tol, 4 gap) instead, gap = the L2-relative difference of two float64 BN backwards of
  the same reference gradient, one of them fed that gradient rounded once to the storage
  dtype (the formula cancels most of dh there; the gap is a property of the reference alone).
  Where 4 gap > 0.5 the check cannot discriminate and the tensor is skipped by name; only
  ``SKIPPABLE`` branches may be.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.conv_props import conv_dgrad, conv_fwd, conv_wgrad
from oracle.tfseg import BN_EPS, OracleNet, build_specs, init_params, psp_grids, resnet_units

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ABI = {"bf16": 1, "fp16": 2}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}

PM = "feature_extractor/pyramid_module"
# the only BN backwards the few-sample rule may skip: the PSP grid-1 branch and the ASPP image
# pool (both {PM}/Conv: one sample per image and channel)
SKIPPABLE = (f"{PM}/Conv",)
FEW_SAMPLES = 64


def _elementwise(got, ref, rtol, atol_rms, what, absref=None, n_sum=0):
    """|got - ref| <= rtol |ref| + atol_rms rms(ref) [+ 2^-24 sqrt(n_sum) absref]: absref =
    the same sum over |terms| (an fp32 sum of n_sum terms in any order is off by ~sqrt(n) ulps
    of the absolute sum, which matters where the signed sum cancels). Returns the worst
    err / bound."""
    got = got.double()
    ref = ref.double().to(got.device)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    rms = float(ref.pow(2).mean().sqrt())
    bound = rtol * ref.abs() + atol_rms * rms
    if absref is not None:
        bound = bound + 2.0 ** -24 * math.sqrt(n_sum) * absref
    excess = (got - ref).abs() / bound
    nbad = int((excess > 1).sum())
    assert nbad == 0, f"{what}: {nbad} of {ref.numel()} elements out of tolerance " \
                      f"(worst {float(excess.max()):.3g}x the bound)"
    return float(excess.max())


def _tiles(got, ref, tol, tile_tol, what, rows=256):
    """L2-relative over the tensor and (tile_tol not None) over every `rows`-pixel tile of the
    NHWC pixel order. Returns the tensor's rel."""
    C = ref.shape[-1]
    g = got.double().reshape(-1, C)
    r = ref.double().reshape(-1, C).to(g.device)
    rel = float((g - r).norm() / r.norm().clamp_min(1e-300))
    assert rel < tol, f"{what}: rel {rel:.3g} (tolerance {tol:.3g})"
    if tile_tol is None:
        return rel
    M = r.shape[0]
    pad = (-M) % rows
    e2 = F.pad((g - r).pow(2).sum(1), (0, pad)).reshape(-1, rows).sum(1)
    r2 = F.pad(r.pow(2).sum(1), (0, pad)).reshape(-1, rows).sum(1)
    floor = 1e-2 * float(r2.mean())   # tiles the ReLU mask zeroed almost entirely
    trel = (e2 / r2.clamp_min(floor)).sqrt()
    worst = int(trel.argmax())
    assert float(trel[worst]) < tile_tol, f"{what}: tile {worst} of {len(trel)} rel {float(trel[worst]):.3g}"
    return rel


def _bn_bwd(dz, y, z, gamma, y_exact):
    """TF fused-BN training backward of [relu](bn(y)) (z = the ReLU output whose positives
    pass the gradient, None = no ReLU), float64: dy = g * invstd * (dh - mean dh - xh mean(dh xh)).
    The batch moments come from y_exact (the unrounded conv output: the native statistics are
    reduced from the fp32 accumulators in the conv epilogue), x-hat from the stored y the
    native BN backward reads. With 4 nearly equal samples (the ASPP image-pool branch: means of
    random images) moments of the 16-bit y would be off by more than the batch spread."""
    C = y.shape[-1]
    ye = y_exact.double().reshape(-1, C)
    dh = dz.double() if z is None else dz.double() * (z > 0)
    dh = dh.reshape(-1, C)
    mu = ye.mean(0)
    inv = torch.rsqrt(ye.var(0, unbiased=False) + BN_EPS)
    xh = (y.double().reshape(-1, C) - mu) * inv
    out = gamma * inv * (dh - dh.mean(0) - xh * (dh * xh).mean(0))
    return out.reshape(y.shape)


def bn_bwd_gap(dz, y, z, gamma, y_exact, dtype):
    """(reference BN backward, gap): gap = the L2-relative difference between the float64 BN
    backward fed dz and the same fed dz rounded once to the storage dtype."""
    ref = _bn_bwd(dz, y, z, gamma, y_exact)
    rnd = _bn_bwd(dz.to(TDT[dtype]).double(), y, z, gamma, y_exact)
    return ref, float((rnd - ref).norm() / ref.norm().clamp_min(1e-300))


def _bn_fwd(y, gamma, beta, y_exact, relu=True, shortcut=None):
    """[relu](bn(y) [+ shortcut]) in float64: the batch moments from y_exact (as _bn_bwd), the
    normalised values from the stored y the native BN apply reads."""
    C = y.shape[-1]
    ye = y_exact.double().reshape(-1, C)
    mu = ye.mean(0)
    inv = torch.rsqrt(ye.var(0, unbiased=False) + BN_EPS)
    out = (y.double() - mu) * (gamma * inv) + beta
    if shortcut is not None:
        out = out + shortcut
    return torch.relu(out) if relu else out


def _maxpool_pads(H, W, Ho, Wo):
    return max((Ho - 1) * 2 + 3 - H, 0) // 2, max((Wo - 1) * 2 + 3 - W, 0) // 2


def _maxpool_fwd(z0):
    """slim max_pool2d 3x3 / 2 SAME (out = ceil(in / 2), TF's pads, padding never selected)."""
    N, H, W, C = z0.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ph, pw = _maxpool_pads(H, W, Ho, Wo)
    zp = torch.full((N, H + 2, W + 2, C), -math.inf, dtype=torch.float64, device=z0.device)
    zp[:, ph:ph + H, pw:pw + W] = z0
    out = None
    for i in range(3):
        for j in range(3):
            t = zp[:, i:i + 2 * (Ho - 1) + 1:2, j:j + 2 * (Wo - 1) + 1:2]
            out = t if out is None else torch.maximum(out, t)
    return out


def _maxpool_bwd(z0, g):
    """3x3 / 2 SAME max-pool backward: the gradient goes to the first maximum of each window
    in row-major scan order (TF MaxPoolGrad), padding never selected."""
    N, H, W, C = z0.shape
    Ho, Wo = g.shape[1], g.shape[2]
    ph, pw = _maxpool_pads(H, W, Ho, Wo)
    zp = torch.full((N, H + 2, W + 2, C), -math.inf, dtype=torch.float64, device=z0.device)
    zp[:, ph:ph + H, pw:pw + W] = z0
    taps = [zp[:, i:i + 2 * (Ho - 1) + 1:2, j:j + 2 * (Wo - 1) + 1:2] for i in range(3) for j in range(3)]
    am = torch.stack(taps, 0).argmax(0)     # first maximum
    del taps
    acc = torch.zeros_like(zp)
    for t in range(9):
        i, j = divmod(t, 3)
        acc[:, i:i + 2 * (Ho - 1) + 1:2, j:j + 2 * (Wo - 1) + 1:2] += g * (am == t)
    return acc[:, ph:ph + H, pw:pw + W]


def step_chain(cuda, cfg, dtype, param_seed, data_seed, loss_scale=None, links=False,
               bn_tol=2e-2, tile_tol=5e-2, few_sample_gap=False, report=None):
    """One native step of `cfg` in `dtype` (seeded weights and synthetic batch), then the checks
    of the module docstring. `report` (a dict) receives the debug tensors' dims (`dims`), the
    worst err / bound of the forward links (`link_excess`: name -> figure), every BN backward's
    (rel, gap, tolerance) (`bn_bwd`) and the names the few-sample rule skipped (`skipped`)."""
    from input_pipelines.synthetic import batch
    from seg_hip import SegContext
    assert cfg.fov_k == 0 and cfg.norm == "batch" and cfg.upsampling == "bilinear"
    assert cfg.pyramid in ("psp", "aspp")
    depth, pyramid, H, W = cfg.depth, cfg.pyramid, cfg.height, cfg.width
    npp, npb, npi = cfg.nb_pp, cfg.nb_pb, cfg.nb_pi
    NB = npp + npb + npi
    rep = report if report is not None else {}
    rep.update(dims={}, link_excess={}, bn_bwd={}, skipped=[])
    params = {k: v.astype(np.float32) for k, v in init_params(cfg, seed=param_seed).items()}
    data = batch(data_seed, npp, npb, npi, H, W)
    ctx = SegContext(depth=depth, pyramid=pyramid, height=H, width=W, nb_pp=npp, nb_pb=npb,
                     nb_pi=npi, dtype=dtype)
    ctx.load_params(params)
    if loss_scale is not None:
        ctx.set_loss_scale(loss_scale)
    dec = torch.zeros((NB, H, W), dtype=torch.int32, device=cuda)
    ctx.forward(torch.as_tensor(data["images"]).to(cuda))
    dev = lambda a: None if a is None else torch.as_tensor(a).to(cuda)
    ctx.loss(dev(data["px"]), dev(data["bbox"]), dev(data["tag"]), dec)
    losses, _, logits = ctx.outputs()
    ctx.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ctx.grads).all()), "non-finite gradients"
    u = ULP[dtype]
    specs = build_specs(cfg)
    idx = {s.name: i for i, s in enumerate(specs)}
    info = {p.name: p for p in ctx.param_info}

    def X(i):
        return ctx.debug_device(f"conv{i}_x").double()

    def Y(i):
        return ctx.debug_device(f"conv{i}_y").double()

    def DY(i):
        return ctx.debug_device(f"conv{i}_dy").double()

    def Wt(i):   # the weights the step ran with (16-bit copies of the fp32 masters)
        return torch.as_tensor(params[specs[i].name + "/weights"]).to(cuda).to(TDT[dtype]).double()

    def gamma(i):
        return torch.as_tensor(params[specs[i].name + "/BatchNorm/gamma"], dtype=torch.float64, device=cuda)

    def beta(i):
        return torch.as_tensor(params[specs[i].name + "/BatchNorm/beta"], dtype=torch.float64, device=cuda)

    def native_grad(i):
        p = info[specs[i].name + "/weights"]
        return ctx.grads[p.offset:p.offset + p.numel].view(p.shape)

    for i in range(len(specs)):
        rep["dims"][f"conv{i}_x"] = tuple(ctx.debug_device(f"conv{i}_x").shape)
        rep["dims"][f"conv{i}_y"] = tuple(ctx.debug_device(f"conv{i}_y").shape)

    # conv3 layers the linear BN-backward fold took (csrc/lbf.h): their weight gradient was
    # formed from the affine dz3 = A dyhat + B + D z3 without rounding dz3 to 16 bits (so the
    # 16-bit dz3 the apply would have stored is no reference for it: its rounding errors follow
    # z3 wherever the gate is closed and do not average out, 2.4-2.8e-3 of the gradient on
    # these layers, profiles/r05_lbf_diag.txt); the reference is that affine form in float64
    # from the step's coefficients and gated gradient with the exact conv output. The
    # coefficients themselves are checked through dz3 (chk below: the apply on the same inputs
    # against the float64 BN backward)
    folded = set()
    if ctx.counter("lbf_layers") > 0:
        for i, s in enumerate(specs):
            try:
                ctx.debug_device(f"conv{i}_lbfcoef")
                folded.add(i)
            except Exception:
                pass

    # ---- every conv: forward output and weight gradient (the stem's 3 real channels of tap8)
    for i, s in enumerate(specs):
        x = X(i)
        _elementwise(Y(i), conv_fwd(x, Wt(i), s), 2 * u, 1e-3, f"fwd {s.name}")
        if i in folded:
            coef = ctx.debug_device(f"conv{i}_lbfcoef").double().reshape(3, -1)
            dy = coef[0] * ctx.debug_device(f"conv{i}_dyhat").double() + coef[1] + \
                coef[2] * conv_fwd(x, Wt(i), s)
        else:
            dy = DY(i)
        _elementwise(native_grad(i), conv_wgrad(x, dy, s), 1e-3, 1e-4, f"wgrad {s.name}",
                     absref=conv_wgrad(x.abs(), dy.abs(), s), n_sum=dy[..., 0].numel())
        del dy
        del x

    rn = f"feature_extractor/base/resnet_v1_{depth}"
    scopes = [f"{rn}/{unit[0]}" for unit in resnet_units(depth, 8)]
    heads = ("l1", "l2_vehicle", "l2_human")
    fd = cfg.feature_dims_decreased
    idfd = idx["feature_extractor/extension/decrease_fdims"]
    ifin = idx[f"{PM}/Conv_5" if pyramid == "aspp" else f"{PM}/Conv_4"]

    # ---- forward links: each native 16-bit tensor against the float64 restatement of the op
    # that wrote it, fed the native tensors upstream of it
    def link(got, ref, what):
        rep["link_excess"][what] = _elementwise(got, ref, 2 * u, 1e-3, f"link {what}")

    def act(i, relu=True, shortcut=None):
        return _bn_fwd(Y(i), gamma(i), beta(i), conv_fwd(X(i), Wt(i), specs[i]), relu, shortcut)

    def unit_links(scope, out):
        i1, i2, i3 = idx[f"{scope}/conv1"], idx[f"{scope}/conv2"], idx[f"{scope}/conv3"]
        short = scope.replace(rn + "/", "").replace("/bottleneck_v1", "")
        link(X(i2), act(i1), f"{short} bn1+relu")
        link(X(i3), act(i2), f"{short} bn2+relu")
        isc = idx.get(f"{scope}/shortcut")
        xin = X(i1)
        if isc is not None:
            assert torch.equal(X(isc), xin), f"{short}: shortcut and conv1 read different inputs"
            s, kind = act(isc, relu=False), "projection"
        elif out.shape[1] == xin.shape[1] and out.shape[2] == xin.shape[2]:
            s, kind = xin, "identity"
        else:   # resnet_utils.subsample: the identity shortcut read at stride 2
            s, kind = xin[:, ::2, ::2], "subsample"
        link(out, act(i3, relu=True, shortcut=s), f"{short} out ({kind})")
        return kind

    if links:
        z0 = ctx.debug_device("z0").double()
        rep["dims"]["z0"] = tuple(z0.shape)
        link(z0, act(0), "stem bn+relu")
        link(X(idx[f"{scopes[0]}/conv1"]), _maxpool_fwd(z0), "stem max-pool")
        del z0
        kinds = []
        for k, scope in enumerate(scopes):
            out = X(idx[f"{scopes[k + 1]}/conv1"]) if k + 1 < len(scopes) else X(idfd)
            kinds.append(unit_links(scope, out))
        # R50 / R101 at output stride 8: 4 projection units, 1 subsample unit (block1's last)
        assert kinds.count("projection") == 4 and kinds.count("subsample") == 1, kinds
        feat = X(idx["adaptation_module/l1_features/conv1"])
        zd = act(idfd)
        if pyramid == "aspp":
            concat = X(ifin)
            for b in range(1, 5):
                ib = idx[f"{PM}/Conv_{b}"]
                if b == 1:
                    link(X(ib), zd, "decrease_fdims bn+relu")
                else:
                    assert torch.equal(X(ib), X(idx[f"{PM}/Conv_1"])), f"ASPP branch {b} input"
                link(concat[..., b * fd:(b + 1) * fd], act(ib), f"ASPP branch {b} bn+relu")
            ip = idx[f"{PM}/Conv"]
            link(X(ip), X(idx[f"{PM}/Conv_1"]).mean((1, 2), keepdim=True), "ASPP image pool mean")
            zb = ctx.debug_device("pyr0_z").double()
            link(zb, act(ip), "ASPP image pool bn+relu")
            link(concat[..., :fd], zb.expand(-1, concat.shape[1], concat.shape[2], -1),
                 "ASPP image pool broadcast")
            link(feat, act(ifin), "pyramid out bn+relu")
            del concat, zb
        else:
            link(X(ifin)[..., :fd], zd, "decrease_fdims bn+relu")
            for b, nm in enumerate(["Conv", "Conv_1", "Conv_2", "Conv_3"]):
                link(ctx.debug_device(f"pyr{b}_z").double(), act(idx[f"{PM}/{nm}"]), f"PSP branch {nm} bn+relu")
            link(feat, act(ifin), "pyramid out bn+relu")
        del zd
        for h in heads:
            assert torch.equal(X(idx[f"adaptation_module/{h}_features/conv1"]), feat), f"{h} head input"
            kind = unit_links(f"adaptation_module/{h}_features", X(idx[f"softmax_classifier/{h}_logits"]))
            assert kind == "identity"
        del feat

    def chk(i, dz, z, what):
        name = specs[i].name
        ye = conv_fwd(X(i), Wt(i), specs[i])
        what = f"{what} -> dy {name}"
        if not few_sample_gap:
            rel = _tiles(DY(i), _bn_bwd(dz, Y(i), z, gamma(i), ye), bn_tol, tile_tol, what)
            rep["bn_bwd"][name] = (rel, None, bn_tol)
            return
        ref, gap = bn_bwd_gap(dz, Y(i), z, gamma(i), ye, dtype)
        samples = ye[..., 0].numel()
        few = name.startswith(PM + "/") and samples < FEW_SAMPLES
        tol = max(bn_tol, 4 * gap) if few else bn_tol
        if few and 4 * gap > 0.5:   # the check cannot discriminate
            assert name in SKIPPABLE, f"{what}: gap {gap:.3g} on a tensor that may not be skipped"
            rep["skipped"].append(name)
            rep["bn_bwd"][name] = (None, gap, None)
            return
        rel = _tiles(DY(i), ref, tol, tile_tol, what)
        rep["bn_bwd"][name] = (rel, gap, tol)

    def dgrad(i, like):
        return conv_dgrad(DY(i), Wt(i), specs[i], like.shape[1], like.shape[2])

    def unit_chain(scope, g_out, out):
        """conv3 (+ projection shortcut) from the unit-output gradient, then conv3 -> conv2 ->
        conv1 inside the unit; returns the gradient w.r.t. the unit input."""
        i1, i2, i3 = idx[f"{scope}/conv1"], idx[f"{scope}/conv2"], idx[f"{scope}/conv3"]
        chk(i3, g_out, out, f"{scope} out")
        isc = idx.get(f"{scope}/shortcut")
        if isc is not None:
            chk(isc, g_out, out, f"{scope} out")
        chk(i2, dgrad(i3, X(i3)), X(i3), f"{scope} conv3 dgrad")
        chk(i1, dgrad(i2, X(i2)), X(i2), f"{scope} conv2 dgrad")
        xin = X(i1)
        g_in = dgrad(i1, xin)
        m = g_out * (out > 0)
        if isc is not None:
            g_in += dgrad(isc, xin)
        elif m.shape[1] == xin.shape[1] and m.shape[2] == xin.shape[2]:
            g_in += m
        else:   # resnet_utils.subsample: identity shortcut read at stride 2
            g_in[:, ::2, ::2] += m
        return g_in

    # ---- heads: logits dgrad -> head unit; dfeat = sum over heads (identity shortcuts)
    dfeat = None
    for h in heads:
        il = idx[f"softmax_classifier/{h}_logits"]
        out = X(il)
        g = unit_chain(f"adaptation_module/{h}_features", dgrad(il, out), out)
        dfeat = g if dfeat is None else dfeat + g
    if pyramid == "aspp":
        # ---- ASPP: final 1x1 over the 1280-channel concat, four conv branches, image pool
        concat = X(ifin)
        chk(ifin, dfeat, X(idx["adaptation_module/l1_features/conv1"]), "dfeat")
        dconcat = dgrad(ifin, concat)
        dz_dfd = 0
        for b in range(1, 5):
            ib = idx[f"{PM}/Conv_{b}"]
            chk(ib, dconcat[..., b * fd:(b + 1) * fd], concat[..., b * fd:(b + 1) * fd], "ASPP concat")
            dz_dfd = dz_dfd + dgrad(ib, X(ib))
        ip = idx[f"{PM}/Conv"]
        chk(ip, dconcat[..., :fd].sum((1, 2), keepdim=True), concat[:, :1, :1, :fd], "ASPP image pool")
        dz_dfd = dz_dfd + dgrad(ip, X(ip)) / (X(ifin).shape[1] * X(ifin).shape[2])
        chk(idfd, dz_dfd, X(idx[f"{PM}/Conv_1"]), "ASPP inputs")
    else:
        # ---- PSP (hierarchical.py:186-207): concat = [z | resize(relu(bn(conv(avgpool_k(z)))))
        # for the grids k = 1, 2, 3, 6], the 1280 -> 256 Conv_4 over it. Forward: the pooled
        # inputs (VALID windows of (hf/8, wf/8) // k, remainder rows / columns dropped) and the
        # align-corners resizes into the concat; backward: the resize transposes, the branch BN
        # backward gated by the branch's own ReLU output, the branch data gradients and the
        # average-pool transposes summed with the identity slice into decrease_fdims' output
        # gradient. float64 references; pooling and resizing by torch on the device
        concat = X(ifin)
        z = concat[..., :fd].permute(0, 3, 1, 2)                       # NCHW, decrease_fdims output
        hf, wf = z.shape[2], z.shape[3]
        chk(ifin, dfeat, X(idx["adaptation_module/l1_features/conv1"]), "dfeat")
        dconcat = dgrad(ifin, concat)
        dz_dfd = dconcat[..., :fd].clone()
        grids = psp_grids(H, W)
        rep["psp_grids"] = grids
        for b, nm in enumerate(["Conv", "Conv_1", "Conv_2", "Conv_3"]):
            ib = idx[f"{PM}/{nm}"]
            kh, kw = grids[b]
            pooled = F.avg_pool2d(z, (kh, kw), stride=(kh, kw)).permute(0, 2, 3, 1)
            _elementwise(X(ib), pooled, 2 * u, 1e-3, f"PSP pool {nm} ({kh}x{kw})")
            zb = ctx.debug_device(f"pyr{b}_z").double()
            up = F.interpolate(zb.permute(0, 3, 1, 2), size=(hf, wf), mode="bilinear",
                               align_corners=True).permute(0, 2, 3, 1)
            _elementwise(concat[..., (b + 1) * fd:(b + 2) * fd], up, 2 * u, 1e-3, f"PSP resize {nm}")
            src = torch.zeros_like(zb.permute(0, 3, 1, 2), requires_grad=True)
            F.interpolate(src, size=(hf, wf), mode="bilinear", align_corners=True).backward(
                dconcat[..., (b + 1) * fd:(b + 2) * fd].permute(0, 3, 1, 2))
            dzb = src.grad.permute(0, 2, 3, 1)
            chk(ib, dzb, zb, f"PSP resize transpose {nm}")
            dpool = dgrad(ib, X(ib))
            zin = torch.zeros_like(z, requires_grad=True)
            F.avg_pool2d(zin, (kh, kw), stride=(kh, kw)).backward(dpool.permute(0, 3, 1, 2))
            dz_dfd += zin.grad.permute(0, 2, 3, 1)
            del zb, up, src, dzb, dpool, zin
        chk(idfd, dz_dfd, concat[..., :fd], "PSP inputs")
    # ---- encoder units, top down, through residual / subsample / projection shortcuts
    g_out, out = dgrad(idfd, X(idfd)), X(idfd)
    for k in reversed(range(len(scopes))):
        g_out = unit_chain(scopes[k], g_out, out)
        out = X(idx[f"{scopes[k]}/conv1"])
    # ---- stem: max-pool backward -> ReLU mask -> BN backward
    z0 = ctx.debug_device("z0").double()
    rep["dims"]["z0"] = tuple(z0.shape)
    chk(0, _maxpool_bwd(z0, g_out), z0, "max-pool")
    del z0, g_out, out, dfeat, dconcat, concat, dz_dfd

    # ---- loss head on the native low-resolution logits (define_losses_hierarchical.py:98-210)
    net = OracleNet(cfg, params)
    lg = logits.double().cpu()
    low = {}
    c0 = 0
    for key, c in (("l1_logits", 14), ("l2_vehicle_logits", 7), ("l2_human_logits", 3)):
        low[key] = lg[..., c0:c0 + c].permute(0, 3, 1, 2).contiguous()
        c0 += c
    L = net.losses(low, data["px"], data["bbox"], data["tag"])
    ref = [float(L[k]) for k in ("segmentation", "l1_segmentation", "l2_vehicle_segmentation",
                                  "l2_human_segmentation")]
    lv = losses.cpu().numpy()
    np.testing.assert_allclose(lv[:4], ref, rtol=1e-4)
    for a, b in zip(lv[4:7], L["counts"]):   # weak weights follow the l1 argmax (near-ties)
        assert abs(int(a) - int(b)) <= (0 if npb + npi == 0 else max(2, 1e-5 * int(b)))
    _, _, _, fused = net.head_predictions(low)
    mism = float((dec.cpu().long() != fused).double().mean())
    assert mism < 1e-5, f"fused decisions differ on {mism:.2e} of the pixels"
    ctx.close()
    return rep
