"""The argument tuples of the conv kernel-selection tests (tests/test_conv_plan.py) and of the
generator of their parent fixture (tests/golden/make_conv_plan_fixture.py): every request is the
scalar fields of ConvArgs / WgradArgs in declaration order (csrc/conv_args.h) plus pointer flags,
built as csrc/net_layers.cpp builds them (fwd_conv_args, dgrad_conv_args, wgrad_conv_args, the
space-to-depth stem rewrite, strides as alloc_conv pads them). Deterministic, no GPU."""
from oracle.tfseg import SegConfig, build_specs, psp_grids, resnet_units

NT_FIELDS = ("N H W C ldx ldw Ho Wo Co ldy ldr ldr2 KH KW sf st pad_h pad_w dil tap8 ldx2 C2 "
             "ldw2 ldm").split()
WG_FIELDS = "lddy N H W C ldx Ho Wo Co KH KW sf pad_h pad_w dil splits lddy2 Co1".split()
F_RES, F_RES2, F_STATS, F_MASK, F_DUAL = 1, 2, 4, 8, 16


def geom(H, W, k, stride, rate, explicit_pad):
    """conv_geom of csrc/net_build.cpp: (Ho, Wo, pad_h, pad_w)"""
    keff = k + (k - 1) * (rate - 1)
    if explicit_pad:
        return (H - 1) // stride + 1, (W - 1) // stride + 1, (keff - 1) // 2, (keff - 1) // 2
    Ho, Wo = -(-H // stride), -(-W // stride)
    return (Ho, Wo, max((Ho - 1) * stride + keff - H, 0) // 2, max((Wo - 1) * stride + keff - W, 0) // 2)


def pad8(c):
    return (c + 7) // 8 * 8


def co_pad(co):
    return (co + 15) // 16 * 16 if co % 8 else co


def nt(**kw):
    d = dict.fromkeys(NT_FIELDS, 0)
    d.update(kw)
    return [d[k] for k in NT_FIELDS]


def fwd_fields(N, H, W, Ci, Co, k, stride, rate, ep, ldx=None, ldy=None):
    Ho, Wo, ph, pw = geom(H, W, k, stride, rate, ep)
    return nt(N=N, H=H, W=W, C=Ci, ldx=ldx or pad8(Ci), ldw=k * k * Ci, Ho=Ho, Wo=Wo, Co=Co,
              ldy=ldy or co_pad(Co), KH=k, KW=k, sf=stride, st=1, pad_h=ph, pad_w=pw, dil=rate)


def s2d_fields(N, H, W, Co=64):
    """the 16-bit stem (7 x 7 / 2, explicit padding) as 4 x 4 VALID over the space-to-depth image"""
    Ho, Wo, _, _ = geom(H, W, 7, 2, 1, True)
    return nt(N=N, H=Ho + 3, W=Wo + 3, C=16, ldx=16, ldw=256, Ho=Ho, Wo=Wo, Co=Co, ldy=co_pad(Co),
              KH=4, KW=4, sf=1, st=1, dil=1, tap8=2)


def dgrad_fields(N, H, W, Ci, Co, k, stride, rate, ep, lddy=None, lddx=None):
    """the data gradient of that conv as a forward problem over dy (dgrad_conv_args)"""
    Ho, Wo, ph, pw = geom(H, W, k, stride, rate, ep)
    keff = k + (k - 1) * (rate - 1)
    return nt(N=N, H=Ho, W=Wo, C=Co, ldx=lddy or co_pad(Co), ldw=k * k * Co, Ho=H, Wo=W, Co=Ci,
              ldy=lddx or pad8(Ci), KH=k, KW=k, sf=1, st=stride, pad_h=keff - 1 - ph,
              pad_w=keff - 1 - pw, dil=rate)


def with_(f, **kw):
    d = dict(zip(NT_FIELDS, f))
    d.update(kw)
    return [d[k] for k in NT_FIELDS]


def wgrad_fields(N, H, W, Ci, Co, k, stride, rate, ep, s2d=False):
    Ho, Wo, ph, pw = geom(H, W, k, stride, rate, ep)
    d = dict.fromkeys(WG_FIELDS, 0)
    d.update(lddy=co_pad(Co), N=N, H=H, W=W, C=Ci, ldx=pad8(Ci), Ho=Ho, Wo=Wo, Co=co_pad(Co), KH=k,
             KW=k, sf=stride, pad_h=ph, pad_w=pw, dil=rate, splits=1)
    if s2d:
        d.update(H=Ho + 3, W=Wo + 3, C=16, ldx=16, KH=4, KW=4, sf=1, pad_h=0, pad_w=0, dil=1)
    return [d[k] for k in WG_FIELDS]


def network_convs(cfg):
    """(name, N, H, W, spec) of every conv of the network: the input map each one reads"""
    specs = {s.name.split("resnet_v1_%d/" % cfg.depth)[-1]: s for s in build_specs(cfg)}
    N = cfg.nb
    out = []
    H, W = cfg.height, cfg.width
    out.append(("conv1", N, H, W, specs["conv1"]))
    H, W = geom(H, W, 7, 2, 1, True)[:2]
    H, W = -(-H // 2), -(-W // 2)   # 3 x 3 / 2 SAME max pool
    for scope, din, d, dbn, s, r in resnet_units(cfg.depth, cfg.output_stride):
        Ho, Wo = geom(H, W, 3, s, r, s > 1)[:2]
        if scope + "/shortcut" in specs:
            out.append((scope + "/shortcut", N, H, W, specs[scope + "/shortcut"]))
        out.append((scope + "/conv1", N, H, W, specs[scope + "/conv1"]))
        out.append((scope + "/conv2", N, H, W, specs[scope + "/conv2"]))
        out.append((scope + "/conv3", N, Ho, Wo, specs[scope + "/conv3"]))
        H, W = Ho, Wo
    pooled = {}
    if cfg.pyramid == "psp":
        for i, (kh, kw) in enumerate(psp_grids(cfg.height, cfg.width)):
            pooled["Conv" + ("" if i == 0 else "_%d" % i)] = ((H - kh) // kh + 1, (W - kw) // kw + 1)
    elif cfg.pyramid == "aspp":
        pooled["Conv"] = (1, 1)   # the image pool
    for name, s in specs.items():
        if "/bottleneck_v1/" in name and "adaptation_module" not in name or name == "conv1":
            continue
        h, w = pooled.get(name.split("/")[-1], (H, W)) if "pyramid_module" in name else (H, W)
        out.append((name, N, h, w, s))
    return out


NETWORKS = [SegConfig(height=h, width=w, nb_pp=n[0], nb_pb=n[1], nb_pi=n[2], pyramid=p)
            for (h, w, n) in ((1024, 2048, (4, 0, 0)), (97, 145, (1, 1, 1)), (101, 103, (1, 1, 0)))
            for p in ("aspp", "psp")]


def shapes():
    """(label, (N, H, W, Ci, Co, k, stride, rate, explicit_pad)), duplicates removed"""
    from test_gpu_conv import CASES, LD_CASES, RES_CASES, WGRAD_CFG_CASES, WGRAD_PATCH_CASES
    out, seen = [], set()

    def add(label, t):
        t = tuple(int(v) for v in t)
        if t not in seen:
            seen.add(t)
            out.append((label, t))
    for i, c in enumerate(CASES):
        add("CASES[%d]" % i, c)
    for i, c in enumerate(LD_CASES + WGRAD_PATCH_CASES + [c[0] for c in WGRAD_CFG_CASES]):
        add("extra[%d]" % i, c)
    for i, (N, H, W, Co, Ci, _, _) in enumerate(RES_CASES):   # 1 x 1 convs Ci -> Co, by their dgrad
        add("RES_CASES[%d]" % i, (N, H, W, Ci, Co, 1, 1, 1, False))
    for cfg in NETWORKS:
        for name, N, H, W, s in network_convs(cfg):
            add("%s %dx%d %s" % (cfg.pyramid, cfg.height, cfg.width, name),
                (N, H, W, s.ci, s.co, s.k, s.stride, s.rate, s.explicit_pad))
    for co in (14, 7, 3):   # the logits, 16-channel rows
        add("logits %d" % co, (2, 9, 10, 256, co, 1, 1, 1, False))
    return out


def nt_requests():
    """(label, out_f32, fields, flags): forward, data gradient, with one and two residuals, with
    a mask, with the second GEMM; the space-to-depth stem at an even and an odd size"""
    out = []
    for label, c in shapes():
        N, H, W, Ci, Co, k, s, r, ep = c
        out.append((label + " fwd", 0, fwd_fields(*c), F_STATS))
        out.append((label + " fwd nostats", 0, fwd_fields(*c), 0))
        out.append((label + " fwd f32out", 1, fwd_fields(*c), 0))
        if Ci == 3:
            continue
        d = dgrad_fields(*c)
        ld, ldm = d[NT_FIELDS.index("ldy")], Ci // 8
        out.append((label + " dgrad", 0, d, 0))
        out.append((label + " dgrad r", 0, with_(d, ldr=ld), F_RES))
        out.append((label + " dgrad r r2", 0, with_(d, ldr=ld, ldr2=ld), F_RES | F_RES2))
        out.append((label + " dgrad mask", 0, with_(d, ldm=ldm), F_MASK))
        out.append((label + " dgrad r mask", 0, with_(d, ldr=ld, ldm=ldm), F_RES | F_MASK))
        out.append((label + " dgrad mask f32out", 1, with_(d, ldm=ldm), F_MASK))
        dual = dict(ldx2=pad8(Co), C2=Co, ldw2=Co)
        out.append((label + " dgrad dual", 0, with_(d, **dual), F_DUAL))
        out.append((label + " dgrad dual mask", 0, with_(d, ldm=ldm, **dual), F_DUAL | F_MASK))
        out.append((label + " dgrad dual r", 0, with_(d, ldr=ld, **dual), F_DUAL | F_RES))
    for N, H, W in ((4, 1024, 2048), (2, 64, 128), (3, 97, 145), (2, 101, 103)):
        out.append(("stem s2d %dx%d" % (H, W), 0, s2d_fields(N, H, W), F_STATS))
    return out


def wg_requests():
    """(label, fields, flags): the weight gradient of every shape, with a second dy source where
    the shape is 1 x 1, and the stem in space-to-depth form"""
    out = []
    for label, c in shapes():
        f = wgrad_fields(*c)
        out.append((label + " wgrad", f, 0))
        Co = f[WG_FIELDS.index("Co")]
        for co1 in sorted({Co // 2 // 8 * 8, Co // 2 // 256 * 256} - {0}) if c[5] == 1 else ():
            g = list(f)
            g[WG_FIELDS.index("lddy2")] = g[WG_FIELDS.index("lddy")]
            g[WG_FIELDS.index("Co1")] = co1
            out.append((label + " wgrad dy2 Co1=%d" % co1, g, 1))
    for N, H, W in ((4, 1024, 2048), (2, 64, 128), (3, 97, 145), (2, 101, 103)):
        out.append(("stem s2d %dx%d wgrad" % (H, W), wgrad_fields(N, H, W, 3, 64, 7, 2, 1, True, s2d=True), 0))
    return out
