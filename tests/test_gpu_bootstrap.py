"""Bootstrapped per-pixel l1 loss (--bootstrapping_percentage, seg_set_bootstrap) on the GPU:
the exact K-th-largest select on crafted arrays, the l1 loss map against the float64 restatement
(tests/bootstrap_ref.py) on the native logits, the selection exact on the device's own map, the
gradient seed and losses under the device's mask, the off-path identities, determinism, one
16-bit context and the public layer.

One context per shape runs every percentage once (module cache); the tests read the record.
Bounds: the map and the gradient seed at 1e-5 (the L2-relative norm of tests/test_gpu_step.py,
the bound test_loss_head_gradient_fp32 holds the seed at), the l1 loss at 1e-3; everything about
the selection, the l2 terms and the identities is bitwise. Measured margins:
profiles/bootstrap_margins.txt."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bootstrap_ref as br
from oracle.tfseg import OracleNet, SegConfig, init_params

pytestmark = pytest.mark.gpu

C1, C2, C3 = 14, 7, 3
CT = C1 + C2 + C3
PCTS = (1, 25, 60)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# the select op on crafted arrays
# ---------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 257, 6145, (1 << 20) + 3)


def _ks(n):
    return sorted({k for k in (1, 2, n // 2, n - 1, n) if 1 <= k <= n})


def _uniform(rng, n, k):
    return [rng.random(n, dtype=np.float32)]


def _all_equal(rng, n, k):
    return [np.full(n, 0.37, np.float32)]


def _all_zero(rng, n, k):
    return [np.zeros(n, np.float32)]


def _two_values(rng, n, k):
    """The tie group holding rank k extends to both sides of it: once the low value's group
    (k // 2 high entries), once the high value's (k + (n - k) // 2 high entries)."""
    out = []
    for n_hi in (k // 2, k + (n - k) // 2):
        a = np.full(n, 0.25, np.float32)
        a[:n_hi] = 3.5
        out.append(rng.permutation(a))
    return out


def _wide_mix(rng, n, k):
    kind = rng.integers(0, 3, n)
    den = (rng.integers(1, 1 << 23, n).astype(np.uint32)).view(np.float32)     # denormals
    big = (10.0 ** rng.uniform(-30, 30, n)).astype(np.float32)
    big[rng.integers(0, n)] = np.float32(1e30)
    return [np.where(kind == 0, den, np.where(kind == 1, np.float32(0), big)).astype(np.float32)]


def _low_bits(rng, n, k):
    """Three values of the top digit, four of the middle one, the lowest 10 bits random: every
    digit pass has to decide something."""
    bits = (np.uint32(0x3F800000) + (rng.integers(0, 3, n).astype(np.uint32) << 21)
            + (rng.integers(0, 4, n).astype(np.uint32) << 10) + rng.integers(0, 1024, n).astype(np.uint32))
    return [bits.astype(np.uint32).view(np.float32)]


@pytest.mark.parametrize("make", [_uniform, _all_equal, _all_zero, _two_values, _wide_mix, _low_bits],
                         ids=lambda f: f.__name__.strip("_"))
def test_select_op(cuda, make):
    from seg_hip import bootstrap_threshold
    rng = np.random.default_rng(7)
    for n in SIZES:
        for k in _ks(n):
            for a in make(rng, n, k):
                assert a.dtype == np.float32 and a.shape == (n,) and np.isfinite(a).all()
                assert not np.signbit(a).any()
                rc, tau, n_ge = bootstrap_threshold(torch.from_numpy(a).to(cuda), k)
                assert rc == 0, (n, k, rc)
                want = np.sort(a)[n - k]
                assert _bits(np.float32(tau)) == _bits(want), (n, k, tau, want)
                assert n_ge == int((a >= want).sum()), (n, k, n_ge)


def test_select_op_bad_k(cuda):
    from seg_hip import LIB, bootstrap_threshold
    t = torch.rand(65, device=cuda)
    for k in (0, -1, 66):
        rc, _, _ = bootstrap_threshold(t, k)
        assert rc == -22, (k, rc)
        assert b"seg_op_bootstrap_threshold" in LIB.seg_last_error(None)


# ---------------------------------------------------------------------------------------------
# one context per shape: every percentage once
# ---------------------------------------------------------------------------------------------
SHAPES = {
    "48x64": (SegConfig(height=48, width=64, nb_pp=1, nb_pb=1, pyramid="none"), "fp32"),
    "64x128-aspp-pp2": (SegConfig(height=64, width=128, nb_pp=2, pyramid="aspp"), "fp32"),
    "64x512-yf": (SegConfig(height=64, width=512, nb_pp=1, nb_pb=1, pyramid="none"), "fp32"),
    "101x103": (SegConfig(height=101, width=103, nb_pp=1, nb_pb=1, pyramid="none"), "fp32"),
    "97x145-yf": (SegConfig(height=97, width=145, nb_pp=1, nb_pb=1, nb_pi=1, pyramid="none"), "fp32"),
    "64x128-bf16": (SegConfig(height=64, width=128, nb_pp=1, nb_pb=1, pyramid="none"), "bf16"),
}
FP32 = [k for k, v in SHAPES.items() if v[1] == "fp32"]
_CACHE = {}


def _void_rectangle(px):
    """Valid labels only inside a rectangle of under 20 % of the image; void (19) elsewhere."""
    n, h, w = px.shape
    out = np.full_like(px, 19)
    y1, x1 = max(1, (2 * h) // 5), max(1, (2 * w) // 5)          # 0.4 * 0.4 = 16 %
    out[:, :y1, :x1] = np.where(px[:, :y1, :x1] == 19, 3, px[:, :y1, :x1])
    return out


def _record(cuda, key):
    if key in _CACHE:
        return _CACHE[key]
    from input_pipelines.synthetic import batch
    from seg_hip import SegContext
    cfg, dtype = SHAPES[key]
    params = {k: v.astype(np.float32) for k, v in init_params(cfg, seed=3).items()}
    data = batch(11, cfg.nb_pp, cfg.nb_pb, cfg.nb_pi, cfg.height, cfg.width)
    ctx = SegContext(depth=cfg.depth, pyramid=cfg.pyramid, height=cfg.height, width=cfg.width,
                     nb_pp=cfg.nb_pp, nb_pb=cfg.nb_pb, nb_pi=cfg.nb_pi, dtype=dtype,
                     weight_decay=cfg.weight_decay, bn_decay=cfg.bn_decay)
    ctx.load_params(params)
    px = torch.as_tensor(data["px"]).to(cuda)
    px_rect = torch.as_tensor(_void_rectangle(data["px"])).to(cuda)
    bb = torch.as_tensor(data["bbox"]).to(cuda) if cfg.nb_pb else None
    tg = torch.as_tensor(data["tag"]).to(cuda) if cfg.nb_pi else None
    ctx.forward(torch.as_tensor(data["images"]).to(cuda))

    def snap(labels=px, with_map=False):
        ctx.loss(labels, bb, tg)
        torch.cuda.synchronize()
        s = dict(out=ctx.outputs()[0].cpu().numpy().copy(),
                 grad_un=ctx.debug_tensor("grad_un")[..., :CT].copy(),
                 dzscale=ctx.debug_tensor("dzscale").reshape(-1)[:CT].copy(),
                 launches=ctx.counter("bootstrap_launches"))
        if with_map:
            s["map"] = ctx.debug_tensor("l1_loss_map")[..., 0].copy()
            s["tau"] = ctx.debug_tensor("bootstrap_tau").reshape(-1)[:1].copy()
        return s

    r = dict(cfg=cfg, params=params, data=data, rect=_void_rectangle(data["px"]))
    r["off"] = snap()
    assert r["off"]["launches"] == 0
    r["rect_off"] = snap(px_rect)
    hd = torch.empty((cfg.nb, cfg.height, cfg.width, 3), dtype=torch.int32, device=cuda)
    ctx.full_predictions(head_decisions=hd)
    r["d1_weak"] = hd[cfg.nb_pp:, ..., 0].cpu().numpy().astype(np.int64)
    r["logits"] = ctx.outputs()[2][..., :CT].double().cpu()
    for p in PCTS + (100,):
        ctx.set_bootstrap(p)
        r[p] = snap(with_map=True)
    ctx.set_bootstrap(25)
    r["25_again"] = snap(with_map=True)
    r["rect_25"] = snap(px_rect, with_map=True)
    ctx.set_bootstrap(-1)
    r["off_again"] = snap()
    ctx.close()
    _CACHE[key] = r
    return r


def _reference(r):
    """float64 map and weights on the native logits (once per record)."""
    if "ref" not in r:
        lg = r["logits"]
        low = {"l1_logits": lg[..., :C1].permute(0, 3, 1, 2).contiguous()}
        r["ref"] = br.l1_loss_map(r["cfg"], low["l1_logits"], r["data"]["px"])
    return r["ref"]


def _check_map(r, key):
    m_ref, w = _reference(r)
    m = r[25]["map"]
    assert m.shape == m_ref.shape
    assert np.isfinite(m).all() and not np.signbit(m).any()       # finite, >= +0, never -0
    assert (_bits(m)[~w] == 0).all()                               # exactly +0.0f where unweighted
    err = _rel(m, m_ref)
    print(f"[bootstrap] {key}: l1 loss map rel {err:.3e}")
    assert err < 1e-5, err
    for p in PCTS + (100,):
        assert _same(r[p]["map"], m)                               # the map does not depend on p


def _check_selection(r, key):
    cfg = r["cfg"]
    m_ref, w = _reference(r)
    for p in PCTS:
        m, tau = r[p]["map"], r[p]["tau"]
        M = m.size
        K = br.k_of(p, M)
        assert M == cfg.nb_pp * cfg.height * cfg.width
        want = np.sort(m.ravel())[M - K]
        assert _bits(tau)[0] == _bits(want), (p, tau, want)
        n1 = int((w & (m >= tau[0])).sum())
        assert int(r[p]["out"][4]) == n1, (p, r[p]["out"][4], n1)
        assert n1 >= 1
        ref_mask = br.select_mask(m_ref, w, br.threshold(m_ref, K))
        diff = float((ref_mask != (w & (m >= tau[0]))).mean())
        print(f"[bootstrap] {key} p={p}: K {K} n1 {n1} tau {tau[0]:.6g} "
              f"float64-mask differs on {100 * diff:.4f} % of pixels")


def _check_gradient(r, key):
    cfg = r["cfg"]
    _, w = _reference(r)
    net = OracleNet(cfg, r["params"])
    lg = r["logits"]
    for p in PCTS:
        s = r[p]
        mask = w & (s["map"] >= s["tau"][0])
        low, c0 = {}, 0
        for name, c in (("l1_logits", C1), ("l2_vehicle_logits", C2), ("l2_human_logits", C3)):
            low[name] = lg[..., c0:c0 + c].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            c0 += c
        L = br.losses_with_mask(net, low, r["data"]["px"], r["data"].get("bbox"), r["data"].get("tag"),
                                mask, weak_l1_decisions=r["d1_weak"] if cfg.nb_pb + cfg.nb_pi else None)
        assert tuple(int(v) for v in L["counts"]) == tuple(int(v) for v in s["out"][4:7])
        l1_ref = float(L["l1_segmentation"].detach())
        l1_err = abs(float(s["out"][1]) - l1_ref) / abs(l1_ref)
        print(f"[bootstrap] {key} p={p}: l1 loss rel {l1_err:.3e}")
        assert l1_err < 1e-3, l1_err
        L["segmentation"].backward()
        g_nat = s["grad_un"].astype(np.float64) * s["dzscale"].astype(np.float64)
        c0 = 0
        for name, c in (("l1_logits", C1), ("l2_vehicle_logits", C2), ("l2_human_logits", C3)):
            ref = low[name].grad.permute(0, 2, 3, 1).numpy()
            err = _rel(g_nat[..., c0:c0 + c], ref)
            print(f"[bootstrap] {key} p={p}: seed {name} rel {err:.3e}")
            assert err < 1e-5, (name, err)
            c0 += c
        # l2 terms bitwise those of the off run on the same context and inputs
        off = r["off"]
        for i in (2, 3, 5, 6, 8, 9):
            assert _same(s["out"][i], off["out"][i]), i
        assert _same(s["grad_un"][..., C1:], off["grad_un"][..., C1:])
        assert _same(s["dzscale"][C1:], off["dzscale"][C1:])
        # weak images take no l1 gradient
        assert not s["grad_un"][cfg.nb_pp:, ..., :C1].any()
        # a subset of the off path's pixels, the hardest ones: never more pixels, never an easier
        # mean (1e-6: the two means are rounded separately); 1 % of these maps is a strict subset
        assert s["out"][4] <= off["out"][4] and s["out"][1] >= off["out"][1] * (1 - 1e-6)
        if p == 1:
            assert s["out"][4] < off["out"][4] and s["out"][1] > off["out"][1]


@pytest.mark.parametrize("key", FP32)
def test_map_matches_reference(cuda, key):
    _check_map(_record(cuda, key), key)


@pytest.mark.parametrize("key", FP32)
def test_selection_exact_on_device_map(cuda, key):
    _check_selection(_record(cuda, key), key)


@pytest.mark.parametrize("key", FP32)
def test_gradient_seed_and_losses_under_device_mask(cuda, key):
    _check_gradient(_record(cuda, key), key)


@pytest.mark.parametrize("key", FP32)
def test_identity(cuda, key):
    r = _record(cuda, key)
    off = r["off"]
    _, w = _reference(r)
    # p = 100 selects every weighted pixel
    s = r[100]
    assert s["launches"] > 0
    assert _same(s["out"], off["out"]) and _same(s["grad_un"], off["grad_un"])
    assert _same(s["dzscale"], off["dzscale"])
    want = 0.0 if (~w).any() else s["map"].min()
    assert _bits(s["tau"])[0] == _bits(np.float32(want))
    # fewer than K positive entries: tau = 0 and again the off outputs
    rw = br.l1_weight(r["cfg"], r["rect"])
    assert 0 < rw.mean() < 0.20
    a, b = r["rect_25"], r["rect_off"]
    assert _bits(a["tau"])[0] == 0
    assert _same(a["out"], b["out"]) and _same(a["grad_un"], b["grad_un"])
    assert _same(a["dzscale"], b["dzscale"])
    assert int(a["out"][4]) == int(rw.sum())
    # turned off again: no further launches, the off outputs
    z = r["off_again"]
    assert z["launches"] == r["rect_25"]["launches"] == len(PCTS) + 3
    assert _same(z["out"], off["out"]) and _same(z["grad_un"], off["grad_un"])
    assert _same(z["dzscale"], off["dzscale"])


@pytest.mark.parametrize("key", FP32)
def test_deterministic(cuda, key):
    r = _record(cuda, key)
    a, b = r[25], r["25_again"]
    for f in ("out", "grad_un", "dzscale", "map", "tau"):
        assert _same(a[f], b[f]), f


def test_bf16_context(cuda):
    """16-bit storage: the logits the loss head reads are fp32 there too."""
    key = "64x128-bf16"
    r = _record(cuda, key)
    _check_map(r, key)
    _check_selection(r, key)
    _check_gradient(r, key)


# ---------------------------------------------------------------------------------------------
# the public layer
# ---------------------------------------------------------------------------------------------
def test_define_losses_bootstraps(cuda):
    from estimator.define_losses_hierarchical import define_losses
    from estimator.mode_keys import ModeKeys
    from input_pipelines.synthetic import batch
    from seg_hip import LIB, SegContext
    cfg = SHAPES["48x64"][0]
    direct = _record(cuda, "48x64")
    ctx = SegContext(depth=cfg.depth, pyramid=cfg.pyramid, height=cfg.height, width=cfg.width,
                     nb_pp=cfg.nb_pp, nb_pb=cfg.nb_pb, nb_pi=cfg.nb_pi, dtype="fp32",
                     weight_decay=cfg.weight_decay, bn_decay=cfg.bn_decay)
    ctx.load_params(direct["params"])
    data = batch(11, cfg.nb_pp, cfg.nb_pb, cfg.nb_pi, cfg.height, cfg.width)
    ctx.forward(torch.as_tensor(data["images"]).to(cuda))
    labels = {"prolabels_per_pixel": torch.as_tensor(data["px"]).to(cuda),
              "prolabels_per_bbox": torch.as_tensor(data["bbox"]).to(cuda)}
    off = define_losses(ModeKeys.TRAIN, {"_context": ctx}, labels, None,
                        SimpleNamespace(bootstrapping_percentage=-1)).counts()
    assert ctx.counter("bootstrap_launches") == 0
    on = define_losses(ModeKeys.TRAIN, {"_context": ctx}, labels, None,
                       SimpleNamespace(bootstrapping_percentage=25))
    assert ctx.counter("bootstrap_launches") == 1
    assert on.counts()[0] == int(direct[25]["out"][4])
    assert on.counts()[0] < off[0] == int(direct["off"]["out"][4])
    assert on.counts()[1:] == off[1:]
    assert _same(on["l1_segmentation"].cpu().numpy(), direct[25]["out"][1])
    # the C ABI refuses a percentage above 100 and names the flag
    rc = LIB.seg_set_bootstrap(ctx.h, 101)
    assert rc == -22
    assert b"bootstrapping_percentage" in LIB.seg_last_error(ctx.h)
    with pytest.raises(RuntimeError, match="bootstrapping_percentage"):
        ctx.set_bootstrap(101)
    assert ctx.counter("bootstrap_launches") == 1
    ctx.close()
    # a context without strong images accepts the call and does nothing
    weak = SegContext(pyramid="none", height=48, width=64, nb_pp=0, nb_pb=1, dtype="fp32")
    weak.set_bootstrap(25)
    with pytest.raises(RuntimeError, match="never enabled"):
        weak.debug_tensor("l1_loss_map")
    weak.close()
