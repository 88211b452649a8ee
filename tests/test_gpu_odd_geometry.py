"""Odd-size geometry, layer by layer in 16-bit storage, forward glue included.

The reference trains Vistas at 621 x 855 (neither dimension a multiple of 8), where every
stride-2 stage but the first sees an odd or a padded input. Two small shapes reproduce every
parity case of that size and of its all-odd sibling, with the PSP grids still at 1 / 2 / 3 / 6
cells:

| image     | after conv1 | after pool (pads h, w) | features | H//8, W//8 | PSP windows                  |
| 101 x 103 | 51 x 52     | 26 x 26 (1, 0)         | 13 x 13  | 12, 12     | (12,12) (6,6) (4,4) (2,2)    |
| 97 x 145  | 49 x 73     | 25 x 37 (1, 1)         | 13 x 19  | 12, 18     | (12,18) (6,9) (4,6) (2,3)    |

101 x 103 is 621 x 855's class (5, 7 mod 8): the mixed pool pads, the PSP windows computed from
(H // 8, W // 8) on a map one row and one column larger (last row and column dropped). At
97 x 145 block1's strided 3 x 3 and the identity shortcut read at stride 2 see odd 25 x 37
inputs. The 16-bit stem is the space-to-depth one, whose last s2d row / column is half outside
the padded image; the padded max-pool runs unfused (BN apply, then the pool) and its backward
takes the padded row kernel; M = 3 * 13 * 19 = 741 pixels are no multiple of any tile.

``test_step_chain_odd`` runs tests/step_chain.py (every conv, the backward chain, the forward
links, the loss head with the weak-label mix) at these shapes in bf16 and fp16, plus the even
64 x 128 control (a failure there would be about the links, not the geometry). BN-backward
outputs: L2-relative 2e-2, the project's number at small sizes (test_bf16_backward_layerwise);
pyramid branches normalised over fewer than 64 samples per channel: max(2e-2, 4 gap), skipped
by name where 4 gap > 0.5 (step_chain's docstring; the gap table and the measured margins are
in profiles/odd_geometry_margins.txt). The per-256-pixel-tile 5e-2 stays a full-size check.

``test_vistas_crop_geometry`` creates the 621 x 855 context itself (no step) and compares every
conv's input / output dims with the oracle's own geometry.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle.tfseg import (SegConfig, build_specs, conv_tf, maxpool_same_3x3s2, psp_grids, resnet_units,
                          same_pads)
from step_chain import PM, step_chain

pytestmark = pytest.mark.gpu

# image -> conv1 output, pool output, pool pads (h, w), feature map, PSP windows
GEOMETRY = {
    (101, 103): ((51, 52), (26, 26), (1, 0), (13, 13), [(12, 12), (6, 6), (4, 4), (2, 2)]),
    (97, 145): ((49, 73), (25, 37), (1, 1), (13, 19), [(12, 18), (6, 9), (4, 6), (2, 3)]),
    (64, 128): ((32, 64), (16, 32), (0, 0), (8, 16), [(8, 16), (4, 8), (2, 5), (1, 2)]),   # even control
}
CASES = [(hw, pyr, dt) for hw in ((101, 103), (97, 145)) for pyr in ("psp", "aspp") for dt in ("bf16", "fp16")] + \
    [((64, 128), "psp", "bf16")]


@pytest.mark.parametrize("hw,pyramid,dtype", CASES, ids=[f"{h}x{w}-{p}-{d}" for (h, w), p, d in CASES])
def test_step_chain_odd(cuda, hw, pyramid, dtype):
    H, W = hw
    cfg = SegConfig(depth=50, height=H, width=W, nb_pp=1, nb_pb=1, nb_pi=1, pyramid=pyramid)
    rep = {}
    try:
        step_chain(cuda, cfg, dtype, param_seed=7, data_seed=13,
                   loss_scale=1024.0 if dtype == "fp16" else None, links=True,
                   bn_tol=2e-2, tile_tol=None, few_sample_gap=True, report=rep)
    finally:
        _print_margins(f"{H}x{W}-{pyramid}-{dtype}", rep)
    # ---- the geometry this case is here for
    conv1, pool, pads, feat, windows = GEOMETRY[hw]
    specs = build_specs(cfg)
    idx = {s.name: i for i, s in enumerate(specs)}
    dims = rep["dims"]
    hw_of = lambda name: tuple(dims[name][1:3])
    rn = "feature_extractor/base/resnet_v1_50"
    assert hw_of("conv0_x") == (H, W) and hw_of("conv0_y") == conv1 and hw_of("z0") == conv1
    first = idx[f"{rn}/block1/unit_1/bottleneck_v1/conv1"]
    assert hw_of(f"conv{first}_x") == pool
    assert (same_pads(conv1[0], 3, 2)[0], same_pads(conv1[1], 3, 2)[0]) == pads
    strided = idx[f"{rn}/block1/unit_3/bottleneck_v1/conv2"]
    assert hw_of(f"conv{strided}_x") == pool and hw_of(f"conv{strided}_y") == feat
    idfd = idx["feature_extractor/extension/decrease_fdims"]
    assert hw_of(f"conv{idfd}_x") == feat and hw_of(f"conv{idfd}_y") == feat
    assert psp_grids(H, W) == windows
    if hw != (64, 128):
        assert feat[0] == H // 8 + 1 or feat[1] == W // 8 + 1
    if pyramid == "psp":
        assert rep["psp_grids"] == windows
        cells = [hw_of(f"conv{idx[f'{PM}/{nm}']}_x") for nm in ("Conv", "Conv_1", "Conv_2", "Conv_3")]
        if hw != (64, 128):
            assert cells == [(1, 1), (2, 2), (3, 3), (6, 6)]
        assert cells == [((feat[0] - kh) // kh + 1, (feat[1] - kw) // kw + 1) for kh, kw in windows]
    # only the one-sample-per-image branch may have been skipped (step_chain asserts the names)
    assert len(rep["skipped"]) <= 1


def _print_margins(case, rep):
    """The figures of profiles/odd_geometry_margins.txt (shown with pytest -s / on failure)."""
    links = rep.get("link_excess", {})
    if links:
        worst = max(links, key=links.get)
        print(f"\n[margins] {case}: forward links {len(links)}, worst err/bound {links[worst]:.3f} ({worst})")
    bn = {k: v for k, v in rep.get("bn_bwd", {}).items() if v[0] is not None}
    if bn:
        worst = max(bn, key=lambda k: bn[k][0])
        print(f"[margins] {case}: BN backward {len(bn)}, worst rel {bn[worst][0]:.3e} ({worst}, "
              f"gap {bn[worst][1]:.2e}, tolerance {bn[worst][2]:.2e})")
    for k, (rel, gap, tol) in rep.get("bn_bwd", {}).items():
        if k.startswith(PM + "/"):
            print(f"[margins] {case}: {k}: rel {'skipped' if rel is None else f'{rel:.3e}'} gap {gap:.3e}"
                  + ("" if tol is None else f" tolerance {tol:.2e}"))


def _oracle_dims(cfg):
    """(x, y) spatial dims of every conv from the oracle's own geometry: conv_tf on one-channel
    zero tensors, maxpool_same_3x3s2, psp_grids and avg_pool2d (VALID, remainders dropped)."""
    def conv(hw, s):
        y = conv_tf(torch.zeros(1, 1, *hw), torch.zeros(1, s.k, s.k, 1), s)
        return tuple(y.shape[2:])
    specs = build_specs(cfg)
    by = {s.name: s for s in specs}
    out = {}

    def run(name, hw):
        out[name] = (hw, conv(hw, by[name]))
        return out[name][1]

    def unit(scope, hw):
        if f"{scope}/shortcut" in by:
            run(f"{scope}/shortcut", hw)
        return run(f"{scope}/conv3", run(f"{scope}/conv2", run(f"{scope}/conv1", hw)))

    rn = f"feature_extractor/base/resnet_v1_{cfg.depth}"
    hw = run(f"{rn}/conv1", (cfg.height, cfg.width))
    hw = tuple(maxpool_same_3x3s2(torch.zeros(1, 1, *hw)).shape[2:])
    for u in resnet_units(cfg.depth, cfg.output_stride):
        hw = unit(f"{rn}/{u[0]}", hw)
    hw = run("feature_extractor/extension/decrease_fdims", hw)
    assert cfg.pyramid == "psp"
    for (kh, kw), nm in zip(psp_grids(cfg.height, cfg.width), ("Conv", "Conv_1", "Conv_2", "Conv_3")):
        run(f"{PM}/{nm}", tuple(F.avg_pool2d(torch.zeros(1, 1, *hw), (kh, kw), stride=(kh, kw)).shape[2:]))
    run(f"{PM}/Conv_4", hw)
    for h in ("l1", "l2_vehicle", "l2_human"):
        unit(f"adaptation_module/{h}_features", hw)
        run(f"softmax_classifier/{h}_logits", hw)
    return [out[s.name] for s in specs]


def test_vistas_crop_geometry(cuda):
    """seg_create accepts the reference's own Vistas crop (621 x 855) and agrees with the oracle
    on every conv's input and output dims. No step runs at this size: the small shapes above
    carry the numerics of its parity class."""
    from seg_hip import SegContext
    H, W = 621, 855
    cfg = SegConfig(depth=50, height=H, width=W, nb_pp=1, pyramid="psp")
    ref = _oracle_dims(cfg)
    specs = build_specs(cfg)
    idx = {s.name: i for i, s in enumerate(specs)}
    rn = "feature_extractor/base/resnet_v1_50"
    assert ref[0] == ((621, 855), (311, 428))
    assert ref[idx[f"{rn}/block1/unit_1/bottleneck_v1/conv1"]][0] == (156, 214)
    assert ref[idx["feature_extractor/extension/decrease_fdims"]][1] == (78, 107)
    assert psp_grids(H, W) == [(77 // k, 106 // k) for k in (1, 2, 3, 6)]
    assert [ref[idx[f"{PM}/{nm}"]][0] for nm in ("Conv", "Conv_1", "Conv_2", "Conv_3")] == \
        [(1, 1), (2, 2), (3, 3), (6, 6)]
    ctx = SegContext(depth=50, pyramid="psp", height=H, width=W, nb_pp=1, dtype="bf16")
    try:
        for i, s in enumerate(specs):
            x, y = ctx.debug_dims(f"conv{i}_x"), ctx.debug_dims(f"conv{i}_y")
            assert (x[1:3], y[1:3]) == ref[i], (s.name, x, y, ref[i])
            assert x[::3] == (1, s.ci) and y[::3] == (1, s.co), (s.name, x, y)
    finally:
        ctx.close()
