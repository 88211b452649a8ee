"""Host checks of the bootstrapped l1 loss semantics (tests/bootstrap_ref.py, the float64
restatement the GPU tests compare against) and of the settings validation."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bootstrap_ref as br
from oracle.tfseg import OracleNet, SegConfig, init_params


def test_k_formula():
    assert br.k_of(1, 3) == 1                      # 1 % of 3 pixels rounds down to 0 -> at least 1
    assert br.k_of(100, 3) == 3
    assert br.k_of(100, 48 * 64) == 48 * 64
    M = 4 * 1024 * 2048                            # 8.4 M entries: p * M exceeds 2^31 from p = 1 up
    assert br.k_of(25, M) == M // 4 == 2097152
    assert br.k_of(1, M) == 83886
    assert br.k_of(99, M) == (99 * M) // 100 == 8304721
    assert br.k_of(100, M) == M
    with pytest.raises(ValueError):
        br.k_of(101, M)


def _synthetic(cfg, seed, labels):
    rng = np.random.default_rng(seed)
    hl, wl = cfg.height // 8, cfg.width // 8
    low = {"l1_logits": torch.as_tensor(rng.normal(0, 2, (cfg.nb, 14, hl, wl))),
           "l2_vehicle_logits": torch.as_tensor(rng.normal(0, 2, (cfg.nb, 7, hl, wl))),
           "l2_human_logits": torch.as_tensor(rng.normal(0, 2, (cfg.nb, 3, hl, wl)))}
    return low, labels


@pytest.fixture(scope="module")
def net():
    cfg = SegConfig(height=48, width=64, nb_pp=2, pyramid="none")
    return OracleNet(cfg, init_params(cfg, seed=0))


def _labels(cfg, seed, valid_box=None):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 20, size=(cfg.nb_pp, cfg.height, cfg.width)).astype(np.int32)
    if valid_box is not None:   # everything void (19) but a rectangle
        y0, y1, x0, x1 = valid_box
        keep = lab[:, y0:y1, x0:x1].copy()
        keep[keep == 19] = 3
        lab[:] = 19
        lab[:, y0:y1, x0:x1] = keep
    return lab


def test_p100_equals_oracle(net):
    cfg = net.cfg
    low, lab = _synthetic(cfg, 1, _labels(cfg, 2))
    L = net.losses(low, lab)
    m, tau, mask, k = br.bootstrap(cfg, low["l1_logits"], lab, 100)
    w = br.l1_weight(cfg, lab)
    assert k == m.size and (~w).any()
    assert tau == 0.0                      # an unweighted pixel exists: the minimum is its 0
    assert (mask == w).all()
    B = br.losses_with_mask(net, low, lab, None, None, mask)
    assert B["counts"] == tuple(L["counts"])
    assert float(B["l1_segmentation"]) == float(L["l1_segmentation"])
    assert float(B["segmentation"]) == float(L["segmentation"])


def test_few_labelled_pixels_equals_oracle(net):
    """A rectangle of valid pixels covering under 20 % of the image: fewer than K = 25 % of the
    entries are positive, tau = 0 and every weighted pixel is selected."""
    cfg = net.cfg
    low, lab = _synthetic(cfg, 3, _labels(cfg, 4, valid_box=(5, 25, 10, 40)))
    w = br.l1_weight(cfg, lab)
    assert 0 < w.mean() < 0.20
    L = net.losses(low, lab)
    m, tau, mask, k = br.bootstrap(cfg, low["l1_logits"], lab, 25)
    assert tau == 0.0 and (mask == w).all() and mask.sum() < k
    B = br.losses_with_mask(net, low, lab, None, None, mask)
    assert B["counts"][0] == L["counts"][0] == int(w.sum())
    assert float(B["l1_segmentation"]) == float(L["l1_segmentation"])


def test_selection_and_autograd(net):
    cfg = net.cfg
    low, lab = _synthetic(cfg, 5, _labels(cfg, 6))
    m, tau, mask, k = br.bootstrap(cfg, low["l1_logits"], lab, 25)
    assert (m >= 0).all() and tau > 0
    assert k <= mask.sum() == (m >= tau).sum()          # ties all selected; tau > 0 => weighted
    assert (m > tau).sum() < k
    assert np.isclose(m[mask].mean(), float(br.losses_with_mask(net, low, lab, None, None, mask)["l1_segmentation"]))
    lw = {kk: v.clone().requires_grad_(True) for kk, v in low.items()}
    br.losses_with_mask(net, lw, lab, None, None, mask)["segmentation"].backward()
    g = lw["l1_logits"].grad
    assert g is not None and float(g.abs().sum()) > 0
    # an all-void image contributes nothing to the l1 gradient
    lab2 = lab.copy()
    lab2[1] = 19
    _, _, mask2, _ = br.bootstrap(cfg, low["l1_logits"], lab2, 25)
    lw = {kk: v.clone().requires_grad_(True) for kk, v in low.items()}
    br.losses_with_mask(net, lw, lab2, None, None, mask2)["l1_segmentation"].backward()
    assert float(lw["l1_logits"].grad[1].abs().sum()) == 0.0


def _settings(p):
    return SimpleNamespace(height_network=64, width_network=128, height_feature_extractor=64,
                           width_feature_extractor=128, learning_rate_schedule="schedule_3",
                           training_problem_def={"lids2cids": [0, 1, 2, -1]},
                           bootstrapping_percentage=p)


def test_validation():
    from system_factory import _validate_settings
    with pytest.raises(ValueError, match="bootstrapping_percentage"):
        _validate_settings(_settings(101))
    for p in (-1, 0, 1, 100):
        _validate_settings(_settings(p))
    assert not br.is_on(0) and not br.is_on(-1) and br.is_on(1) and br.is_on(100)
    with pytest.raises(ValueError):
        br.is_on(101)


def test_estimator_configures_context_once():
    """configure_bootstrap: 0 and -1 leave an off context untouched, a percentage is set once,
    and 101 raises before reaching the library."""
    from estimator.define_losses_hierarchical import configure_bootstrap

    class Ctx:
        def __init__(self):
            self.calls = []

        def set_bootstrap(self, p):
            self.calls.append(p)
            self.bootstrap = p if p > 0 else -1

    c = Ctx()
    for p in (-1, 0):
        configure_bootstrap(c, SimpleNamespace(bootstrapping_percentage=p))
    configure_bootstrap(c, None)
    assert c.calls == []
    for _ in range(3):
        configure_bootstrap(c, SimpleNamespace(bootstrapping_percentage=25))
    assert c.calls == [25]
    configure_bootstrap(c, SimpleNamespace(bootstrapping_percentage=-1))
    assert c.calls == [25, -1]
    with pytest.raises(ValueError, match="bootstrapping_percentage"):
        configure_bootstrap(c, SimpleNamespace(bootstrapping_percentage=101))
