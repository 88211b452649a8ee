"""The float64 restatements of tests/step_chain.py, pinned on the CPU to the oracle's own ops and
their autograd at the odd sizes tests/test_gpu_odd_geometry.py runs them at (no GPU): the
SAME-padded 3x3 / 2 max-pool forward and backward with mixed, full and no pads, the BN [+
shortcut] [+ ReLU] forward and the BN backward."""
import pytest
import torch

from oracle.tfseg import BN_EPS, bn_train, maxpool_same_3x3s2, same_pads
from step_chain import _bn_bwd, _bn_fwd, _maxpool_bwd, _maxpool_fwd, _maxpool_pads, bn_bwd_gap

# conv1 outputs of 101 x 103 (pads 1, 0), 97 x 145 (1, 1), 64 x 128 (0, 0), and (0, 1)
POOL_SHAPES = [(51, 52), (49, 73), (32, 64), (12, 9)]


@pytest.mark.parametrize("hw", POOL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maxpool_restatement(hw):
    g = torch.Generator().manual_seed(hw[0])
    # ReLU-like input with many exact ties (zeros): the first maximum in scan order takes the
    # gradient, which is TF's MaxPoolGrad and torch's CPU max_pool2d backward alike
    z = torch.relu(torch.randn(2, hw[0], hw[1], 5, generator=g, dtype=torch.float64))
    z = (z * 4).round() / 4
    Ho, Wo = (hw[0] + 1) // 2, (hw[1] + 1) // 2
    assert _maxpool_pads(hw[0], hw[1], Ho, Wo) == (same_pads(hw[0], 3, 2)[0], same_pads(hw[1], 3, 2)[0])
    zt = z.permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = maxpool_same_3x3s2(zt)
    assert torch.equal(_maxpool_fwd(z), ref.detach().permute(0, 2, 3, 1))
    gy = torch.randn(2, Ho, Wo, 5, generator=g, dtype=torch.float64)
    ref.backward(gy.permute(0, 3, 1, 2))
    got = _maxpool_bwd(z, gy)
    assert torch.allclose(got, zt.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    # nothing is lost in the padding
    assert torch.allclose(got.sum((1, 2)), gy.sum((1, 2)), rtol=0, atol=1e-9)


@pytest.mark.parametrize("relu,shortcut", [(True, False), (False, False), (True, True)])
def test_bn_restatement(relu, shortcut):
    g = torch.Generator().manual_seed(3)
    y = torch.randn(3, 13, 19, 6, generator=g, dtype=torch.float64) * 2 + 0.5     # 741 pixels
    gamma = torch.rand(6, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(6, generator=g, dtype=torch.float64)
    s = torch.randn(3, 13, 19, 6, generator=g, dtype=torch.float64) if shortcut else None
    yt = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = bn_train(yt, gamma, beta)[0]
    if shortcut:
        out = out + s.permute(0, 3, 1, 2)
    if relu:
        out = torch.relu(out)
    got = _bn_fwd(y, gamma, beta, y, relu=relu, shortcut=s)
    assert torch.allclose(got, out.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    dz = torch.randn(3, 13, 19, 6, generator=g, dtype=torch.float64)
    out.backward(dz.permute(0, 3, 1, 2))
    z = got if relu else None
    ref = _bn_bwd(dz, y, z, gamma, y)
    assert torch.allclose(ref, yt.grad.permute(0, 2, 3, 1), rtol=1e-9, atol=1e-12)
    # the gap: zero for a gradient the storage dtype holds exactly, ~u for a random one, and
    # large where three samples per channel cancel nearly all of it
    exact = (dz * 8).round() / 8
    assert bn_bwd_gap(exact, y, z, gamma, y, "bf16")[1] == 0.0
    assert 1e-4 < bn_bwd_gap(dz, y, z, gamma, y, "bf16")[1] < 2.0 ** -8
    assert 1e-5 < bn_bwd_gap(dz, y, z, gamma, y, "fp16")[1] < 2.0 ** -11
    y3 = y[:, :1, :1]
    few = bn_bwd_gap(dz[:, :1, :1] + 10.0, y3, None, gamma, y3, "bf16")[1]
    assert few > 10 * bn_bwd_gap(dz, y, None, gamma, y, "bf16")[1]
    assert BN_EPS == 1.001e-5
