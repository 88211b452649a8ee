"""CPU only: the BN-backward conditioning table of tests/test_gpu_odd_geometry.py.

For every case of that test, one float64 oracle step (the same seeded weights and synthetic
batch), then per BN layer the gap of tests/step_chain.py: the L2-relative difference between
the float64 BN backward of the oracle's own gradient and of that gradient rounded once to the
storage dtype (fp16 under the test's loss scale of 1024). No native code runs. Prints every
layer whose gap is above 5e-3 (a quarter of the 2e-2 tolerance), all pyramid-module layers, and
the worst of the rest; the table goes into profiles/odd_geometry_margins.txt.

    python tools/odd_geometry_gaps.py
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"),
          os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from input_pipelines.synthetic import batch  # noqa: E402
from oracle.tfseg import OracleNet, SegConfig, init_params  # noqa: E402
from step_chain import FEW_SAMPLES, PM, bn_bwd_gap  # noqa: E402


class Recording(OracleNet):
    """Keeps every conv's output y and its BN [+ ReLU] output (whose .grad is the layer's dz)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ys, self.outs = {}, {}

    def conv_bn(self, x, name, relu=None, record=None):
        out = super().conv_bn(x, name, relu=relu, record=self.ys)
        out.retain_grad()
        self.outs[name] = out
        return out


def gaps(cfg, dtype, loss_scale):
    params = {k: v.astype(np.float32) for k, v in init_params(cfg, seed=7).items()}
    data = batch(13, cfg.nb_pp, cfg.nb_pb, cfg.nb_pi, cfg.height, cfg.width)
    net = Recording(cfg, params)
    net._trainable()
    low = net.forward(torch.as_tensor(data["images"]))
    net.losses(low, data["px"], data["bbox"], data["tag"])["segmentation"].backward()
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    rows = []
    for s in net.specs:
        y, out = nhwc(net.ys[s.name]), net.outs[s.name]
        gamma = net.p[f"{s.name}/BatchNorm/gamma"].detach()
        _, gap = bn_bwd_gap(nhwc(out.grad) * loss_scale, y, nhwc(out) if s.relu else None, gamma, y, dtype)
        rows.append((s.name, y[..., 0].numel(), gap))
    return rows


def main():
    shapes = [(101, 103), (97, 145)]
    cases = [(hw, pyr, dt) for hw in shapes for pyr in ("psp", "aspp") for dt in ("bf16", "fp16")] + \
        [((64, 128), "psp", "bf16")]
    for (H, W), pyr, dt in cases:
        cfg = SegConfig(depth=50, height=H, width=W, nb_pp=1, nb_pb=1, nb_pi=1, pyramid=pyr)
        t0 = time.time()
        rows = gaps(cfg, dt, 1024.0 if dt == "fp16" else 1.0)
        print(f"# {H}x{W}-{pyr}-{dt}  (oracle step {time.time() - t0:.1f} s)")
        rest = [r for r in rows if not r[0].startswith(PM + "/")]
        worst = max(rest, key=lambda r: r[2])
        print(f"  worst outside the pyramid module: gap {worst[2]:.3e}  {worst[0]} ({worst[1]} samples)")
        for name, n, gap in rows:
            if name.startswith(PM + "/") or gap > 5e-3:
                note = ""
                if name.startswith(PM + "/") and n < FEW_SAMPLES:
                    note = "  skipped (4 gap > 0.5)" if 4 * gap > 0.5 else f"  tolerance {max(2e-2, 4 * gap):.2e}"
                print(f"  {name}: {n} samples per channel, gap {gap:.3e}{note}")


if __name__ == "__main__":
    main()
