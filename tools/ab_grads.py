"""One training step's gradients, losses and low-res logits from the working-tree library and
from an A/B build (SEG_HIP_LIB), each in its own child process: max difference per tensor class
(conv weights, BN gammas / betas by parameter kind; losses; logits).
    python tools/ab_grads.py ab/<variant>/libseg_hip.so [dtype pyramid height width nb_pp,nb_pb,nb_pi] [--self]
Default: the C2 step (bf16 aspp 1024 2048 4,0,0). --self runs the A/B build against itself: which
tensor classes repeat from run to run at all."""
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import os, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from input_pipelines.synthetic import batch
from models.initializers import init_params
from seg_hip import SegContext
dtype, pyramid, H, W = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
npp, npb, npi = (int(v) for v in sys.argv[6].split(","))
ctx = SegContext(depth=50, pyramid=pyramid, height=H, width=W, nb_pp=npp, nb_pb=npb, nb_pi=npi, dtype=dtype)
ctx.load_params(init_params(ctx.param_info, seed=0))
d = batch(1000, npp, npb, npi, H, W)
dev = lambda k: torch.as_tensor(d[k]).cuda()
ctx.forward(dev("images"))
ctx.loss(dev("px") if npp else None, dev("bbox") if npb else None, dev("tag") if npi else None)
ctx.backward(); torch.cuda.synchronize()
losses, _, logits = ctx.outputs()
KINDS = ["batch-statistics tail", "weights", "gamma", "beta", "biases"]
kinds = np.zeros(ctx.grads.numel(), np.int8)
for p in ctx.param_info:
    if p.kind in KINDS:
        kinds[p.offset:p.offset + p.numel] = KINDS.index(p.kind)
np.savez(sys.argv[1], grads=ctx.grads.cpu().numpy(), losses=losses.cpu().numpy(),
         logits=logits.float().cpu().numpy(), kinds=kinds)
print("losses", losses.cpu().numpy()[:4])
"""


def run(lib, out, cfg):
    env = dict(os.environ)
    env.pop("SEG_HIP_LIB", None)
    if lib:
        env["SEG_HIP_LIB"] = lib
    src = CHILD % (REPO, os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd"))
    r = subprocess.run([sys.executable, "-c", src, out] + cfg, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout.strip(), r.stderr.strip()[-300:])
    r.check_returncode()
    return np.load(out)


own = "--self" in sys.argv
if own:
    sys.argv.remove("--self")
cfg = sys.argv[2:7] if len(sys.argv) >= 7 else ["bf16", "aspp", "1024", "2048", "4,0,0"]
a = run(os.path.abspath(sys.argv[1]) if own else None, "/tmp/ab_grads_a.npz", cfg)
print("A/B build against itself" if own else "working tree against the A/B build")
b = run(os.path.abspath(sys.argv[1]), "/tmp/ab_grads_b.npz", cfg)
worst = 0.0
for name in ("losses", "logits"):
    d = float(np.abs(a[name].astype(np.float64) - b[name]).max())
    worst = max(worst, d)
    print(f"{' '.join(cfg)} {name}: max |a-b| {d:.3e}")
for kind in np.unique(a["kinds"]):
    sel = a["kinds"] == kind
    d = float(np.abs(a["grads"][sel].astype(np.float64) - b["grads"][sel]).max())
    worst = max(worst, d)
    name = ["batch-statistics tail", "weights", "gamma", "beta", "biases"][kind]
    print(f"{' '.join(cfg)} grads, {name} ({int(sel.sum())} values): max |a-b| {d:.3e}")
print(f"{' '.join(cfg)}: max difference {worst:.3e}, bitwise equal "
      f"{all(np.array_equal(a[k], b[k]) for k in ('grads', 'losses', 'logits'))}")
