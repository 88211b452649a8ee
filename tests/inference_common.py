"""What tests/test_gpu_tta.py and tests/test_gpu_window.py share: the cid maps, the norm-relative
error, the script loader, the moving-statistics set-up and the two module-scoped contexts (the
test modules import the fixtures by name, so each module gets its own instance)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")
PROBLEM = os.path.join(PKG, "problem_definitions", "cityscapes", "problem01.json")

# the maps of tests/test_gpu_eval.py (copied)
MAPS = {
    "identity": list(range(19)) + [-1],
    # merge some classes, ignore others (-1 -> void = max + 1)
    "merge": [0, 0, 1, 1, 2, -1, 3, 3, 4, 5, 6, 7, 7, 8, 8, 8, 9, 9, 9, -1],
}


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _script(name):
    spec = importlib.util.spec_from_file_location(f"seg_{name}_inference_gpu", os.path.join(PKG, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _realistic_moving_stats(ctx, images):
    """Moving statistics = the batch statistics of one training-mode forward (the gradient
    buffer's tail has the moving buffer's layout), so that the moving-statistics forward gives
    logits in the range a trained checkpoint gives."""
    ctx.set_bn_inference(False)
    ctx.forward(images)
    torch.cuda.synchronize()
    ctx.moving.copy_(ctx.grads[ctx.n_train:ctx.n_train + ctx.n_moving])
    ctx.params_updated()
    ctx.set_bn_inference(True)


@pytest.fixture(scope="module")
def city_ctx(cuda):
    """A 64 x 128 PSP fp32 context after a moving-statistics forward."""
    from input_pipelines.synthetic import batch
    from models.initializers import init_params
    from seg_hip import SegContext
    ctx = SegContext(pyramid="psp", height=64, width=128, nb_pp=2, dtype="fp32")
    ctx.load_params(init_params(ctx.param_info, seed=3))
    _realistic_moving_stats(ctx, torch.as_tensor(batch(99, 2, 0, 0, 64, 128)["images"]).to(cuda))
    ctx.forward(torch.as_tensor(batch(12, 2, 0, 0, 64, 128)["images"]).to(cuda))
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def vistas_ctx(cuda):
    """A 53 | 12 | 5 context of the synthetic logits' network size (its forward is not used)."""
    from seg_hip import SegContext
    ctx = SegContext(pyramid="none", height=64, width=128, nb_pp=2, dtype="fp32", dataset="vistas")
    yield ctx
    ctx.close()
