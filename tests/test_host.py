"""CPU tests of the host side: the C-ABI library loads and exports every declared symbol,
the ctypes struct mirrors the header, and the drop-in Python surface (argparse flags,
learning-rate schedule, per-tower batch split, gradient averaging over 2 gloo ranks)."""
import os
import re
import socket

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "seg_hip.h")


def _declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"\b(seg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import seg_hip
    for name in _declared():
        assert hasattr(seg_hip.LIB, name), name
    assert sorted(seg_hip.EXPORTED_SYMBOLS) == _declared()


def test_cfg_struct_matches_header():
    import seg_hip
    src = open(HEADER).read()
    body = src[src.index("typedef struct seg_cfg {"):src.index("} seg_cfg;")]
    fields = []
    for line in body.splitlines()[1:]:
        m = re.match(r"\s*(int|float)\s+([^;]+);", line)
        if m:
            fields += [n.strip() for n in m.group(2).split(",")]
    assert [f[0] for f in seg_hip.SegCfg._fields_] == fields


def test_train_arguments_match_reference_defaults():
    from estimator.mode_keys import ModeKeys
    from models.resnet50_extended_model_hierarchical import add_model_arguments
    from utils.utils import SemanticSegmentationArguments
    a = SemanticSegmentationArguments(mode=ModeKeys.TRAIN)
    add_model_arguments(a.argparser)
    s = a.parse_args(["/tmp/log", "cityscapes", "--psp_module"])
    assert (s.Nb, s.Ne, s.learning_rate_initial, s.learning_rate_boundaries) == (4, 17, 0.01, [8, 15, 17])
    assert (s.regularization_weight, s.momentum, s.ema_decay, s.batch_norm_decay) == (0.00017, 0.9, 0.9, 0.9)
    assert (s.stride_feature_extractor, s.feature_dims_decreased, s.psp_module) == (8, 256, True)
    assert (s.height_feature_extractor, s.width_feature_extractor) == (512, 1024)


def test_learning_rate_schedule_piecewise_constant():
    from estimator.define_optimizer import define_optimizer

    class P:
        learning_rate_schedule = "piecewise_constant"
        learning_rate_boundaries = [10, 20]
        learning_rate_values = [0.01, 0.005, 0.0025]
        learning_rate_initial = 0.01
        learning_rate_final = 0.0
        learning_rate_power = 0.9
        optimizer = "SGDM"
        momentum = 0.9
        use_nesterov = False
    opt = define_optimizer(None, P)
    assert [opt.learning_rate(s) for s in (0, 10, 11, 20, 21)] == [0.01, 0.01, 0.005, 0.005, 0.0025]
    assert opt.momentum == 0.9


def test_facade_lr_boundaries_in_epochs():
    from system_factory import SemanticSegmentation
    from utils.utils import SemanticSegmentationArguments
    from models.resnet50_extended_model_hierarchical import add_model_arguments
    a = SemanticSegmentationArguments(mode="train")
    add_model_arguments(a.argparser)
    s = a.parse_args(["/tmp/x", "cityscapes", "--Ntrain", "400", "--Nb", "4"])
    s.training_problem_def_path = os.path.join(
        REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd",
        "problem_definitions", "cityscapes", "problem01.json")
    sys_ = SemanticSegmentation({}, None, s)
    assert sys_.settings.output_Nclasses == 20
    sys_._prepare_train_settings()
    st = sys_.settings
    assert st.num_batches_per_epoch == 100 and st.num_training_steps == 1700
    assert st.learning_rate_boundaries == [800, 1500]          # last boundary == Ne is dropped
    np.testing.assert_allclose(st.learning_rate_values, [0.01, 0.005, 0.0025])


def test_get_temp_nb():
    from input_pipelines.utils import get_temp_Nb

    class Cfg:
        class train_distribute:
            num_towers = 4
    assert get_temp_Nb(Cfg, 32) == 8
    with pytest.raises(AssertionError):
        get_temp_Nb(Cfg, 6)

    class One:
        train_distribute = None
    assert get_temp_Nb(One, 6) == 6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q, bucketed=False):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from estimator.define_estimator_hierarchical import allreduce_grads

    class Ctx:
        grads = torch.arange(12, dtype=torch.float32) * (rank + 1)

    class BucketCtx(Ctx):
        # ready order of a backward: weight ranges from the top down, then the BN tail
        @staticmethod
        def grad_buckets():
            return [(7, 10), (2, 7), (0, 2), (10, 12)]
    c = BucketCtx if bucketed else Ctx
    scale = allreduce_grads(c)
    q.put((rank, scale, (c.grads * scale).tolist()))
    dist.destroy_process_group()


@pytest.mark.parametrize("bucketed", [False, True])
def test_gradient_averaging_two_gloo_ranks(bucketed):
    """Per-tower gradients are SUM all-reduced then scaled by 1/N (MirroredStrategy mean);
    the bucketed path (the order seg_grad_buckets reports) gives the same mean."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, bucketed)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    exp = (np.arange(12) * 1 + np.arange(12) * 2) / 2.0
    for _, scale, g in res:
        assert scale == 0.5
        np.testing.assert_allclose(g, exp)


def test_initializer_matches_oracle_scheme():
    from models.initializers import init_params
    from oracle.tfseg import SegConfig, build_specs, init_params as oracle_init

    class PI:
        def __init__(self, name, kind, shape, numel):
            self.name, self.kind, self.shape, self.numel = name, kind, shape, numel
    cfg = SegConfig(depth=50, pyramid="psp")
    info = []
    for s in build_specs(cfg):
        info.append(PI(s.name + "/weights", "weights", (s.co, s.k, s.k, s.ci), s.co * s.k * s.k * s.ci))
        info.append(PI(s.name + "/BatchNorm/gamma", "gamma", (s.co,), s.co))
    ours = init_params(info, seed=7)
    ref = oracle_init(cfg, seed=7)
    for k in ours:
        np.testing.assert_allclose(ours[k].reshape(-1), ref[k].reshape(-1).astype(np.float32))


DP4 = dict(H=32, W=64, world=4)


def _dp4_cpu_worker(rank, port, q):
    """One rank of a world-size-4 data-parallel step on the CPU (gloo): this rank's share of
    the reference's 4 : 8 : 4 batch (train.rank_sub_batches under DistributeConfig(4), seeds
    of train.synthetic_seed), the oracle standing in for the device engine, and the host
    gradient exchange of the product (allreduce_grads over a flat [grads | BN-stat tail]
    buffer, bucket by bucket)."""
    try:
        import torch
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=DP4["world"])
        import train
        from estimator.define_estimator_hierarchical import allreduce_grads
        from input_pipelines.synthetic import batch
        from oracle.tfseg import OracleNet, SegConfig, init_params
        from system_factory import DistributeConfig
        from types import SimpleNamespace
        config = SimpleNamespace(train_distribute=DistributeConfig(DP4["world"]))
        params = SimpleNamespace(Nb_per_pixel=4, Nb_per_bbox=8, Nb_per_image=4)
        nb = train.rank_sub_batches(config, params)
        cfg = SegConfig(height=DP4["H"], width=DP4["W"], nb_pp=nb[0], nb_pb=nb[1], nb_pi=nb[2],
                        pyramid="none")
        d = batch(train.synthetic_seed(rank, 0), *nb, DP4["H"], DP4["W"])
        net = OracleNet(cfg, init_params(cfg, seed=0))
        L, _, g, _, _, _, st = net.train_step(d["images"], d["px"], d["bbox"], d["tag"])
        keys = sorted(g)
        skeys = sorted(st)
        flat = torch.cat([g[k].reshape(-1) for k in keys] +
                         [torch.cat([st[k][0].reshape(-1), st[k][1].reshape(-1)]) for k in skeys]).float()
        n_g = sum(g[k].numel() for k in keys)

        class Ctx:   # the bound flat buffer and the backward's bucket order (tail last)
            grads = flat.clone()

            @staticmethod
            def grad_buckets():
                return [(n_g // 2, n_g), (0, n_g // 2), (n_g, flat.numel())]
        scale = allreduce_grads(Ctx)
        q.put((rank, nb, float(L["segmentation"]), tuple(int(c) for c in L["counts"]),
               flat.numpy(), (Ctx.grads * scale).numpy(), None))
        dist.destroy_process_group()
    except Exception as e:
        import traceback
        q.put((rank, None, None, None, None, None, traceback.format_exc() + repr(e)))


def test_dp_four_ranks_mixed_batch_host_path():
    """VERDICT r3 item 5 on the CPU: at world size 4 each rank takes a quarter of EVERY
    sub-batch (1 strong + 2 bbox + 1 tag of the reference's 4 : 8 : 4, get_temp_Nb per
    stream), normalises its loss by its own non-zero-weight counts (they differ between the
    ranks, so a global normalisation would give other gradients), and the bucketed SUM
    all-reduce scaled by 1/4 yields, on every rank, exactly the mean of the four per-rank
    [gradients | BN batch statistics] buffers (fp32 sums of 4 values: within a few ulp of
    the sum of their magnitudes)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp4_cpu_worker, args=(r, port, q)) for r in range(DP4["world"])]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[6] is None, r[6]
    assert all(r[1] == [1, 2, 1] for r in res)
    assert len({r[3] for r in res}) > 1          # per-rank counts differ
    local = np.stack([r[4] for r in res]).astype(np.float64)
    mean = local.mean(0)
    bound = 4 * np.finfo(np.float32).eps * np.abs(local).sum(0) / 4 + 1e-30
    for r in res:
        assert np.all(np.abs(r[5] - mean) <= bound), float(np.max(np.abs(r[5] - mean) / bound))
        np.testing.assert_array_equal(r[5], res[0][5])


def _run_bench(args, env_extra, timeout=300):
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=timeout, cwd=repo)


def test_bench_world_size_must_match_gpus():
    """under an external launcher WORLD_SIZE must equal --gpus (a mismatch
    exits non-zero before anything touches a GPU)."""
    r = _run_bench(["--gpus", "4", "--steps", "1"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=2 but --gpus 4" in r.stderr, r.stderr
    assert '{"metric"' not in r.stdout


def test_bench_rejects_zero_timed_steps():
    """--steps is the number of timed steps: a run without one has no ms_per_step to report."""
    r = _run_bench(["--gpus", "1", "--steps", "0", "--warmup", "1"], {})
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr
    assert '{"metric"' not in r.stdout


def test_bench_launches_ranks_and_propagates_failure():
    """`bench.py --gpus 2` with no WORLD_SIZE starts two rank processes of itself (RANK /
    LOCAL_RANK / WORLD_SIZE / MASTER_* set, 127.0.0.1). Here (no GPU) both ranks fail at device
    selection: the parent must report the failing rank, print no result line and exit non-zero."""
    r = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"SEG_BENCH_BACKEND": "nccl"})
    assert r.returncode != 0
    assert '{"metric"' not in r.stdout
    assert "exited with" in r.stderr, r.stderr[-2000:]
    # each child saw its own rank environment (whichever rank failed first is reported)
    assert "LOCAL_RANK" in r.stderr and ("rank 0" in r.stderr or "rank 1" in r.stderr)


# ---- utils/launch.py: the self-launch of `bench.py --gpus N` and `train.py --distribute` ----
_RANK_SCRIPT = """
import os, sys, time
out = sys.argv[1]
r = int(os.environ["RANK"])
with open(os.path.join(out, f"r{r}.txt"), "w") as f:
    f.write(" ".join(os.environ[k] for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE",
                                               "MASTER_ADDR", "MASTER_PORT")) + " " + str(os.getpid()))
mode = sys.argv[2]
if mode == "fail1" and r == 1:
    sys.exit(3)
if mode in ("fail1", "sleep"):
    time.sleep(60)
"""


def _rank_script(tmp_path):
    p = tmp_path / "rank.py"
    p.write_text(_RANK_SCRIPT)
    return str(p)


def test_spawn_ranks_sets_rank_environment(tmp_path):
    import sys
    from utils.launch import spawn_ranks
    rc = spawn_ranks(3, [sys.executable, _rank_script(tmp_path), str(tmp_path), "ok"])
    assert rc == 0
    rows = [(tmp_path / f"r{r}.txt").read_text().split() for r in range(3)]
    assert [row[:5] for row in rows] == [[str(r), str(r), "3", "3", "127.0.0.1"] for r in range(3)]
    assert len({row[5] for row in rows}) == 1   # one rendezvous port


def test_spawn_ranks_failure_stops_the_others(tmp_path):
    import sys
    import time
    from utils.launch import spawn_ranks
    t0 = time.monotonic()
    rc = spawn_ranks(2, [sys.executable, _rank_script(tmp_path), str(tmp_path), "fail1"])
    assert rc == 3 and time.monotonic() - t0 < 30   # rank 0 (sleeping 60 s) was stopped


def test_spawn_ranks_deadline(tmp_path):
    import sys
    import time
    from utils.launch import spawn_ranks
    t0 = time.monotonic()
    rc = spawn_ranks(2, [sys.executable, _rank_script(tmp_path), str(tmp_path), "sleep"], deadline_s=1.0)
    assert rc == 124 and time.monotonic() - t0 < 30


def test_spawn_ranks_forwards_sigterm(tmp_path):
    """a signal to the launching process (e.g. `timeout` ending bench.py --gpus N)
    reaches every rank; the parent exits 128 + SIGTERM and no rank is left running."""
    import signal
    import subprocess
    import sys
    import time
    parent = tmp_path / "parent.py"
    parent.write_text(
        "import sys\n"
        f"sys.path.insert(0, {os.path.join(REPO, 'iv2019-boosting-semantic-segmentation-with-weak-labels_amd')!r})\n"
        "from utils.launch import spawn_ranks\n"
        f"sys.exit(spawn_ranks(2, [sys.executable, {_rank_script(tmp_path)!r}, {str(tmp_path)!r}, 'sleep']))\n")
    p = subprocess.Popen([sys.executable, str(parent)])
    for _ in range(200):
        if all((tmp_path / f"r{r}.txt").exists() for r in range(2)):
            break
        time.sleep(0.1)
    time.sleep(0.3)
    pids = [int((tmp_path / f"r{r}.txt").read_text().split()[-1]) for r in range(2)]
    p.send_signal(signal.SIGTERM)
    assert p.wait(timeout=40) == 128 + signal.SIGTERM
    for pid in pids:
        alive = True
        for _ in range(50):
            try:
                os.kill(pid, 0)
                with open(f"/proc/{pid}/stat") as f:
                    if f.read().split()[2] == "Z":
                        alive = False
                        break
            except (ProcessLookupError, FileNotFoundError):
                alive = False
                break
            time.sleep(0.1)
        assert not alive, pid


def test_train_distribute_self_launch_propagates_failure(tmp_path):
    """`train.py --distribute` without WORLD_SIZE starts its ranks itself (SEG_TRAIN_RANKS=2
    here); with no GPU both fail at device selection, and the launch must fail, naming the
    failing rank, instead of hanging or exiting 0."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SEG_TRAIN_RANKS="2")
    train_py = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd", "train.py")
    r = subprocess.run([sys.executable, train_py, str(tmp_path / "logs"), "cityscapes", "--max_steps", "1",
                        "--distribute"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "exited with" in r.stderr and "a rank failed" in r.stderr, r.stderr[-3000:]


def test_bn_op_structs_match_header(tmp_path):
    """seg_bn_apply_args / seg_bn_bwd_args in ctypes lay out as a C compiler lays out the header's"""
    import ctypes
    import subprocess
    import seg_hip
    pairs = [("seg_bn_apply_args", seg_hip.BnApplyArgs), ("seg_bn_bwd_args", seg_hip.BnBwdArgs)]
    body = "".join(f'printf("%zu", sizeof({c}));' + "".join(
        f'printf(" %zu", offsetof({c}, {f[0]}));' for f in s._fields_) + 'printf("\\n");' for c, s in pairs)
    src = tmp_path / "layout.c"
    src.write_text('#include "seg_hip.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   f"int main(void) {{ {body} return 0; }}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for (c, s), line in zip(pairs, lines):
        want = [ctypes.sizeof(s)] + [getattr(s, f[0]).offset for f in s._fields_]
        assert [int(v) for v in line.split()] == want, c


def test_bn_op_entries_validate_before_any_launch():
    """no GPU is touched: the row-block count, and -EINVAL with a text for null / bad arguments"""
    import ctypes
    import errno
    import seg_hip
    L = seg_hip.LIB
    assert [L.seg_op_bn_rowblocks(m, 64) for m in (1, 64, 65, 391, 65536, 66000)] == [1, 1, 2, 7, 1024, 1024]
    assert L.seg_op_bn_rowblocks(0, 64) == -errno.EINVAL
    assert L.seg_op_bn_stats_finalize(None, 10, 8, 64, None, None, None, None, None, None, None) == -errno.EINVAL
    assert b"seg_op_bn_stats_finalize" in L.seg_last_error(None)
    assert L.seg_op_bn_apply(1, 0, None, None) == -errno.EINVAL
    a = seg_hip.BnApplyArgs()
    assert L.seg_op_bn_apply(1, 0, ctypes.byref(a), None) == -errno.EINVAL
    b = seg_hip.BnBwdArgs()
    assert L.seg_op_bn_backward(7, 0, 0, 0, ctypes.byref(b), None) == -errno.EINVAL
    assert L.seg_op_bn_backward_dual(1, 0, 0, ctypes.byref(b), None, None) == -errno.EINVAL
    assert b"seg_op_bn_backward_dual" in L.seg_last_error(None)
