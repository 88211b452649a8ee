"""Training-throughput benchmark of the MI355X path (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run does only what the headline figure needs: set-up, W warm-up steps, K timed steps,
the outputs of the last timed step to DIR (--dump-outputs) and the result line. --full adds,
outside the timed region, everything else this benchmark measures: the roofline object (one
extra profiled step after the timed ones), the training-summary mIoU, the EVAL path, the
train.py leg and the CPU baseline (each still switched off by its own --no-* option).

N > 1: `python bench.py --gpus N` launches N fresh rank processes itself (one per GPU, RCCL),
as the reference's --distribute takes every visible GPU in one launch (system_factory.py:
279-281); the parent never touches the GPU, re-prints rank 0's JSON line and fails if any rank
fails. Under an external launcher (python -m torch.distributed.run --nnodes=1 --nproc-per-node
N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...) WORLD_SIZE is set and must
equal --gpus.

Workload (BASELINE config C2, the metric's single-GPU configuration): ResNet-50 dilated
(output stride 8) + ASPP (as C2 names it; the reference's commented-out _create_aspp_module,
hierarchical.py:209-226 -- `--pyramid psp` runs the reference's live PSP module instead),
1024x2048 crops, 4 per-pixel-labelled images per GPU, bf16
storage with fp32 accumulation, synthetic seeded data resident in HBM. One step = forward +
fused multi-loss head + backward + gradient all-reduce (RCCL, N>1) + fused SGDM/L2/BN
moving-average update + the EMA of the model variables (N=1: the reference's single-GPU
default, ema_decay 0.9; distributed runs drop it, as the reference does). Weak scaling: 4
images per GPU at every N.

Prints ONE JSON line (rank 0) with the metric and `ms_per_step`; with --full also a roofline
object for the dominant kernel class (HIP-event timed in one extra step after the timed
region) and the CPU baseline (the oracle — a PyTorch-CPU fp32 restatement of the reference
semantics — timed on this host's cores). The fields of the --full legs are null in a plain run.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")
sys.path[:0] = [REPO, PKG]

H, W, NB = 1024, 2048, 4
# BASELINE.json configs as per-GPU workloads (4 images per GPU; weak scaling). C4/C5 keep the
# reference's 1 : 2 : 1 pixel : bbox : tag proportion (train.py:62-64); C5 runs fp16 storage
# with fp32 master weights / gradients and dynamic loss scaling (DynamicLossScaler). C1 is the
# reference's own CPU-runnable case (R50, no pyramid -- train.py's default -- 512 x 1024,
# batch 2), run here on the GPU for completeness.
CONFIGS = {
    "C1": {"depth": 50, "mix": (2, 0, 0), "hw": (512, 1024), "pyramid": "none",
           "name": "C1: ResNet-50 dilated OS8"},
    "C2": {"depth": 50, "mix": (4, 0, 0), "name": "C2: ResNet-50 dilated OS8"},
    "C3": {"depth": 101, "mix": (4, 0, 0), "name": "C3: ResNet-101 dilated OS8"},
    "C4": {"depth": 101, "mix": (2, 2, 0), "name": "C4: ResNet-101 dilated OS8, strong + bbox-weak"},
    "C5": {"depth": 101, "mix": (1, 2, 1), "dtype": "fp16",
           "name": "C5: ResNet-101 dilated OS8, per-pixel + bbox + tag, fp16 + fp32 master"},
}
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_TBS = 8.0          # MI355X HBM3E peak (MI355X_MICROARCH.md)
# the kernels each profiled class launches (rocprofv3 names: conv_nt_pp_kernel for Co > 128,
# conv_nt_v2_kernel for Co <= 128 and the tap8 stem; conv_wgrad_pp_kernel for 256 x 256 tiles,
# conv_wgrad_v2_kernel below; fp32 parity mode runs the v1 conv_nt_kernel / conv_wgrad_kernel)
CLS_NAMES = {0: "conv_nt_pp/v2_kernel (forward implicit GEMM)",
             1: "conv_nt_pp/v2_kernel (data-gradient)",
             2: "conv_wgrad_pp/v2_kernel (weight-gradient, split-K)",
             3: "bn_apply8_kernel (BN + ReLU + residual)", 4: "bn_bwd_reduce8_kernel",
             5: "bn_bwd_apply8_kernel"}
CLS_NAMES_F32 = {0: "conv_nt_kernel (fp32 MFMA forward)", 1: "conv_nt_kernel (fp32 MFMA data-gradient)",
                 2: "conv_wgrad_kernel (fp32 MFMA weight-gradient, split-K)"}
EMA_DECAY = 0.9   # utils/utils.py:112 default; off when distributed (system_factory.py:236-238)


def host_cpu_info():
    """Host CPU facts reported beside the CPU baseline: logical CPUs, the affinity set this
    process may run on, the cgroup v2 CPU quota (None = unlimited) and the CPU model."""
    info = {"cpu_count": os.cpu_count()}
    try:
        info["affinity"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        info["affinity"] = None
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = round(int(q) / int(per), 2)
    except (OSError, ValueError):
        pass
    info["cgroup_cpu_quota"] = quota
    model, sockets = None, set()
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model is None:
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                sockets.add(line.split(":", 1)[1].strip())
    except OSError:
        pass
    info["cpu_model"] = model
    info["sockets"] = len(sockets) or None
    return info


def baseline_threads(info):
    """Threads for the CPU baseline: every core this process may use. On the GPU box that is the
    cgroup CPU quota (16 of the 256 logical CPUs); more threads than the quota only contend for
    it (profiles/r03_cpu_threads.txt: the C1 step takes 6.3 s on 16, 7.7 s on 32, 11.0 s on 64)."""
    n = info.get("affinity") or info.get("cpu_count") or 1
    if info.get("cgroup_cpu_quota"):
        n = min(n, max(1, int(info["cgroup_cpu_quota"])))
    return n


def cpu_baseline(pyramid, reps=3):
    """Oracle (PyTorch-CPU fp32 restatement of the TF semantics) on the host cores, as SURVEY
    §8(d) / BASELINE.md plan it: one warm-up step at the timed shape, then the median of `reps`
    full training steps (fwd + loss + bwd + SGDM), at 1024x2048 batch 1 (the metric's image) and
    at C1 (the reference's own CPU configuration: R50, no pyramid, 512x1024, batch 2)."""
    import statistics
    import torch
    from input_pipelines.synthetic import batch
    from oracle.tfseg import OracleNet, SegConfig, init_params
    info = host_cpu_info()
    threads = baseline_threads(info)
    torch.set_num_threads(threads)

    def timed(cfg, d):
        net = OracleNet(cfg, init_params(cfg), dtype=torch.float32)
        net.train_step(d["images"], d["px"])          # warm-up at the timed shape
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            net.train_step(d["images"], d["px"])
            ts.append(time.perf_counter() - t)
        return statistics.median(ts), ts

    cfg = SegConfig(height=H, width=W, nb_pp=1, pyramid=pyramid)
    dt, ts = timed(cfg, batch(2, 1, 0, 0, H, W))
    c1 = SegConfig(height=512, width=1024, nb_pp=2, pyramid="none")
    d1, ts1 = timed(c1, batch(3, 2, 0, 0, 512, 1024))
    return {"value": round(1.0 / dt, 4), "unit": "images/sec", "cores": threads, "kind": "port",
            "cpu_model": info["cpu_model"], "cpu_count": info["cpu_count"],
            "cgroup_cpu_quota": info["cgroup_cpu_quota"], "sockets": info["sockets"],
            "sample": f"1 image 1024x2048, median of {reps} full steps (fwd+loss+bwd+SGDM) after "
                      f"1 warm-up step at that shape, R50+{pyramid.upper()}, fp32, oracle/tfseg.py "
                      f"(PyTorch CPU) on {threads} threads; steps " +
                      ", ".join(f"{t:.1f}" for t in ts) + " s",
            "c1": {"value": round(2.0 / d1, 4), "unit": "images/sec",
                   "sample": f"C1: R50 (no pyramid) 512x1024 batch 2, median of {reps} steps after 1 "
                             "warm-up; steps " + ", ".join(f"{t:.1f}" for t in ts1) + " s"}}


def train_py_leg(args, steps=10, warmup=3):
    """The drop-in trainer end to end: ``train.py``'s facade
    (SemanticSegmentation.train -> define_estimator -> model_fn / define_losses / train_op) on
    the bench's workload, timed over `steps` steps after `warmup` (system_factory's
    timing_warmup: synchronised clock, input pipeline included), twice:
    * real data: a 1024 x 2048 Cityscapes-format TFRecord written here (8 records: PNG image +
      label-id PNG, KEYS2FEATURES_v5), decoded on the host by the pool of
      input_pipelines/train_inputs.py, preprocessed on the device;
    * synthetic: train.synthetic_train_input's seeded batches, resident in HBM and cycled
      (a pool of `warmup` batches, generated on the host during the warm-up steps)."""
    import shutil
    import tempfile
    import numpy as np
    import train
    from estimator.define_estimator_hierarchical import get_or_create_global_step
    from input_pipelines.tfrecords import encode_example, encode_png, write_records
    from input_pipelines.train_inputs import default_workers
    from models import resnet50_extended_model_hierarchical as mh
    tmp = tempfile.mkdtemp(prefix="seg_trainpy_")
    try:
        rng = np.random.default_rng(5)
        recs = []
        t_gen = time.perf_counter()
        for i in range(8):
            # photo-like content (smooth 32 px blocks + small noise: ~3x PNG compression, as
            # Cityscapes' leftImg8bit PNGs) and blocky label ids 0..33
            base = rng.integers(0, 256, (H // 32, W // 32, 3), dtype=np.uint8).repeat(32, 0).repeat(32, 1)
            img = np.clip(base.astype(np.int16) + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
            lab = rng.integers(0, 34, (H // 32, W // 32), dtype=np.uint8).repeat(32, 0).repeat(32, 1)
            recs.append(encode_example({
                'image/encoded': [encode_png(img)], 'image/format': [b'png'],
                'image/shape': [H, W, 3], 'image/path': [f'img_{i}.png'.encode()],
                'label/encoded': [encode_png(lab[..., None])], 'label/format': [b'png'],
                'label/shape': [H, W, 1], 'label/path': [f'lab_{i}.png'.encode()]}))
        path = os.path.join(tmp, "cityscapes_1024x2048.tfrecord")
        write_records(path, recs)
        png_mb = sum(len(r) for r in recs) / len(recs) / 1e6
        t_gen = time.perf_counter() - t_gen
        out = {"decode_workers": default_workers(), "prefetch_batches": 2, "steps": steps,
               "warmup": warmup, "record_mb": round(png_mb, 2)}
        pyr = {"aspp": ["--aspp_module"], "psp": ["--psp_module"], "none": []}[args.pyramid]
        for mode in ("real_data", "synthetic"):
            mh.release_contexts()
            get_or_create_global_step().value = 0
            argv = [os.path.join(tmp, mode), "cityscapes", "--max_steps", str(warmup + steps),
                    "--compute_dtype", args.dtype, "--height_feature_extractor", str(H),
                    "--width_feature_extractor", str(W), "--Nb_per_pixel", str(NB),
                    "--Nb_per_bbox", "0", "--Nb_per_image", "0",
                    "--save_summaries_steps", "1000000", "--save_checkpoints_steps", "1000000"] + pyr
            if mode == "real_data":
                argv += ["--tfrecords_path_per_pixel", path]
            else:   # the resident pool fills during the warm-up steps (host generation)
                argv += ["--synthetic_pool", str(warmup)]
            system, _ = train.build_system(argv)
            system.train(max_steps=warmup + steps, log_fn=lambda *a: None, timing_warmup=warmup)
            tm = system.last_train_timing
            out[mode] = {"images_per_sec": round(tm["images"] / tm["seconds"], 3),
                         "ms_per_step": round(tm["seconds"] * 1e3 / tm["steps"], 2)}
            mh.release_contexts()
        out["images_per_sec"] = out["real_data"]["images_per_sec"]
        out["what"] = (f"train.py (SemanticSegmentation.train) on the bench workload, {NB} images/step; "
                       f"real_data: {len(recs)} generated 1024x2048 PNG TFRecords ({png_mb:.1f} MB "
                       f"each, written in {t_gen:.0f} s), host decode on {out['decode_workers']} "
                       "threads 2 batches ahead; synthetic: seeded batches resident in HBM")
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


DUMP_BUDGET_BYTES = 48 << 20   # all .npy files of one --dump-outputs together (limit: 64 MB)


def dump_outputs(ctx, out_dir):
    """--dump-outputs: what a caller of the timed step holds after its last step, as float32
    `out_dir/<name>.npy`: the losses, the regularisation value and the low-resolution logits
    (real class columns) of seg_outputs, and the state the update wrote (params, momentum, BN
    moving statistics, EMA). An array larger than its share of DUMP_BUDGET_BYTES is written as
    a fixed sample: the elements at sorted indices drawn once from a generator seeded by the
    array's length, so two builds sample the same elements."""
    import numpy as np
    import torch
    from seg_hip import DATASET
    losses, reg, logits = ctx.outputs()
    nc = sum((53, 12, 5) if ctx.cfg.dataset == DATASET["vistas"] else (14, 7, 3))
    arrays = {"losses": losses, "reg": reg, "logits": logits[..., :nc], "params": ctx.params,
              "momentum": ctx.momentum, "moving": ctx.moving}
    if ctx.ema is not None:
        arrays["ema"] = ctx.ema
    cap = DUMP_BUDGET_BYTES // 4 // len(arrays)   # float32 elements per array
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    for name, t in arrays.items():
        t = t.detach().float()
        if t.numel() > cap:
            idx = np.sort(np.random.default_rng(t.numel()).integers(0, t.numel(), cap))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy().astype(np.float32))


def launch_ranks(n, argv):
    """`bench.py --gpus N` without WORLD_SIZE: start N child processes of this script (never an
    exec of this one; utils/launch.spawn_ranks: rank r on GPU r, rendezvous on 127.0.0.1, the
    children in this process group, SIGTERM / SIGINT forwarded, a wall-clock deadline). Runs
    before anything in this process touches the GPU. Returns the exit code: 0 only if every
    rank exited 0 and rank 0 printed the JSON line (re-printed here on stdout). A failing rank
    stops the others."""
    import shutil
    import tempfile
    from utils.launch import spawn_ranks
    tmp = tempfile.mkdtemp(prefix="seg_bench_ranks_")
    outs = [open(os.path.join(tmp, f"rank{r}.out"), "w+") for r in range(n)]
    try:
        rc = spawn_ranks(n, [sys.executable, os.path.abspath(__file__)] + argv, outs=outs,
                         deadline_s=float(os.environ.get("SEG_BENCH_DEADLINE_S", "1800")), name="bench.py")
        line = None
        for r, out in enumerate(outs):
            out.seek(0)
            for ln in out.read().splitlines():
                if r == 0 and ln.startswith('{"metric"'):
                    line = ln
                else:
                    print(f"[rank {r}] {ln}", file=sys.stderr)
    finally:
        for out in outs:
            out.close()
        shutil.rmtree(tmp, ignore_errors=True)
    if rc == 0 and line is None:
        print("bench.py: rank 0 printed no result line", file=sys.stderr)
        rc = 1
    if line is not None and rc == 0:
        print(line, flush=True)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp16", "fp32"],
                    help="storage dtype (default: the config's; fp16 for C5, else bf16)")
    ap.add_argument("--pyramid", default=None, choices=["aspp", "psp", "none"],
                    help="default: the config's (ASPP as C2-C5 name it; none for C1)")
    ap.add_argument("--config", default="C2", choices=sorted(CONFIGS),
                    help="BASELINE.json workload preset (per-GPU share); C2 is the metric's")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs outside the headline figure: roofline profile, "
                         "training-summary mIoU, EVAL path, train.py leg, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--no-train-py", action="store_true",
                    help="skip the drop-in trainer leg (train.py on real and synthetic data)")
    ap.add_argument("--no-defer-stem", action="store_true",
                    help="A/B: join every weight gradient before the update (the N > 1 order)")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    # the legs beside the headline figure run under --full only
    do_profile = args.full and not args.no_profile
    do_eval = args.full and not args.no_eval
    do_train_py = args.full and not args.no_train_py
    do_cpu = args.full and not args.no_cpu_baseline
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}", file=sys.stderr)
        sys.exit(2)

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("SEG_BENCH_BACKEND", "nccl")
    # one rank per GPU (the driver's launch); more ranks than GPUs only for the one-GPU
    # rehearsal of the N > 1 path (SEG_BENCH_BACKEND=gloo: RCCL does not share a device)
    from utils.launch import rank_device
    ndev = torch.cuda.device_count()
    local_dev = rank_device(local, backend, ndev)
    shared_device = world > max(ndev, 1)
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from estimator.define_estimator_hierarchical import allreduce_grads
    from input_pipelines.synthetic import batch
    from models.initializers import init_params
    from seg_hip import SegContext

    global H, W, NB
    cfg = CONFIGS[args.config]
    depth, (nb_pp, nb_pb, nb_pi) = cfg["depth"], cfg["mix"]
    H, W = cfg.get("hw", (H, W))
    NB = nb_pp + nb_pb + nb_pi
    if args.dtype is None:
        args.dtype = cfg.get("dtype", "bf16")
    if args.pyramid is None:
        args.pyramid = cfg.get("pyramid", "aspp")
    # the reference's single-GPU step keeps an EMA of the model variables (ema_decay 0.9 with
    # num_updates = global_step, in UPDATE_OPS); MirroredStrategy runs drop it
    ema_on = world == 1
    ctx = SegContext(depth=depth, pyramid=args.pyramid, height=H, width=W, nb_pp=nb_pp, nb_pb=nb_pb,
                     nb_pi=nb_pi, dtype=args.dtype, device=local_dev, ema=ema_on)
    ctx.load_params(init_params(ctx.param_info, seed=0))
    if world == 1 and args.dtype != "fp16" and not args.no_defer_stem:
        # single process: the update of every parameter but the stem's runs beside the stem's
        # weight gradient, the step's last kernel (define_estimator_hierarchical.train_op does
        # the same); N > 1 updates after the all-reduce, fp16 after the overflow check
        ctx.set_defer_stem(True)
    data = batch(1000 + rank, nb_pp, nb_pb, nb_pi, H, W)
    img = torch.as_tensor(data["images"]).to(dev)
    px = torch.as_tensor(data["px"]).to(dev) if nb_pp else None
    bbox = torch.as_tensor(data["bbox"]).to(dev) if nb_pb else None
    tag = torch.as_tensor(data["tag"]).to(dev) if nb_pi else None
    del data

    scaler = None
    if args.dtype == "fp16":
        from estimator.define_optimizer import DynamicLossScaler
        scaler = DynamicLossScaler(ctx)

    from estimator.define_estimator_hierarchical import ema_decay_effective
    gstep = [0]
    comm_ev = []      # (backward issued, last all-reduce done) per timed step, N > 1
    timing = [None]

    def step():
        ctx.forward(img)
        ctx.loss(px, bbox, tag)
        ctx.backward()
        scale = allreduce_grads(ctx, timing=timing[0])
        ema = ema_decay_effective(EMA_DECAY, gstep[0]) if ema_on else 0.0
        ctx.apply_update(0.01, 0.9, ema, scale)
        gstep[0] += 1
        if scaler is not None:
            scaler.update()   # reads the device overflow flag (one 4-byte copy per step)

    for _ in range(args.warmup):
        step()
    calib = 0
    if scaler is not None:
        # the dynamic scale settles before the timed region (untimed extra warmup steps until
        # four consecutive steps have finite gradients), so the timed steps apply their updates
        while calib < 32 and scaler.good_steps < 4:
            step()
            calib += 1
        skipped0 = scaler.skipped
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    if world > 1:
        timing[0] = comm_ev
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    timing[0] = None
    comm = {"world_size": world, "backend": None, "allreduce_bytes_per_step": None,
            "buckets": None, "exposed_allreduce_ms": None, "exposed_allreduce_ms_max_rank": None}
    if world > 1:
        t = torch.tensor([elapsed], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # what the process group saw and what the gradient exchange cost: bytes all-reduced per
        # step (fp32 [grads | BN statistics]), and the all-reduce time the update waited for
        # after this rank's backward had been issued (mean over the timed steps; the max over
        # ranks beside it)
        bk = ctx.grad_buckets()
        exposed = [max(0.0, a.elapsed_time(b)) for a, b in comm_ev]
        ex = sum(exposed) / max(len(exposed), 1)
        te = torch.tensor([ex], device=dev)
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        comm.update(world_size=dist.get_world_size(), backend=str(dist.get_backend()),
                    allreduce_bytes_per_step=int(sum(hi - lo for lo, hi in bk) * 4),
                    buckets=len(bk), exposed_allreduce_ms=round(ex, 3),
                    exposed_allreduce_ms_max_rank=round(float(te.item()), 3))
    losses, _, _ = ctx.outputs()
    lv = losses.cpu().numpy()
    if not np.all(np.isfinite(lv)):
        raise RuntimeError(f"non-finite losses {lv}")
    if args.dump_outputs and rank == 0:
        dump_outputs(ctx, args.dump_outputs)

    roofline = None
    if do_profile:
        # HIP-event kernel timing (roofline) is recorded on the launch stream during ONE extra
        # step after the timed region: events around every conv launch cost ~1.8 ms per step
        # and the profiled step runs its backward on one stream
        ctx.profile(True)
        step()
        torch.cuda.synchronize()
        cls = {c: ctx.profile_read(c) for c in (0, 1, 2)}
        # every profiled class against its own roofline: conv classes in TFLOP/s vs the bf16
        # MFMA peak, BN streaming classes in TB/s of algorithmic bytes vs HBM peak
        bn = {c: ctx.profile_read(c) for c in (3, 4, 5)}
        all_classes = {}
        for c, r_ in list(cls.items()) + list(bn.items()):
            if r_["ms"] <= 0:
                continue
            conv = c < 3
            ach = r_["gflop"] / r_["ms"]   # GFLOP/ms = TFLOP/s; GB/ms = TB/s
            pk = (PEAK_BF16_TFLOPS if args.dtype in ("bf16", "fp16") else PEAK_F32_TFLOPS) if conv else PEAK_HBM_TBS
            all_classes[CLS_NAMES[c]] = {"ms": round(r_["ms"], 3), "launches": r_["launches"],
                                         "achieved": round(ach, 2),
                                         "unit": "TFLOP/s" if conv else "TB/s",
                                         "peak": pk, "frac": round(ach / pk, 4)}
        dom = max(cls, key=lambda c: cls[c]["ms"])
        r = cls[dom]
        peak = PEAK_BF16_TFLOPS if args.dtype in ("bf16", "fp16") else PEAK_F32_TFLOPS
        achieved = r["gflop"] / r["ms"]  # GFLOP/ms == TFLOP/s
        # HBM bytes per launch of that class from the committed PMC passes of this code
        # (tools/pmc_traffic.sh + tools/pmc_traffic.py; rocprofv3 cannot run inside the bench)
        traffic, tsrc, step_ledger = None, None, None
        for tname in ("r06_s25_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json",
                      "r01_pmc_traffic.json"):
            tpath = os.path.join(REPO, "profiles", tname)
            if not os.path.exists(tpath):
                continue
            tj = json.load(open(tpath))
            key = "conv_wgrad" if dom == 2 else "conv_nt"
            if key in tj:
                traffic = round(tj[key]["hbm_bytes_per_launch"])
                tsrc = f"profiles/{tname} ({key}, bytes per launch)"
                if "hbm_bytes" in tj.get("step", {}):
                    step_ledger = (tj["step"], f"profiles/{tname} (step)")
                break
        # the north star's named target: the dilated 3x3 convs of the encoder (block3 rate 2,
        # block4 rate 4, and the ASPP rates), per pass, against the MFMA peak
        dump = ctx.profile_dump()
        if os.environ.get("SEG_BENCH_DUMP"):   # diagnostics: the profiled step's records
            with open(os.environ["SEG_BENCH_DUMP"], "w") as f:
                json.dump(dump, f)
        # compulsory HBM bytes per launch of the dominant class (every operand once; for the
        # weight gradient x + dy in 16 bit and the fp32 dW): traffic / this = re-read factor
        rows_dom = [row for row in dump if row["cls"] == dom]
        alg_bytes = sum(row["gbytes"] for row in rows_dom) * 1e9 / max(len(rows_dom), 1)
        dil = {}
        for row in dump:
            if row["cls"] <= 2 and row["k"] == 3 and row["rate"] > 1:
                d = dil.setdefault(row["cls"], [0.0, 0.0, 0])
                d[0] += row["gflop"]; d[1] += row["ms"]; d[2] += 1
        dilated = {}
        for c_, (gf, ms_, n_) in sorted(dil.items()):
            dilated[("fwd", "dgrad", "wgrad")[c_]] = {"launches": n_, "ms": round(ms_, 3),
                                                      "achieved": round(gf / ms_, 1),
                                                      "frac": round(gf / ms_ / peak, 4)}
        if dil:
            gf = sum(v[0] for v in dil.values()); ms_ = sum(v[1] for v in dil.values())
            dilated["all"] = {"achieved": round(gf / ms_, 1), "frac": round(gf / ms_ / peak, 4),
                              "unit": "TFLOP/s"}
        # SURVEY §8(d)'s recommended form beside the plain MFMA fraction: per launch the
        # attainable time max(flops / P_mfma, compulsory bytes / BW_hbm) (short-K 1x1 layers and
        # the small-channel weight gradients are HBM-bound at their arithmetic intensity), summed
        # over the class and divided by its measured time; and the same sum over every profiled
        # conv / BN launch against the step time
        bound_ms = {}
        for row in dump:
            t_mfma = row["gflop"] / peak if row["cls"] <= 2 else 0.0      # GFLOP / (TFLOP/s) = ms
            gb = row["gbytes"] if row["cls"] <= 2 else row["gflop"]     # BN classes: gflop = GB
            bound_ms[row["cls"]] = bound_ms.get(row["cls"], 0.0) + max(t_mfma, gb / PEAK_HBM_TBS)
        for c_, b_ms in bound_ms.items():
            nm = CLS_NAMES[c_]
            if nm in all_classes and all_classes[nm]["ms"] > 0:
                all_classes[nm]["attainable_frac"] = round(b_ms / all_classes[nm]["ms"], 4)
        step_bound = round(sum(bound_ms.values()) / (elapsed * 1e3 / args.steps), 4)
        # the whole step against the chip: algorithmic conv flops at the MFMA peak vs the HBM-side
        # bytes of one step (PMC ledger, every kernel) at the achievable 6.29 TB/s
        # (MI355X_MICROARCH.md): the larger is the step's floor
        step_ms = elapsed * 1e3 / args.steps
        step_tflop = sum(row["gflop"] for row in dump if row["cls"] <= 2) / 1e3
        step_roof = {"tflop": round(step_tflop, 3), "mfma_ms": round(step_tflop / peak * 1e3, 3)}
        if step_ledger:
            sb = step_ledger[0]["hbm_bytes"]
            step_roof.update(hbm_bytes=round(sb), hbm_ms=round(sb / 6.29e12 * 1e3, 3),
                             source=step_ledger[1])
            step_roof["bound_ms"] = max(step_roof["mfma_ms"], step_roof["hbm_ms"])
            step_roof["frac"] = round(step_roof["bound_ms"] / step_ms, 4)
        names = dict(CLS_NAMES, **(CLS_NAMES_F32 if args.dtype == "fp32" else {}))
        roofline = {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak,
                    "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic,
                    "traffic_source": tsrc,
                    "algorithmic_bytes": round(alg_bytes),
                    "traffic_ratio": round(traffic / alg_bytes, 3) if traffic and alg_bytes else None,
                    "kernel": names[dom],
                    "launches": r["launches"],
                    "avg_launch_ms": round(r["ms"] / max(r["launches"], 1), 4),
                    # fwd + dgrad share the conv_nt*_kernel names in a rocprofv3 trace: their
                    # joint per-launch average is what profiles/*_kernel_classes_*.txt lists
                    "avg_launch_ms_nt_fwd_dgrad": round((cls[0]["ms"] + cls[1]["ms"]) /
                                                        max(cls[0]["launches"] + cls[1]["launches"], 1), 4),
                    "share_of_step": round(r["ms"] / (elapsed * 1e3 / args.steps), 3),
                    "profiled_steps": 1,
                    "classes_ms_per_step": {CLS_NAMES[c]: round(cls[c]["ms"], 2) for c in cls},
                    "classes": all_classes,
                    "dilated_3x3_encoder": dilated,
                    "attainable_frac": all_classes.get(CLS_NAMES[dom], {}).get("attainable_frac"),
                    "step_bound_frac": step_bound,
                    "step_hbm_bytes": step_roof.get("hbm_bytes"),
                    "step": step_roof,
                    "max_layer": r["max_layer"]}
        ctx.profile(False)
        if shared_device:
            # ranks time-slicing one GPU: per-kernel times include the other ranks' kernels
            roofline = {"invalid": f"{world} ranks share {ndev} GPU(s) (rehearsal): kernel times "
                                   "include other ranks' work", "bound": "mfma", "frac": None}

    # training-summary mIoU of the metric (define_metrics.py:5-20 via the device confusion
    # kernel), on the strong images of one extra forward + loss with fused decisions, outside
    # the timed region and after the profiled step has been read; random-init weights, so it
    # only exercises the path (the reference's 70.46 needs trained weights and Cityscapes)
    miou = None
    if args.full and nb_pp:
        from estimator.define_metrics import confusion_matrix, mean_iou_from_cm
        dec = torch.empty((nb_pp + nb_pb + nb_pi, H, W), dtype=torch.int32, device=dev)
        ctx.forward(img)
        ctx.loss(px, bbox, tag, dec)
        cm = confusion_matrix(ctx, px, dec[:nb_pp], 20)
        miou = round(float(mean_iou_from_cm(cm)), 5)
    # EVAL path (define_estimator_hierarchical.py:161-194) on the same resident batch, outside
    # the timed training region: moving-statistics BN forward + seg_predict (fused decisions,
    # cid map, nearest resize at label size = network size) + device confusion matrix
    ev = None
    if do_eval and nb_pp:
        from estimator.define_metrics import confusion_matrix
        from utils.utils import metrics_from_confusion_matrix
        cmap = list(range(19)) + [-1]
        edec = torch.empty((nb_pp + nb_pb + nb_pi, H, W), dtype=torch.int32, device=dev)
        ctx.set_bn_inference(True)

        def eval_batch():
            ctx.forward(img)
            ctx.predict(cmap, edec)
            return confusion_matrix(ctx, px, edec[:nb_pp], 20)
        eval_batch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            ecm = eval_batch()
        torch.cuda.synchronize()
        te = (time.perf_counter() - t0) / 3
        ctx.set_bn_inference(False)
        _, _, emiou, _, _ = metrics_from_confusion_matrix(
            np.asarray(ecm.cpu().numpy() if hasattr(ecm, "cpu") else ecm, np.int32)[:-1, :-1])
        ev = {"images_per_sec_per_gpu": round(NB / te, 3), "ms_per_batch": round(te * 1e3, 2),
              "batch": NB, "miou_eval": round(float(emiou), 3),
              "what": "moving-statistics BN forward + seg_predict + confusion (3 batches)"}
    ctx.close()
    train_py = None
    if world == 1 and do_train_py and args.config == "C2":
        # a failure of this side leg (host PNG encode, TFRecord writes, decode threads, a second
        # context) must not cost the headline line
        try:
            train_py = train_py_leg(args)
            train_py["ratio_to_value"] = round(train_py["images_per_sec"] /
                                               (NB * args.steps / elapsed), 3)
        except Exception as e:   # noqa: BLE001
            import traceback
            traceback.print_exc()
            train_py = {"error": repr(e)[:500]}
    cpu = None
    if rank == 0 and world == 1 and do_cpu and args.config == "C2":
        cpu = cpu_baseline(pyramid=args.pyramid)

    if world > 1 and comm["world_size"] != args.gpus:
        raise RuntimeError(f"process group has {comm['world_size']} ranks, --gpus {args.gpus}")
    if rank == 0:
        value = world * NB * args.steps / elapsed
        out = {"metric": "training images/sec at 1024x2048 bf16, 1/2/4/8 MI355X + mIoU vs ref",
               "value": round(value, 3), "unit": "images/sec", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "full": args.full,
               "ms_per_step": round(elapsed * 1e3 / args.steps, 2),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": args.dtype, "data": "synthetic (seeded; random-init weights)",
               "ema": EMA_DECAY if ema_on else None,
               "config": {"workload": cfg["name"] + " + " + args.pyramid.upper() +
                                      ", %dx%d, multi-loss head (pixel:bbox:tag = %d:%d:%d), "
                                      "fwd+loss+bwd+allreduce+SGDM%s" % (H, W, nb_pp, nb_pb, nb_pi,
                                                                         "+EMA" if ema_on else ""),
                          "global_batch": world * NB, "per_gpu_batch": NB,
                          "image": [H, W], "parallelism": f"dp{world}"},
               "losses_last_step": [round(float(x), 5) for x in lv[:4]],
               "miou_train_summary": miou,
               "eval": ev,
               "loss_scale": None if scaler is None else {
                   "scale": scaler.scale, "skipped_warmup": skipped0, "calibration_steps": calib,
                   "skipped_timed": scaler.skipped - skipped0},
               "comm": comm,
               "train_py": train_py,
               "roofline": roofline, "cpu_baseline": cpu}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
