"""The launch-sequence pin's cases and recorder, shared by tests/golden/make_step_sequence_fixture.py
(run once against the parent commit's library) and tests/test_gpu_step_sequence.py (the working
tree's library).

A profiled step runs on one stream and seg_profile_dump lists every conv, BN-apply, BN-reduce and
BN-backward-apply launch in issue order. One record is kept as [class, conv index, work, bytes]
with the work and bytes columns exactly as printed ("%.6f"); the time column is dropped. All cases
are 64 x 128, depth 50, synthetic data as in test_lbf_matches: the smallest size at which the
fold, the pre-masked stores and the dual kernels are all taken."""
import ctypes

H, W = 64, 128
COUNTERS = ["premask_launches", "lbf_layers", "loss_yf_launches", "bootstrap_launches"]

# name, SegContext arguments, switches (set_premask / set_lbf)
CASES = [
    # fold, pre-masked stores, dual data gradient and dual BN backward
    ("bf16_aspp", dict(dtype="bf16", pyramid="aspp", nb_pp=2), {}),
    ("bf16_aspp_nolbf", dict(dtype="bf16", pyramid="aspp", nb_pp=2), dict(lbf=False)),
    ("bf16_aspp_nopremask_nolbf", dict(dtype="bf16", pyramid="aspp", nb_pp=2),
     dict(premask=False, lbf=False)),
    ("bf16_psp_fov", dict(dtype="bf16", pyramid="psp", fov_k=3, fov_rate=2, nb_pp=1, nb_pb=1), {}),
    ("fp32_psp_hybrid", dict(dtype="fp32", pyramid="psp", upsampling="hybrid", nb_pp=1, nb_pb=1), {}),
    # group norm's per-image launches are not profiled: the conv records and bn_apply_one per image
    ("bf16_gn", dict(dtype="bf16", pyramid="none", norm="group", nb_pp=2), {}),
]
CASE_NAMES = [c[0] for c in CASES]


def record(name):
    """One profiled step (forward, loss, backward) of a case on the loaded library:
    (rows, counters, conv names by index)."""
    import torch
    import seg_hip
    from input_pipelines.synthetic import batch
    from models.initializers import init_params
    _, kw, sw = CASES[CASE_NAMES.index(name)]
    ctx = seg_hip.SegContext(depth=50, height=H, width=W, **kw)
    try:
        ctx.load_params(init_params(ctx.param_info, seed=14))
        if "premask" in sw:
            ctx.set_premask(sw["premask"])
        if "lbf" in sw:
            ctx.set_lbf(sw["lbf"])
        npp, npb = kw.get("nb_pp", 0), kw.get("nb_pb", 0)
        d = batch(25, npp, npb, 0, H, W)
        dev = lambda k: torch.as_tensor(d[k]).cuda()
        ctx.profile(True)
        ctx.forward(dev("images"))
        ctx.loss(dev("px") if npp else None, dev("bbox") if npb else None, None)
        ctx.backward()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 22)
        seg_hip.check(seg_hip.LIB.seg_profile_dump(ctx.h, buf, len(buf)), ctx.h)
        ctx.profile(False)
        # conv index = creation order (the hybrid deconvolutions' weights come after every conv)
        names = [p.name[:-len("/weights")] for p in ctx.param_info if p.name.endswith("/weights")]
        index = {n: i for i, n in enumerate(names)}
        rows = []
        for line in buf.value.decode().splitlines():
            f = line.split()   # cls name ci co k rate Ho Wo work ms bytes
            rows.append([int(f[0]), index[f[1]], f[8], f[10]])
        counters = {k: ctx.counter(k) for k in COUNTERS}
    finally:
        ctx.close()
    return rows, counters, names
