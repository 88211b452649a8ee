"""Bit comparison, and with --time a timing, of the decision heads of two libraries (sibling of
ab_conv_bits.py): seg_predict (replace_voids 0, 1 and 2), seg_full_predictions (all four
outputs), seg_tta_decisions and seg_window_decisions (with and without mean_probs; overlapping,
one-row and one-column grids; with and without flip) on seeded logits, from the working-tree
library and from an A/B build (SEG_HIP_LIB), each in its own child process, one after the other;
seg_crc32c of every output buffer must be equal.

Inputs: both datasets; network 64 x 128 and the odd 101 x 103; output sizes (64, 128), (32, 64),
(45, 77), (128, 256); standard normal logits at amplitude 1.0 and 3.0 and one set quantised to
multiples of 1/8, where exact ties and near-ties occur (the first-maximum and stable top-2 rules
and the replace_voids = 2 ranking only matter there).

--time: seg_predict (modes 0, 1, 2) and seg_full_predictions at 1024 x 2048, N = 1, both
datasets, device events, alternating rounds in one process, medians of 15 rounds after 3 warm-up
rounds (the scheme of tta_table.py), in the order other library, working tree, other library. The
working tree passes when its median is at most the slower of the other library's two medians plus
the gap between those two (the session's own noise).

The other library is built from a checkout of the other commit (`make VARIANT=parent` in its csrc/
writes <checkout>/ab/parent/libseg_hip.so) and copied to ab/ here.

    python tools/ab_decision_bits.py ab/parent/libseg_hip.so [--time]"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")

WIDTHS = {"cityscapes": (14, 7, 3), "vistas": (53, 12, 5)}
MAPS = {"cityscapes": {"identity": list(range(19)) + [-1],
                       "merge": [0, 0, 1, 1, 2, -1, 3, 3, 4, 5, 6, 7, 7, 8, 8, 8, 9, 9, 9, -1]},
        "vistas": {"identity": list(range(65)) + [-1]}}
NETS = [(64, 128), (101, 103)]
OUTS = [(64, 128), (32, 64), (45, 77), (128, 256)]
LOGITS = ["amp 1.0", "amp 3.0", "eighths"]
TTA_LOW = [(4, 8), (6, 12), (8, 16), (10, 20), (13, 13)]       # tests/tta_ref.py's LOW_SIZES
WIN_LOW = (8, 16)                                               # tests/window_ref.py's LOW_HW
# canvas = network + these margins at these strides: overlapping in both axes, one row, one column
GRIDS = {"overlap": ((36, 72), (24, 40)), "one row": ((0, 72), (24, 40)), "one column": ((36, 0), (24, 40))}
WARM, REPS = 3, 15


def draw(torch, g, shape, kind):
    x = torch.randn(shape, generator=g)
    if kind == "eighths":
        return torch.round(x * 8) / 8
    return x * float(kind.split()[1])


def origins(C, n, s):
    return list(range(0, C - n, s)) + [C - n]


def bits(out):
    sys.path[:0] = [REPO, PKG]
    import torch
    from seg_hip import LIB, SegContext

    cuda = torch.device("cuda")
    rows = []

    def crc(t):
        torch.cuda.synchronize()
        b = t.contiguous().view(torch.uint8).cpu().numpy().tobytes()
        return LIB.seg_crc32c(0, b, len(b))

    for dataset in WIDTHS:
        ct = sum(WIDTHS[dataset])
        for net in NETS:
            ctx = SegContext(pyramid="none", height=net[0], width=net[1], nb_pp=2, dtype="fp32", dataset=dataset)
            lg = ctx.outputs()[2]
            outs = OUTS + ([net] if net not in OUTS else [])
            for kind in LOGITS:
                g = torch.Generator().manual_seed(41 + LOGITS.index(kind))
                tag = f"{dataset} {net[0]}x{net[1]} {kind}"
                lg.copy_(draw(torch, g, tuple(lg.shape), kind).to(cuda))
                for mapname, cid_map in MAPS[dataset].items():
                    for ohw in outs:
                        for rv in (0, 1, 2):
                            d = torch.full((2,) + ohw, -7, dtype=torch.int32, device=cuda)
                            ctx.predict(cid_map, d, replace_voids=rv > 0, order="predict" if rv == 2 else "eval")
                            rows.append([f"{tag} predict {mapname} {ohw} rv{rv}", crc(d)])
                full = [torch.full((2,) + net + (ct,), -1.0, device=cuda), torch.full((2,) + net + (ct,), -1.0, device=cuda),
                        torch.full((2,) + net + (3,), -7, dtype=torch.int32, device=cuda),
                        torch.full((2,) + net, -7, dtype=torch.int32, device=cuda)]
                ctx.full_predictions(*full)
                rows.append([f"{tag} full_predictions"] + [crc(t) for t in full])
                cid_map = MAPS[dataset]["identity"]
                ents = [(draw(torch, g, (2,) + low + (ct,), kind).to(cuda), flip) for low in TTA_LOW
                        for flip in (False, True)]
                for name, es in (("10 entries", ents), ("1 entry", ents[4:5]), ("unflipped", ents[0::2])):
                    for ohw in outs:
                        for rv in (0, 1):
                            d = torch.full((2,) + ohw, -7, dtype=torch.int32, device=cuda)
                            ctx.tta_decisions(es, cid_map, d, replace_voids=bool(rv))
                            rows.append([f"{tag} tta {name} {ohw} rv{rv}", crc(d)])
                    d = torch.full((2,) + net, -7, dtype=torch.int32, device=cuda)
                    p = torch.full((2,) + net + (ct,), -1.0, device=cuda)
                    ctx.tta_decisions(es, cid_map, d, replace_voids=True, mean_probs=p)
                    rows.append([f"{tag} tta {name} mean_probs", crc(d), crc(p)])
                for gname, (margin, stride) in GRIDS.items():
                    canvas = (net[0] + margin[0], net[1] + margin[1])
                    ys, xs = origins(canvas[0], net[0], stride[0]), origins(canvas[1], net[1], stride[1])
                    wl = [draw(torch, g, (2,) + WIN_LOW + (ct,), kind).to(cuda) for _ in range(2 * len(ys) * len(xs))]
                    for flip in (False, True):
                        es = wl if flip else wl[0::2]
                        for ohw in [(45, 77), (128, 256), canvas]:
                            for rv in (0, 1):
                                d = torch.full((2,) + ohw, -7, dtype=torch.int32, device=cuda)
                                ctx.window_decisions(es, ys, xs, flip, canvas, cid_map, d, replace_voids=bool(rv))
                                rows.append([f"{tag} window {gname} flip{int(flip)} {ohw} rv{rv}", crc(d)])
                        d = torch.full((2,) + canvas, -7, dtype=torch.int32, device=cuda)
                        p = torch.full((2,) + canvas + (ct,), -1.0, device=cuda)
                        ctx.window_decisions(es, ys, xs, flip, canvas, cid_map, d, replace_voids=True, mean_probs=p)
                        rows.append([f"{tag} window {gname} flip{int(flip)} mean_probs", crc(d), crc(p)])
            ctx.close()
    json.dump(rows, open(out, "w"))


def times(out):
    sys.path[:0] = [REPO, PKG]
    import numpy as np
    import torch
    from seg_hip import SegContext

    cuda = torch.device("cuda")
    H, W = 1024, 2048
    rows = []
    for dataset in WIDTHS:
        ct = sum(WIDTHS[dataset])
        ctx = SegContext(pyramid="none", height=H, width=W, nb_pp=1, dtype="bf16", dataset=dataset)
        lg = ctx.outputs()[2]
        lg.copy_((3.0 * torch.randn(tuple(lg.shape), generator=torch.Generator().manual_seed(7))).to(cuda))
        cid_map = MAPS[dataset]["identity"]
        d = torch.empty((1, H, W), dtype=torch.int32, device=cuda)
        full = [torch.empty((1, H, W, ct), device=cuda), torch.empty((1, H, W, ct), device=cuda),
                torch.empty((1, H, W, 3), dtype=torch.int32, device=cuda), torch.empty((1, H, W), dtype=torch.int32, device=cuda)]
        calls = {f"predict rv{rv}": (lambda rv=rv: ctx.predict(cid_map, d, replace_voids=rv > 0,
                                                                order="predict" if rv == 2 else "eval")) for rv in (0, 1, 2)}
        calls["full_predictions"] = lambda: ctx.full_predictions(*full)
        ts = {k: [] for k in calls}
        for r in range(WARM + REPS):
            for name, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if r >= WARM:
                    ts[name].append(a.elapsed_time(b))
        rows += [[f"{dataset} {k}", float(np.median(v)), float(min(v))] for k, v in ts.items()]
        ctx.close()
        del full
        torch.cuda.empty_cache()
    json.dump(rows, open(out, "w"))


def run(lib, mode, out):
    env = dict(os.environ)
    env.pop("SEG_HIP_LIB", None)
    if lib:
        env["SEG_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out], env=env, capture_output=True,
                       text=True, timeout=420)
    if r.returncode:
        print(r.stdout[-2000:], r.stderr[-2000:])
        r.check_returncode()
    return json.load(open(out))


def main():
    if sys.argv[1] == "--bits-child":
        return bits(sys.argv[2])
    if sys.argv[1] == "--time-child":
        return times(sys.argv[2])
    other = os.path.abspath(sys.argv[1])
    if "--time" in sys.argv[2:]:
        p1 = run(other, "--time-child", "/tmp/ab_decision_time_p1.json")
        new = run(None, "--time-child", "/tmp/ab_decision_time_new.json")
        p2 = run(other, "--time-child", "/tmp/ab_decision_time_p2.json")
        print(f"# medians (minima) in ms of {REPS} rounds after {WARM} warm-up rounds at 1024 x 2048, N = 1; order: "
              f"{os.path.relpath(other, REPO)}, working tree, {os.path.relpath(other, REPO)}")
        print(f"{'call':<30} {'other 1':>16} {'working tree':>16} {'other 2':>16} {'allowed':>8}  verdict")
        slow = 0
        for a, n, b in zip(p1, new, p2):
            allowed = max(a[1], b[1]) + abs(a[1] - b[1])
            slow += n[1] > allowed
            print(f"{a[0]:<30} {a[1]:8.4f} ({a[2]:.4f}) {n[1]:8.4f} ({n[2]:.4f}) {b[1]:8.4f} ({b[2]:.4f}) "
                  f"{allowed:8.4f}  {'ok' if n[1] <= allowed else 'SLOWER'}")
        return 1 if slow else 0
    a = run(None, "--bits-child", "/tmp/ab_decision_bits_a.json")
    b = run(other, "--bits-child", "/tmp/ab_decision_bits_b.json")
    assert [r[0] for r in a] == [r[0] for r in b]
    bad = 0
    print(f"{'call':<78} {'working tree':<44} {os.path.relpath(other, REPO)}")
    for x, y in zip(a, b):
        fmt = lambda r: " ".join(f"{c:08x}" for c in r[1:])
        bad += x != y
        print(f"{x[0]:<78} {fmt(x):<44} {fmt(y)}{'' if x == y else '   DIFFERENT'}")
    nbuf = sum(len(x) - 1 for x in a)
    print(f"{len(a)} calls, {nbuf} buffers: {'all checksums equal' if not bad else f'{bad} calls differ'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
