"""Static A/B of every kernel of two source trees, no GPU: compiles each csrc/*.hip of both trees
to gfx950 assembly (device side only) and compares, per kernel, the descriptor values
(next_free_vgpr, accum_offset, next_free_sgpr, private_segment_fixed_size, static LDS), the
instruction count and the instruction text.
    python tools/kernel_static_ab.py <parent tree> [<this tree>] [--identical REGEX] [--gone REGEX]... [--keep DIR]
Kernel names are demangled and conv_nt_v2_kernel's former MFMA-shape argument (always 16) and the
scalar BN kernels' former vector width (always 1) are dropped, so the two trees' instantiations
pair up. --gone names parent kernels that must have no counterpart here; any other unpaired
kernel fails. Prints one row per kernel whose text differs
and a summary per file; exits 1 if a kernel matching --identical differs, if any differing kernel
has scratch, or a different accum_offset or allocated VGPR count (next_free_vgpr rounded up to the
allocation granule of 8)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
PKG = "iv2019-boosting-semantic-segmentation-with-weak-labels_amd"
FIELDS = ["next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size",
          "group_segment_fixed_size"]


def compile_s(tree, name, out):
    src = os.path.join(tree, PKG, "csrc", name)
    if os.path.exists(out):   # --keep DIR: assembly of an earlier run
        return open(out).read()
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    "-Wno-unused-function", "-Wno-unused-command-line-argument", src, "-o", out], check=True)
    return open(out).read()


def demangle(names):
    r = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def normal_name(d):
    # demangled "...conv_nt_v2_kernel<E, BN, WMW, WNW, STAGES, ST, T8, MF, BM, DU>(ConvArgs)" or, for
    # the fp16 element type the demangler does not know, the mangled "...ILi<BN>E...E": drop MF
    m = re.match(r"(.*conv_nt_v2_kernel<)(.*)(>\(ConvArgs\))$", d)
    if m:
        args = m.group(2).split(", ")
        if len(args) == 10:
            del args[7]
        return m.group(1) + ", ".join(args) + m.group(3)
    m = re.match(r"(.*conv_nt_v2_kernelIDF16_)((?:Li\d+E){9})(EEv8ConvArgs)$", d)
    if m:
        args = re.findall(r"Li\d+E", m.group(2))
        del args[6]
        return m.group(1) + "".join(args) + m.group(3)
    # the scalar BN kernels' former vector width (always 1), demangled or, for fp16, mangled
    if re.search(r"bn_(apply|bwd_reduce|bwd_apply)_kernel", d):
        return re.sub(r"Li1E(?=EEv\d+Bn\w+Args$)", "", re.sub(r", 1(?=>\(Bn\w+Args\)$)", "", d))
    return d


def kernels(asm):
    """{normalised name: (descriptor values, instruction lines)}"""
    desc = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        vals = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        desc[m.group(1)] = [int(vals.get(f, 0)) for f in FIELDS]
    names = list(desc)
    out = {}
    for sym, dem in zip(names, demangle(names) if names else []):
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), asm, re.S | re.M).group(1)
        ins = []
        for line in body.split("\n"):
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") and not t.startswith(".LBB"):
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", t).replace(sym, "KERNEL")
            ins.append(t)
        out[normal_name(dem)] = (desc[sym], [t for t in ins if not t.endswith(":")], ins)
    return out


def main():
    args = [a for a in sys.argv[1:]]
    ident = None
    if "--identical" in args:
        i = args.index("--identical")
        ident = re.compile(args[i + 1])
        del args[i:i + 2]
    gone = []
    while "--gone" in args:   # a parent kernel expected to have no counterpart here (repeatable)
        i = args.index("--gone")
        gone.append(re.compile(args[i + 1]))
        del args[i:i + 2]
    tmp = None
    if "--keep" in args:   # keep (and reuse) the assembly files in DIR
        i = args.index("--keep")
        tmp = args[i + 1]
        os.makedirs(tmp, exist_ok=True)
        del args[i:i + 2]
    parent = os.path.abspath(args[0])
    here = os.path.abspath(args[1] if len(args) > 1 else os.path.join(os.path.dirname(__file__), ".."))
    files = sorted(f for f in os.listdir(os.path.join(here, PKG, "csrc")) if f.endswith(".hip"))
    tmp = tmp or tempfile.mkdtemp()
    with ThreadPoolExecutor(16) as ex:
        jobs = {(t, f): ex.submit(compile_s, tree, f, os.path.join(tmp, f"{t}_{f}.s"))
                for t, tree in (("a", parent), ("b", here)) for f in files}
        asm = {k: j.result() for k, j in jobs.items()}
    bad = 0
    print("file kernel | vgpr accum_offset sgpr scratch static_lds instructions: parent -> this tree")
    for f in files:
        ka, kb = kernels(asm[("a", f)]), kernels(asm[("b", f)])
        for k in [k for k in ka if any(g.search(k) for g in gone)]:
            print(f"{f} {k}: " + ("expected to be gone, still here" if k in kb else "gone, as expected"))
            bad += k in kb
            del ka[k]
        if set(ka) != set(kb):
            print(f"{f}: kernel sets differ: {sorted(set(ka) ^ set(kb))}")
            bad += 1
        same = diff = 0
        for k in sorted(set(ka) & set(kb)):
            (da, ia, ta), (db, ib, tb) = ka[k], kb[k]
            if ta == tb and da == db:
                same += 1
                continue
            diff += 1
            flag = ""
            if ident and ident.search(k):
                flag += " MUST-BE-IDENTICAL"
            if da[3] or db[3] or (da[0] + 7) // 8 != (db[0] + 7) // 8 or da[1] != db[1]:
                flag += " OCCUPANCY"
            bad += bool(flag)
            print(f"{f} {k} | " + " ".join(f"{x}->{y}" if x != y else f"{x}" for x, y in zip(da + [len(ia)], db + [len(ib)])) + flag)
        print(f"{f}: {same + diff} kernels, {same} identical, {diff} differ")
    print("FAIL" if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
