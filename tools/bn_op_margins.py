"""Writes profiles/bn_op_margins.txt from the output of
    python -m pytest -s tests/test_gpu_bn.py
(its "MARGIN op dtype check ratio" lines): the worst err / bound per op, dtype and check, and the
finalize's measured k beside the float32 restatement's.

usage: python tools/bn_op_margins.py <pytest output> [<out file>]"""
import collections
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER = """\
# tests/test_gpu_bn.py on one MI355X: worst |got - ref| / bound per op, dtype and check, over every
# case of the op (bounds and references: tests/bn_refs.py; 0 violations everywhere). Counted checks
# (dyhat, the ReLU bits) are exact and list 0.
# 16-bit outputs sit just under 1 by construction: u |ref| is the half-ulp of a correctly rounded
# store, reached wherever a value falls next to a rounding tie. The fp32 rows are the arithmetic
# alone against 4e: at most 0.76.
# Sums (dbeta, dgamma, sdy, sdyx, part, cs_part): the bound 1e-6 |ref| + 4e sqrt(M) sum |term| grows
# with M^1.5 while an fp32 tree sum's error does not; at 66,000 rows it is about one term wide, so a
# dropped row is a finding of the small shapes (tests/test_bn_refs.py), not of that one. Worst
# native sum ratio: 0.13.
# stats: k_mean / k_var = worst err / (e x the bound's scale) of the native finalize over
# tests/bn_refs.py STATS_CASES; *_restatement = the same figure of the float32 restatement of the
# kernel's formula (sums in the kernel's lane order); the bound allows 4 x the restatement's.
# stats_conv: the finalize on the partials of a native conv; stats_conv_moments: against the float64
# moments of the reference conv (bound: test_stats_finalize_of_a_native_conv's docstring).
# op dtype check worst_ratio
"""


def main(argv):
    src = argv[1]
    dst = argv[2] if len(argv) > 2 else os.path.join(REPO, "profiles", "bn_op_margins.txt")
    worst = collections.OrderedDict()
    for line in open(src):
        i = line.find("MARGIN ")
        if i < 0:
            continue
        _, op, dtype, check, ratio = line[i:].split()
        key = (op, dtype, check)
        worst[key] = max(worst.get(key, 0.0), float(ratio))
    if not worst:
        sys.exit("no MARGIN lines in " + src)
    with open(dst, "w") as f:
        f.write(HEADER)
        for (op, dtype, check), r in sorted(worst.items()):
            f.write(f"{op} {dtype} {check} {r:.4f}\n")
    print(f"{len(worst)} rows -> {dst}")


if __name__ == "__main__":
    main(sys.argv)
