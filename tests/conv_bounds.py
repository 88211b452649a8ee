"""Per-element error bound of a GEMM-shaped op (conv forward / data gradient, with or without
residuals) whose operands are fed as given, accumulated in fp32 and stored in `dtype`.

The L2-relative number the op tests assert averages over the tensor: one wave's worth of wrong
elements (128 rows x 32 columns) in a 64764 x 512 output moves it by about 0.012, under the bf16
tolerance of 2e-2. This bound is per element and derived, not tuned:

    bound = 2u (|dg| + |ref|) + K 2^-23 A + tiny

  u     unit roundoff of the output type (bf16 2^-8, fp16 2^-11, fp32 2^-24)
  dg    the float64 GEMM without residuals (plain convs: dg == ref)
  ref   the float64 result, residuals included
  K     the reduction length
  A     |a| @ |b| in float64 on the operands as fed
  tiny  2^-24 for fp16 (its subnormal spacing: the absolute floor of one rounding), else 0

First term: the output is rounded at most twice -- the v2 epilogue rounds the data gradient,
adds the residuals in fp32 and rounds again: u |dg| + u |ref| to first order; the persistent
residual path rounds dg + r once: u |ref| -- with a factor 2 of margin (the fp32 adds of the
residuals, second-order terms). Second term: an fp32 sum of K exact products in any order is
within gamma_K A <= K 2^-24 A (1 + o(1)) of the exact sum; twice that."""
import numpy as np

UNIT = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
TINY = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -24}


def gemm_bound(dtype, ref, absprod, K, dg=None):
    """Per-element bound (float64 array, ref's shape) on |got - ref|.

    ref: float64 result; absprod: |a| @ |b| in float64 (A above); K: reduction length;
    dg: the float64 GEMM without residuals (None: no residual, dg = ref)."""
    ref = np.asarray(ref, np.float64)
    dg = ref if dg is None else np.asarray(dg, np.float64)
    absprod = np.asarray(absprod, np.float64)
    return 2.0 * UNIT[dtype] * (np.abs(dg) + np.abs(ref)) + K * 2.0 ** -23 * absprod + TINY[dtype]


def violations(dtype, got, ref, absprod, K, dg=None):
    """(number of elements past the bound, max |got - ref| / bound) -- the tests assert 0."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    b = gemm_bound(dtype, ref, absprod, K, dg)
    err = np.abs(got - ref)
    bad = ~(err <= b)   # a NaN is a violation
    ratio = float(np.max(err / np.maximum(b, 1e-300))) if err.size else 0.0
    return int(bad.sum()), ratio
