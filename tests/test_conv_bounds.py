"""The per-element bound of tests/conv_bounds.py, checked on the CPU: a correct fp32-accumulate
GEMM never exceeds it, and it sees a fault the L2-relative assertion of the op tests cannot.

The fault modelled is the one a lost LDS-DMA race in the persistent residual data gradient
would leave: one wave adds, in place, a residual tile (128 rows x 32 columns) that has not
landed, i.e. whatever the LDS buffer held before -- data of the same magnitude from elsewhere."""
import functools

import numpy as np
import pytest
import torch

from conv_bounds import gemm_bound, violations

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"bf16": 2e-2, "fp16": 3e-3}   # the op tests' L2-relative tolerances (test_gpu_conv.py)


def _round(a, dtype):
    return torch.as_tensor(np.asarray(a, np.float32)).to(TDT[dtype]).to(torch.float32).numpy()


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _problem(M, K, N, dtype, seed):
    """The residual data-gradient test's operands: dy [M][K], w [K][N], r [M][N], 16-bit."""
    g = np.random.default_rng(seed)
    dy = _round(g.standard_normal((M, K)), dtype)
    w = _round(g.standard_normal((K, N)) * np.sqrt(2.0 / N), dtype)
    r = _round(g.standard_normal((M, N)), dtype)
    return dy, w, r


def _emulate(dy, w, r, dtype, roundings):
    """fp32 accumulation in MFMA-sized steps (32 products per step, sequential over K), then
    one rounding of dg + r (the persistent residual path) or two (the v2 epilogue)."""
    acc = np.zeros((dy.shape[0], w.shape[1]), np.float32)
    for k in range(0, dy.shape[1], 32):
        acc = acc + dy[:, k:k + 32] @ w[k:k + 32]
    if roundings == 1:
        return _round(acc + r, dtype)
    return _round(_round(acc, dtype) + r, dtype)


def _f64(dy, w, r):
    dg = dy.astype(np.float64) @ w.astype(np.float64)
    absprod = np.abs(dy).astype(np.float64) @ np.abs(w).astype(np.float64)
    return dg, dg + r, absprod


@pytest.mark.parametrize("roundings", [1, 2])
@pytest.mark.parametrize("K", [192, 256, 512])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fp32_accumulate_is_within_the_bound(dtype, K, roundings):
    dy, w, r = _problem(1024, K, 512, dtype, seed=K)
    dg, ref, absprod = _f64(dy, w, r)
    got = _emulate(dy, w, r, dtype, roundings)
    nbad, ratio = violations(dtype, got, ref, absprod, K, dg)
    print(f"{dtype} K={K} roundings={roundings}: max err / bound {ratio:.3f}")
    assert nbad == 0
    # and without a residual (plain convs: dg == ref, one rounding)
    nbad, ratio = violations(dtype, _round(_emulate(dy, w, 0.0, dtype, 1), dtype), dg, absprod, K)
    assert nbad == 0


@functools.lru_cache(maxsize=1)
def _large(dtype):   # computed once per type, shared by the two rounding cases, never written
    dy, w, r = _problem(4 * 63 * 257, 192, 512, dtype, seed=11)
    return (dy, w, r) + _f64(dy, w, r)


@pytest.mark.parametrize("roundings", [1, 2])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stale_block_is_flagged_where_l2_is_blind(dtype, roundings):
    """M = 4 x 63 x 257 rows, 512 columns, K 192 (the suite's largest residual case). A stale
    128 x 32 residual block is flagged element by element in both types. The L2-relative number
    moves to about 0.012 (4096 errors of variance 2 against 33 M elements of variance 1.75):
    under the bf16 tolerance 2e-2, so the old bf16 assertion passes with 4096 wrong elements.
    The fp16 tolerance 3e-3 does see a whole block; there the L2 number is blind from one stale
    16-row DMA piece of half its columns down (256 elements: about 0.003), shown with one stale
    16-byte chunk, the unit the DMA moves."""
    K = 192
    dy, w, r, dg, ref, absprod = _large(dtype)
    good = _emulate(dy, w, r, dtype, roundings)
    assert violations(dtype, good, ref, absprod, K, dg)[0] == 0
    assert _rel(good, ref) < TOL[dtype]
    # the block of wave (wm 1, wn 2) of tile row 7, column half 1 of column tile 1
    r0, c0 = 7 * 256 + 128, 256 + 128 + 64
    rows, cols = (128, 32) if dtype == "bf16" else (1, 8)
    stale = r.copy()
    stale[r0:r0 + rows, c0:c0 + cols] = r[r0 + 4096:r0 + 4096 + rows, c0 - 64:c0 - 64 + cols]
    bad = _emulate(dy, w, stale, dtype, roundings)
    l2 = _rel(bad, ref)
    err = np.abs(bad.astype(np.float64) - ref)
    flagged = err > gemm_bound(dtype, ref, absprod, K, dg)
    print(f"{dtype} roundings={roundings}: stale {rows}x{cols}: L2 {l2:.4f} (tol {TOL[dtype]}), "
          f"{int(flagged.sum())} of {rows * cols} flagged")
    assert l2 < TOL[dtype]                      # the old assertion passes ...
    inside = np.zeros_like(flagged)
    inside[r0:r0 + rows, c0:c0 + cols] = True
    assert not flagged[~inside].any()
    # ... the per-element one does not: two unrelated N(0, 1) values differ by more than the
    # bound (about 2^-7 (|dg| + |ref|), a few hundredths) in all but a few percent of the cases
    assert flagged.sum() >= 0.9 * rows * cols
    if dtype == "fp16":   # a whole block is flagged too (the fp16 L2 tolerance also sees it)
        stale[r0:r0 + 128, c0:c0 + 32] = r[r0 + 4096:r0 + 4096 + 128, c0 - 64:c0 - 64 + 32]
        bad = _emulate(dy, w, stale, dtype, roundings)
        assert violations(dtype, bad, ref, absprod, K, dg)[0] >= 0.9 * 128 * 32
