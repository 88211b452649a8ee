"""Float64 references, per-element bounds and float32 restatements of the batch-norm launches
(csrc/bn.hip through the seg_op_bn_* entries); a plain helper module, like tests/conv_bounds.py.
tests/test_gpu_bn.py holds the kernels to these bounds, tests/test_bn_refs.py shows on the CPU
that the checkers discriminate.

Every reference is fed what the kernel read: 16-bit tensors widened, the fp32 per-channel vectors
as given, and for the backward apply the sdy / sdyx the native finalize wrote, so each kernel is
judged on its own arithmetic. Every check is per element, zero violations allowed.

  u = unit roundoff of a 16-bit store (bf16 2^-8, fp16 2^-11; an fp32 store adds nothing)
  e = 2^-24, the unit roundoff of the fp32 arithmetic
  tiny = 2^-25 for fp16 stores (half its subnormal spacing: the absolute floor of one rounding)

apply          |got - ref| <= 4e (|y - mu||s| + |beta| + |residual term|) + u |ref| + tiny
               (subtract, multiply-add, add of the residual: at most 4 roundings, each relative
               to a partial result no larger than the sum of the magnitudes); the ReLU bits equal
               stored out > 0 exactly, and the reference's sign wherever |ref| exceeds its bound
sums           dbeta, dgamma, sdy, sdyx, the summed cs_part:
               |got - ref| <= 1e-6 |ref| + 4e sqrt(M) sum |term| (step_chain's form for weight
               gradients; the terms are the exact float64 products of the inputs)
stored dyhat   bit-exact: the dz element or 0; with dshift the T-rounding of the fp32 dz + dshift
backward dy    |got - ref| <= u |ref| + 4e |scale| (|d| + |sdy| + |xhat sdyx|) + tiny
stats          against the exact float64 merge of the fp32 partials:
               |mean - ref| <= k_mean e (|mean| + sum_t n_t |mean_t - p| / N)
               |var - ref|  <= k_var e B / N, i.e. relative k_var e kappa with kappa = (B / N) / var,
               the condition number of B / N - dm^2 in the kernel's shifted form (p = tile 0's mean);
               invstd, scale, var_unb and pack through the same var. k_mean and k_var are not
               guessed: 4 x the worst ratio of the float32 restatement of the kernel's formula
               (stats_restate_f32, sums in the kernel's lane order) over STATS_CASES (stats_k()).

What step_chain's L2-relative 2e-2 on the BN-backward dy lets through (test_bn_refs.py asserts
each beside the flag): the last row of a ragged row block dropped from the sums (dy moves by 3e-3
at 391 rows; at 65 rows it is 4e-2 and seen), a zero-filled tail row counted in cs_part and dzscale
applied to the stored dyhat (dy does not move at all), and the dual reduce writing the first
layer's sum of dyhat xhat into the second layer's partials (sdyx is O(1 / sqrt(M)): 8e-2 at 391
rows, 9e-3 at 16,384). var_unb without the Bessel factor is outside it altogether: it feeds only
the moving average. It does see dshift added after the gate, the reversed bit order and the
neighbouring mask byte (O(1) on half the elements). The residual row computed with Wo for Wr and
the ragged stats tile weighted as a full one are forward faults, judged by step_chain's forward
links, not by that number."""
import functools

import numpy as np
import torch

E = 2.0 ** -24
UNIT = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
TINY = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BN_EPS = float(np.float32(1.001e-5))   # SEG_BN_EPS as the kernel holds it
f32 = np.float32


def round_to(a, dtype):
    """float32 array rounded once to `dtype` (round to nearest even), widened back"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "fp32":
        return a
    return torch.from_numpy(a).to(TDT[dtype]).to(torch.float32).numpy()


def fma32(a, b, c):
    """fp32 fused multiply-add of float32 arrays (the float64 product of two floats is exact)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def violations(got, ref, bound):
    """(elements past the bound, worst err / bound); a NaN is a violation"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - np.asarray(ref, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    bad = ~(err <= bound)
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if err.size else 0.0
    return int(bad.sum()), ratio


# ---- ReLU bits ------------------------------------------------------------------------------
def pack_bits(pos):
    """[M][C] bool -> [M][C/8] uint8, bit e of byte g = channel 8 g + e"""
    return np.packbits(np.asarray(pos, bool), axis=1, bitorder="little")


def unpack_bits(mask, C, mutant=None):
    """[M][C/8] uint8 -> [M][C] bool. Mutants: 'bit_reversed' reads bit 7 - e, 'neighbour_byte'
    reads the byte of the next channel group."""
    mask = np.asarray(mask, np.uint8)
    if mutant == "neighbour_byte":
        mask = np.roll(mask, -1, axis=1)
    bits = np.unpackbits(mask, axis=1, bitorder="big" if mutant == "bit_reversed" else "little")
    return bits[:, :C].astype(bool)


# ---- forward statistics ---------------------------------------------------------------------
def tile_partials(x, tile_rows):
    """float64 [M][C] -> the conv epilogue's fp32 partials [ntiles][C][2]: (sum, M2 about the
    tile's own mean) of tile_rows rows, the last tile ragged"""
    M, C = x.shape
    nt = -(-M // tile_rows)
    part = np.zeros((nt, C, 2), np.float64)
    for t in range(nt):
        blk = x[t * tile_rows:(t + 1) * tile_rows]
        part[t, :, 0] = blk.sum(0)
        part[t, :, 1] = ((blk - blk.mean(0)) ** 2).sum(0)
    return part.astype(f32)


def _tile_counts(M, tile_rows, nt):
    return np.minimum(tile_rows, M - np.arange(nt, dtype=np.int64) * tile_rows).astype(np.float64)


def stats_exact(part, M, tile_rows):
    """The exact (float64) merge of the fp32 partials, with the magnitudes the bounds scale by"""
    part = np.asarray(part, np.float64)
    n = _tile_counts(M, tile_rows, part.shape[0])[:, None]
    mean_t = part[:, :, 0] / n
    mean = part[:, :, 0].sum(0) / M
    var = (part[:, :, 1] + n * (mean_t - mean) ** 2).sum(0) / M
    p = mean_t[0]
    return {"mean": mean, "var": var, "N": float(M),
            "B_over_N": (part[:, :, 1] + n * (mean_t - p) ** 2).sum(0) / M,
            "A_abs": (n * np.abs(mean_t - p)).sum(0) / M}


def _sum32(a, order):
    """float32 sum over the tiles. 'lanes' = the order bn.hip's comment gives (64 tile lanes,
    lane l adding tiles l, l + 64, ... in turn; a butterfly over each 8 lanes; the 8 results
    added in order); 'seq' = one running sum over the tiles, an order the kernel does not use"""
    a = np.asarray(a, f32)
    if order == "seq":
        s = np.zeros(a.shape[1:], f32)
        for row in a:
            s = s + row
        return s
    pad = (-a.shape[0]) % 64
    a = np.concatenate([a, np.zeros((pad,) + a.shape[1:], f32)]).reshape((-1, 64) + a.shape[1:])
    lane = np.zeros(a.shape[1:], f32)
    for rnd in a:
        lane = lane + rnd
    w = lane.reshape((8, 8) + lane.shape[1:])   # [wave][lane in wave]
    for o in (1, 2, 4):
        w = w + w[:, np.arange(8) ^ o]
    s = w[0, 0]
    for k in range(1, 8):
        s = s + w[k, 0]
    return s


def stats_restate_f32(part, M, tile_rows, gamma, order="lanes", mutant=None):
    """The finalize in float32, from the formula (bn.hip's comment on the shifted sums): p = tile
    0's mean, A = sum_t n_t (mean_t - p), B = sum_t (M2_t + n_t (mean_t - p)^2), mean = p + A / N,
    var = B / N - (A / N)^2. Mutants: 'no_bessel', 'ragged_full' (the last tile weighted as a
    full one)."""
    part = np.asarray(part, f32)
    n = _tile_counts(M, tile_rows, part.shape[0]).astype(f32)
    if mutant == "ragged_full":
        n[-1] = tile_rows
    n = n[:, None]
    mean_t = part[:, :, 0] / n
    p = mean_t[0]
    d = mean_t - p
    A = _sum32(n * d, order)
    B = _sum32(part[:, :, 1] + (n * d) * d, order)
    N = f32(M)
    dm = A / N
    mean = p + dm
    var = np.maximum(B / N - dm * dm, f32(0))
    inv = (f32(1) / np.sqrt(var + f32(BN_EPS))).astype(f32)
    bessel = f32(1) if mutant == "no_bessel" else N / (N - f32(1) if M > 1 else f32(1))
    return {"mean": mean, "invstd": inv, "scale": np.asarray(gamma, f32) * inv,
            "var_unb": var * bessel, "pack": np.concatenate([mean, var + mean * mean])}


def stats_check(got, part, M, tile_rows, gamma, k_mean, k_var):
    """got: dict of mean, invstd, scale, var_unb and optionally pack ([2C]) as the finalize wrote
    them. Returns {name: (violations, worst err / bound)} and the raw ratios 'k_mean', 'k_var' =
    worst err / (e x the scale of the bound), the figure stats_k() measures."""
    ex = stats_exact(part, M, tile_rows)
    gamma = np.asarray(gamma, np.float64)
    mean, var, N = ex["mean"], ex["var"], ex["N"]
    mean_s = np.abs(mean) + ex["A_abs"]
    var_s = ex["B_over_N"]
    mean_b, var_b = k_mean * E * mean_s, k_var * E * var_s
    inv = 1.0 / np.sqrt(var + BN_EPS)
    # d invstd = -1/2 invstd d var / (var + eps); rsqrt, the add of eps: 4e relative
    inv_b = inv * (0.5 * var_b / (var + BN_EPS) + 4 * E)
    bessel = N / (N - 1.0) if M > 1 else 1.0
    out = {"mean": violations(got["mean"], mean, mean_b),
           "invstd": violations(got["invstd"], inv, inv_b),
           "scale": violations(got["scale"], gamma * inv, np.abs(gamma) * (inv_b + E * inv)),
           "var_unb": violations(got["var_unb"], var * bessel, bessel * var_b + 2 * E * var * bessel)}
    g64 = np.asarray(got["mean"], np.float64)
    out["k_mean"] = (0, float(np.max(np.where(g64 == mean, 0.0, np.abs(g64 - mean) / np.maximum(E * mean_s, 1e-300)))))
    # var as the kernel formed it, recovered from var_unb (exact but for 2 roundings)
    v64 = np.asarray(got["var_unb"], np.float64) / bessel
    out["k_var"] = (0, float(np.max(np.where(v64 == var, 0.0, np.abs(v64 - var) / np.maximum(E * var_s, 1e-300)))))
    if got.get("pack") is not None:
        C = mean.shape[0]
        pk = np.asarray(got["pack"], np.float64)
        ex2 = var + mean * mean
        out["pack_mean"] = violations(pk[:C], mean, mean_b)
        out["pack_ex2"] = violations(pk[C:], ex2, var_b + 2 * np.abs(mean) * mean_b + 3 * E * ex2)
    return out


# the synthetic finalize cases: (M, C, tile_rows, kind); kind 'typical' = every tile N(m_c, s_c),
# 'tile0_zero' = tile 0 constant zero and the rest of mean 3 (the image-border case that stresses
# the shifted form). Channel 0 is constant (1.5: every sum exact, var = 0) in the typical cases.
STATS_CASES = [
    (40, 64, 64, "typical"), (40, 20, 128, "typical"), (1, 64, 64, "typical"),
    (256, 64, 64, "typical"), (1024, 64, 128, "typical"), (2048, 24, 256, "typical"),
    (1000, 64, 64, "typical"), (1000, 20, 128, "typical"), (1000, 64, 256, "typical"),
    (1000, 64, 64, "tile0_zero"), (1000, 64, 128, "tile0_zero"), (1000, 24, 256, "tile0_zero"),
    (2048, 64, 256, "tile0_zero"),
    (66000, 64, 64, "typical"), (66000, 64, 64, "tile0_zero"),
]


def channel_params(C, seed):
    """m_c in [-2, 2], s_c in [0.5, 2], gamma in [0.5, 1.5], beta in [-0.5, 0.5] (float32)"""
    g = np.random.default_rng(seed)
    return (g.uniform(-2, 2, C).astype(f32), g.uniform(0.5, 2, C).astype(f32),
            g.uniform(0.5, 1.5, C).astype(f32), g.uniform(-0.5, 0.5, C).astype(f32))


@functools.lru_cache(maxsize=None)
def stats_case(case):
    """(partials fp32 [nt][C][2], gamma) of a STATS_CASES entry, built from float64 data"""
    M, C, tile_rows, kind = case
    m, s, gamma, _ = channel_params(C, seed=M + C + tile_rows)
    g = np.random.default_rng(7 * M + tile_rows)
    if kind == "tile0_zero":
        x = 3.0 + g.standard_normal((M, C)) * s.astype(np.float64)
        x[:tile_rows] = 0.0
    else:
        x = m.astype(np.float64) + g.standard_normal((M, C)) * s.astype(np.float64)
        x[:, 0] = 1.5
    part = tile_partials(x, tile_rows)
    part.setflags(write=False)
    return part, gamma


@functools.lru_cache(maxsize=1)
def stats_k():
    """(k_mean, k_var, worst float32-restatement ratios): 4 x the worst err / (e x scale) of the
    float32 restatement over STATS_CASES (sums in the kernel's lane order)"""
    worst = {"k_mean": 0.0, "k_var": 0.0}
    for case in STATS_CASES:
        part, gamma = stats_case(case)
        r = stats_check(stats_restate_f32(part, case[0], case[2], gamma), part, case[0], case[2],
                        gamma, 1.0, 1.0)
        for k in worst:
            worst[k] = max(worst[k], r[k][1])
    return 4.0 * worst["k_mean"], 4.0 * worst["k_var"], worst


def layer_inputs(M, C, dtype, seed, dz_dtype=None):
    """One layer's well-conditioned inputs: y ~ N(m_c, s_c) and dz ~ N(0.1, 1) rounded to their
    storage types (float32 values), mean / invstd from the float64 moments of y rounded to fp32,
    scale = gamma invstd, and a second tensor r ~ N(0, 1) of y's type (residual / z source)."""
    m, s, gamma, beta = channel_params(C, seed)
    g = np.random.default_rng(seed + 1000)
    y = round_to(m + s * g.standard_normal((M, C)).astype(f32), dtype)
    dz = round_to(f32(0.1) + g.standard_normal((M, C)).astype(f32), dz_dtype or dtype)
    r = round_to(g.standard_normal((M, C)).astype(f32), dtype)
    y64 = y.astype(np.float64)
    mean = y64.mean(0).astype(f32)
    invstd = (1.0 / np.sqrt(y64.var(0) + BN_EPS)).astype(f32)
    return {"y": y, "dz": dz, "r": r, "mean": mean, "invstd": invstd, "gamma": gamma, "beta": beta,
            "scale": gamma * invstd}


# ---- forward apply --------------------------------------------------------------------------
def res_rows(M, rs, Ho, Wo, Hr, Wr, mutant=None):
    """the residual's row of each output row: row (n, ho rs, wo rs) of the [N][Hr][Wr] grid.
    Mutant 'wo_for_wr': the row pitch taken from the output grid."""
    m = np.arange(M, dtype=np.int64)
    if rs <= 1:
        return m
    wo, t = m % Wo, m // Wo
    ho, n = t % Ho, t // Ho
    return (n * Hr + ho * rs) * (Wo if mutant == "wo_for_wr" else Wr) + wo * rs


def apply_ref(y, mean, scale, beta, relu, out_dtype, res=None, sub=None, y2=None, bn2=None):
    """float64 out = act((y - mean) scale + beta [+ res | + bn2(y2)]) and its per-element bound.
    y, res, y2: float arrays [M][C] as the kernel read them (res: its own rows; sub = (rs, Ho,
    Wo, Hr, Wr)); bn2 = (mean2, scale2, beta2); out_dtype: the stored type."""
    y = np.asarray(y, np.float64)
    mean, scale, beta = (np.asarray(v, np.float64) for v in (mean, scale, beta))
    ref = (y - mean) * scale + beta
    mag = np.abs(y - mean) * np.abs(scale) + np.abs(beta)
    if y2 is not None:
        m2, s2, b2 = (np.asarray(v, np.float64) for v in bn2)
        y2 = np.asarray(y2, np.float64)
        ref = ((y2 - m2) * s2 + b2) + ref
        mag = mag + np.abs(y2 - m2) * np.abs(s2) + np.abs(b2)
    elif res is not None:
        r = np.asarray(res, np.float64)[res_rows(y.shape[0], *(sub or (1, 0, 0, 0, 0)))]
        ref = r + ref
        mag = mag + np.abs(r)
    if relu:
        ref = np.maximum(ref, 0.0)   # 1-Lipschitz: the pre-activation bound holds after it
    return ref, 4 * E * mag + UNIT[out_dtype] * np.abs(ref) + TINY[out_dtype]


def apply_restate_f32(y, mean, scale, beta, relu, out_dtype, res=None, sub=None, y2=None, bn2=None,
                      mutant=None):
    """the apply in float32 as bn.h states it; returns (stored out as float32, bits or None)"""
    y = np.asarray(y, f32)
    v = fma32(y - np.asarray(mean, f32), np.asarray(scale, f32), np.asarray(beta, f32))
    if y2 is not None:
        m2, s2, b2 = (np.asarray(t, f32) for t in bn2)
        v = fma32(np.asarray(y2, f32) - m2, s2, b2) + v
    elif res is not None:
        v = np.asarray(res, f32)[res_rows(y.shape[0], *(sub or (1, 0, 0, 0, 0)), mutant=mutant)] + v
    if relu:
        v = np.maximum(v, f32(0))
    out = round_to(v, out_dtype)
    bits = pack_bits(out > 0) if relu and y.shape[1] % 8 == 0 else None
    return out, bits


def apply_check(got, bits, ref, bound):
    """{name: (violations, ratio)}: the stored output against the bound; the bits (None: not
    written) exactly against the stored output, and against the reference's sign wherever the
    reference is further from 0 than its bound"""
    out = {"out": violations(got, ref, bound)}
    if bits is not None:
        C = got.shape[1]
        b = unpack_bits(bits, C)
        out["bits_vs_stored"] = (int((b != (np.asarray(got) > 0)).sum()), 0.0)
        sure = np.abs(ref) > bound
        out["bits_vs_ref"] = (int(((b != (ref > 0)) & sure).sum()), 0.0)
    return out


# ---- backward -------------------------------------------------------------------------------
def row_blocks(M, rb):
    """[(r0, r1)] of the reduce's row blocks (the trailing ones may be empty)"""
    rows_per = -(-M // rb)
    return [(min(b * rows_per, M), min((b + 1) * rows_per, M)) for b in range(rb)]


def bn_rowblocks(M):
    """bn_bwd_rowblocks: ~64 rows per block, at most 1024 blocks"""
    return max(1, min(1024, (M + 63) // 64))


def _gate(C, z, mask, mutant=None):
    if mask is not None:
        return unpack_bits(mask, C, mutant)
    if z is not None:
        return np.asarray(z) > 0
    return None


def bwd_ref(dz, y, mean, invstd, dtype, z=None, mask=None, dzscale=None, dshift=None,
            scale=None, beta=None):
    """float64 reference of the reduce + finalize of one layer, on the inputs as the kernel read
    them (dz, z, y: float arrays [M][C]; mask: bits [M][C/8]). Returns d (the gated gradient
    times dzscale, float64), dyhat (the gated gradient as stored: float32 values of `dtype`),
    xhat, the sums s1 = sum d, s2 = sum d xhat with the sums of their |terms|, and with beta the
    column sums cs of the forward output as stored (and cs_abs)."""
    dz32 = np.asarray(dz, f32)
    M, C = dz32.shape
    y = np.asarray(y, np.float64)
    g = _gate(C, z, mask)
    pre32 = dz32 + np.asarray(dshift, f32) if dshift is not None else dz32   # one fp32 rounding
    pre64 = np.asarray(dz, np.float64) + (np.asarray(dshift, np.float64) if dshift is not None else 0.0)
    if g is not None:
        pre32 = np.where(g, pre32, f32(0))
        pre64 = np.where(g, pre64, 0.0)
    d = pre64 * np.asarray(dzscale, np.float64) if dzscale is not None else pre64
    xhat = (y - np.asarray(mean, np.float64)) * np.asarray(invstd, np.float64)
    out = {"d": d, "dyhat": round_to(pre32, dtype), "xhat": xhat, "M": M,
           "s1": d.sum(0), "s1_abs": np.abs(d).sum(0),
           "s2": (d * xhat).sum(0), "s2_abs": np.abs(d * xhat).sum(0)}
    if beta is not None:
        v = round_to(np.maximum(fma32(np.asarray(y, f32) - np.asarray(mean, f32), np.asarray(scale, f32),
                                      np.asarray(beta, f32)), f32(0)), dtype).astype(np.float64)
        out["cs"], out["cs_abs"] = v.sum(0), np.abs(v).sum(0)
    return out


def sum_bound(ref, absterms, M):
    return 1e-6 * np.abs(ref) + 4 * E * np.sqrt(M) * absterms


def bwd_sums_check(got, ref, frozen=False):
    """got: dict with any of dbeta, dgamma, sdy, sdyx ([C]), part ([rb][C][2]), cs_part
    ([rb][C]) as the native calls wrote them; ref: bwd_ref's dict"""
    M = ref["M"]
    b1, b2 = sum_bound(ref["s1"], ref["s1_abs"], M), sum_bound(ref["s2"], ref["s2_abs"], M)
    out = {}
    if got.get("dbeta") is not None:
        out["dbeta"] = violations(got["dbeta"], ref["s1"], b1)
    if got.get("dgamma") is not None:
        out["dgamma"] = violations(got["dgamma"], ref["s2"], b2)
    if got.get("part") is not None:   # the partials' sum over the row blocks, in float64
        p = np.asarray(got["part"], np.float64).sum(0)
        out["part_s1"] = violations(p[:, 0], ref["s1"], b1)
        out["part_s2"] = violations(p[:, 1], ref["s2"], b2)
    if got.get("sdy") is not None:
        k = 0.0 if frozen else 1.0 / M
        out["sdy"] = violations(got["sdy"], k * ref["s1"], k * b1)
        out["sdyx"] = violations(got["sdyx"], k * ref["s2"], k * b2)
    if got.get("cs_part") is not None:
        cs = np.asarray(got["cs_part"], np.float64).sum(0)
        out["cs_part"] = violations(cs, ref["cs"], sum_bound(ref["cs"], ref["cs_abs"], M))
    return out


def dyhat_check(got, ref):
    """the stored gated gradient, bit for bit (as values: +0 and -0 are one)"""
    return {"dyhat": (int((np.asarray(got, f32) != ref["dyhat"]).sum()), 0.0)}


def dy_check(got, ref, scale, sdy, sdyx, dtype):
    """the backward apply's dy = scale (d - sdy - xhat sdyx) on the sdy / sdyx it was given"""
    scale, sdy, sdyx = (np.asarray(v, np.float64) for v in (scale, sdy, sdyx))
    r = scale * (ref["d"] - sdy - ref["xhat"] * sdyx)
    bound = UNIT[dtype] * np.abs(r) + TINY[dtype] + \
        4 * E * np.abs(scale) * (np.abs(ref["d"]) + np.abs(sdy) + np.abs(ref["xhat"] * sdyx))
    return {"dy": violations(got, r, bound)}, r


def bwd_restate_f32(dz, y, mean, invstd, scale, dtype, rb, z=None, mask=None, dzscale=None,
                    dshift=None, beta=None, frozen=False, y2=None, mean2=None, invstd2=None,
                    scale2=None, mutant=None):
    """reduce, finalize and apply in float32 as bn.h states them, row block by row block.
    Returns part [rb][C][2], dbeta, dgamma, sdy, sdyx, dyhat and dy (values of `dtype`), with
    beta cs_part [rb][C], and with y2 the second layer's part2 / dbeta2 / dgamma2 / sdy2 / sdyx2 /
    dy2 (the dual launches). Mutants: 'drop_last_row' (row M - 1 missing from the sums),
    'cs_tail_zero_row' (one zero-filled row past the last block counted in cs_part),
    'dshift_after_gate', 'dzscale_on_dyhat', 'bit_reversed', 'neighbour_byte', 'dual_cross'
    (the first layer's sum of dyhat xhat written into the second layer's partials)."""
    dz = np.asarray(dz, f32)
    y = np.asarray(y, f32)
    M, C = dz.shape
    mean, invstd, scale = (np.asarray(v, f32) for v in (mean, invstd, scale))
    g = _gate(C, z, mask, mutant)
    pre = dz
    if dshift is not None and mutant != "dshift_after_gate":
        pre = pre + np.asarray(dshift, f32)
    if g is not None:
        pre = np.where(g, pre, f32(0))
    if dshift is not None and mutant == "dshift_after_gate":
        pre = pre + np.asarray(dshift, f32)
    d = pre * np.asarray(dzscale, f32) if dzscale is not None else pre
    xhat = (y - mean) * invstd
    t1, t2 = d, d * xhat
    if y2 is not None:
        xhat2 = (np.asarray(y2, f32) - np.asarray(mean2, f32)) * np.asarray(invstd2, f32)
        t3 = d * xhat2
    fwd = None
    if beta is not None:
        fwd = round_to(np.maximum(fma32(y - mean, scale, np.asarray(beta, f32)), f32(0)), dtype)
    blocks = row_blocks(M, rb)
    part = np.zeros((rb, C, 2), f32)
    part2 = np.zeros((rb, C, 2), f32)
    cs = np.zeros((rb, C), f32)
    last = max(b for b, (r0, r1) in enumerate(blocks) if r1 > r0)
    for b, (r0, r1) in enumerate(blocks):
        r1s = r1 - 1 if (mutant == "drop_last_row" and b == last) else r1
        part[b, :, 0] = np.add.reduce(t1[r0:r1s], axis=0, dtype=f32)
        part[b, :, 1] = np.add.reduce(t2[r0:r1s], axis=0, dtype=f32)
        if y2 is not None:
            part2[b, :, 0] = part[b, :, 0]
            part2[b, :, 1] = part[b, :, 1] if mutant == "dual_cross" else np.add.reduce(t3[r0:r1s], axis=0, dtype=f32)
        if fwd is not None:
            cs[b] = np.add.reduce(fwd[r0:r1], axis=0, dtype=f32)
            if mutant == "cs_tail_zero_row" and b == last:
                cs[b] = cs[b] + round_to(np.maximum(fma32(f32(0) - mean, scale, np.asarray(beta, f32)), f32(0)), dtype)

    def finalize(p):
        s1 = np.add.reduce(p[:, :, 0], axis=0, dtype=f32)
        s2 = np.add.reduce(p[:, :, 1], axis=0, dtype=f32)
        zero = np.zeros_like(s1)
        return s1, s2, (zero if frozen else s1 / f32(M)), (zero if frozen else s2 / f32(M))

    dbeta, dgamma, sdy, sdyx = finalize(part)
    out = {"part": part, "dbeta": dbeta, "dgamma": dgamma, "sdy": sdy, "sdyx": sdyx,
           "dyhat": round_to(d if mutant == "dzscale_on_dyhat" else pre, dtype),
           "dy": round_to(scale * (d - sdy - xhat * sdyx), dtype)}
    if fwd is not None:
        out["cs_part"] = cs
    if y2 is not None:
        dbeta2, dgamma2, sdy2, sdyx2 = finalize(part2)
        out.update(part2=part2, dbeta2=dbeta2, dgamma2=dgamma2, sdy2=sdy2, sdyx2=sdyx2,
                   dy2=round_to(np.asarray(scale2, f32) * (d - sdy2 - xhat2 * sdyx2), dtype))
    return out
