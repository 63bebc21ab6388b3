"""Float64 reference, derived error bounds and an fp32 model of the sequence-axis LayerNorm family
(csrc/norm.hip, csrc/tome.hip; DESIGN.md "Sequence LayerNorm contract"), in numpy.

Reference: the operation's own formula on the same input values upcast to float64 — fast variance
max(0, E[x^2] - E[x]^2), y = (x - mean) * (rstd * gamma) + beta; the backward takes the fp32 mean
and rstd handed to the kernel, so it is tested on its own.

Bounds: first-order worst-case fp32 bounds that hold for ANY summation order, u = 2^-24 (one
rounding), L rows, per element. They are derived, not tuned to a kernel; tests/test_seqnorm_ref_cpu
keeps them honest (an fp32 model of the kernel's order stays within half of each, every mutant
exceeds each by 4x somewhere).

  amp = E[x^2] / (var64 + eps): what the cancellation in E[x^2] - E[x]^2 multiplies an error by.
  mean   |mean - mean64| <= (L + 1) u mean_L|x|
         (L - 1 additions, each <= u of the running sum <= u sum|x|; one division.)
  rstd   |rstd / rstd64 - 1| <= (1.5 L + 4) u amp
         (E[x^2]: L + 1 roundings of its terms, sums and division; mean^2: 2 (L + 1) + 1 relative,
         mean^2 <= E[x^2]; the subtraction and + eps: 2; all over var + eps, halved by the -1/2
         power: ((L + 1) + (2 L + 3) + 2) / 2 <= 1.5 L + 3, and one for rsqrt itself.)
  y      |y - y64| <= 2^-8 |y64| + (2 L + 8) u amp (|x mul| + |mean mul| + |beta|), mul = rstd64 gamma
         (the kernel computes x mul + (beta - mean mul): each product carries rstd's relative error
         and mean's; 2^-8 is the bf16 unit roundoff of the stored y.)

Backward, g = dy gamma, xh = (x - mean) rstd, G = |g| + mean_L|g| + |xh| mean_L|g xh|:
  dx     |dx - dx64| <= (L + 10) u rstd G + u |addend|
         xh: the subtraction of two given values and the product, 2 u |xh| — mean is an input here,
         so the cancellation in xh amplifies nothing. g: u |g|. mean(g): L u mean|g| for the terms
         and their sum, u for the division. mean(g xh): 4 u per term, (L - 1) u for the sum, u for
         the division: (L + 4) u mean|g xh|. xh mean(g xh): (L + 7) u |xh| mean|g xh|. The two
         subtractions, the product with rstd and the addition of addend add one u of their results
         each, every result <= rstd G (+ |addend|). Collected:
         u rstd (5 |g| + (L + 5) mean|g| + (L + 10) |xh| mean|g xh|) + u |addend|.
         A contracted multiply-add only removes roundings from this count.
  dx bf16 residual: 2^-8 |dx64| + (1 + 2^-8) times the above (the stored value's rounding).
  dgamma |dgamma - (init + sum dy xh)| <= (B L + 3) u (sum_{b,l}|dy xh| + |init|)
         (3 u per term: xh and the product; B L additions in any order, the initial value among
         them — the fp32 atomics of B workgroups.)
  dbeta  |dbeta - (init + sum dy)| <= B L u (sum_{b,l}|dy| + |init|)   (the terms are exact.)
  column sums of z (the fused dropout backward): the kernel adds the fp32 value f = dx * keep /
         keep_prob that it then rounds to z, so against the float64 sum of f (from the kernel's own
         dx): (B L + 2) u (sum|f| + |init|) — one rounding of f, B L additions; and against the
         float64 sum of z: that plus 2^-8 sum|z| (|f - z| <= 2^-8 |z|, half a bf16 ulp of z).

Model: fp32 numpy in the kernels' order — 32 row groups, group r summing rows r, r + 32, ... in
order, then the groups in order; the forward as x mul + (beta - mean mul). Mutants of the model
(`n_rows`, `div`): rows past L are row L - 1 again (the kernels clamp the row of an unconditional
load), so n_rows = L + 1 counts the last row twice, n_rows = L - 1 drops it, n_rows = 32 RPT is a
register-resident form whose clamped rows are not masked (their dy not zeroed); div = 32 RPT
divides by the padded row count instead of L."""
import os
import re

import numpy as np

U = 2.0 ** -24
BF = 2.0 ** -8           # bf16 unit roundoff
RG = 32                  # row groups of every kernel of the family
EPS = 1e-6
F32, F64 = np.float32, np.float64

# the row counts of the contract: 1, 2, around one row group (31, 32, 33), one L % 32 != 0 inside
# each form (97, 161, 225, 289, 353) and both sides of every dispatch boundary
L_LIST = [1, 2, 31, 32, 33, 97, 128, 129, 161, 192, 193, 225, 256, 257, 289, 320, 321, 353]


def _atoi(s):
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


def expected_rpt(L, x_bf16=False, dy_bf16=True):
    """Rows per thread of the form an entry point takes for L rows (L2 / L - r for the fused
    entries): 4 / 6 / 8 / 10 for L <= 128 / 192 / 256 / 320, else 0, the two-pass form. A
    register-resident form needs fp32 x and bf16 dy (the forward has no dy); MMT_SNB_RPT=0 in the
    environment turns them off. The one statement of the rule that snb_rpt (norm.hip) and
    mmt_tome_merge_seqnorm_fwd (tome.hip) must both agree with."""
    env = os.environ.get("MMT_SNB_RPT")
    if (env is not None and _atoi(env) == 0) or x_bf16 or not dy_bf16:
        return 0
    for rpt in (4, 6, 8, 10):
        if L <= RG * rpt:
            return rpt
    return 0


def bf16_round(a):
    """fp32 -> nearest-even bf16, as fp32 (finite values)."""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
    r = ((b >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((b + r) & np.uint32(0xFFFF0000)).view(F32)


# ------------------------------------------------------------------ float64 reference and bounds
def fwd_ref(x, gamma, beta, eps=EPS):
    """x (B, L, D), gamma / beta (D): float64 mean, rstd (B, D), y (B, L, D) and their bounds
    (rstd's is relative) as a dict."""
    x, gamma, beta = (np.asarray(a, dtype=F64) for a in (x, gamma, beta))
    L = x.shape[1]
    mean = x.mean(1)
    m2 = (x * x).mean(1)
    var = np.maximum(0.0, m2 - mean * mean)
    rstd = 1.0 / np.sqrt(var + eps)
    mul = rstd * gamma
    y = (x - mean[:, None]) * mul[:, None] + beta
    amp = m2 / (var + eps)
    y_f32 = (2 * L + 8) * U * amp[:, None] * (np.abs(x * mul[:, None]) + np.abs(mean * mul)[:, None]
                                              + np.abs(beta))
    return {"mean": mean, "rstd": rstd, "y": y,
            "mean_bound": (L + 1) * U * np.abs(x).mean(1),
            "rstd_bound": (1.5 * L + 4) * U * amp,
            "y_f32_bound": y_f32,                       # before the bf16 rounding of the store
            "y_bound": BF * np.abs(y) + y_f32}


def bwd_ref(dy, x, mean, rstd, gamma, addend=None, dgamma0=None, dbeta0=None, x_bf16=False):
    """The backward on the given (fp32) mean / rstd in float64, with the bounds. dgamma0 / dbeta0:
    the values the accumulated gradients start from."""
    dy, x, mean, rstd, gamma = (np.asarray(a, dtype=F64) for a in (dy, x, mean, rstd, gamma))
    B, L, D = x.shape
    z = np.zeros(D)
    dgamma0 = z if dgamma0 is None else np.asarray(dgamma0, dtype=F64)
    dbeta0 = z if dbeta0 is None else np.asarray(dbeta0, dtype=F64)
    add = np.zeros_like(x) if addend is None else np.asarray(addend, dtype=F64)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    mg, mgx = g.mean(1), (g * xh).mean(1)
    dx = rstd[:, None] * (g - mg[:, None] - xh * mgx[:, None]) + add
    G = np.abs(g) + np.abs(g).mean(1)[:, None] + np.abs(xh) * np.abs(g * xh).mean(1)[:, None]
    f32 = (L + 10) * U * np.abs(rstd)[:, None] * G + U * np.abs(add)
    return {"dx": dx, "dx_f32_bound": f32,
            "dx_bound": BF * np.abs(dx) + (1 + BF) * f32 if x_bf16 else f32,
            "dgamma": dgamma0 + (dy * xh).sum((0, 1)),
            "dgamma_bound": (B * L + 3) * U * (np.abs(dy * xh).sum((0, 1)) + np.abs(dgamma0)),
            "dbeta": dbeta0 + dy.sum((0, 1)),
            "dbeta_bound": B * L * U * (np.abs(dy).sum((0, 1)) + np.abs(dbeta0))}


def colsum_ref(f, z, init=None):
    """Column sums of the fused dropout backward: f (B, L, D) the float64 values dx * keep /
    keep_prob of the kernel's own dx, z (B, L, D) the bf16 values it stored. Returns the float64
    sums of f and of z with their bounds."""
    f, z = np.asarray(f, dtype=F64), np.asarray(z, dtype=F64)
    B, L, D = f.shape
    init = np.zeros(D) if init is None else np.asarray(init, dtype=F64)
    bf = (B * L + 2) * U * (np.abs(f).sum((0, 1)) + np.abs(init))
    return {"sum_f": init + f.sum((0, 1)), "sum_f_bound": bf,
            "sum_z": init + z.sum((0, 1)), "sum_z_bound": bf + BF * np.abs(z).sum((0, 1))}


def ratio(got, ref, bound, relative=False):
    """max over elements of |got - ref| / bound (|got / ref - 1| / bound when relative); 0 where
    the difference is exactly 0, whatever the bound."""
    got, ref, bound = (np.asarray(a, dtype=F64) for a in (got, ref, bound))
    err = np.abs(got / ref - 1.0) if relative else np.abs(got - ref)
    assert np.isfinite(err).all(), "non-finite value"
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(q.max())


# ------------------------------------------------------------------ fp32 model of the kernels
def _group_sum(v, L, n_rows):
    """v (B, L, D) fp32: the kernels' sum over rows — row i of n_rows (row min(i, L - 1) of v)
    into row group i % 32 in order, then the 32 groups in order."""
    B, _, D = v.shape
    part = np.zeros((B, RG, D), F32)
    for i in range(n_rows):
        part[:, i % RG] += v[:, min(i, L - 1)]
    s = np.zeros((B, D), F32)
    for r in range(RG):
        s = s + part[:, r]
    return s


def model_fwd(x, gamma, beta, eps=EPS, n_rows=None, div=None):
    """fp32 model of seqnorm_fwd_kernel: mean, rstd, y before and after the bf16 store."""
    x, gamma, beta = (np.asarray(a, dtype=F32) for a in (x, gamma, beta))
    L = x.shape[1]
    n_rows = L if n_rows is None else n_rows
    div = F32(L if div is None else div)
    mean = _group_sum(x, L, n_rows) / div
    var = np.maximum(F32(0), _group_sum(x * x, L, n_rows) / div - mean * mean)
    rstd = F32(1) / np.sqrt(var + F32(eps))
    mul = rstd * gamma
    y32 = x * mul[:, None] + (beta - mean * mul)[:, None]
    return mean, rstd, y32, bf16_round(y32)


def model_bwd(dy, x, mean, rstd, gamma, addend=None, dgamma0=None, dbeta0=None, n_rows=None,
              div=None, x_bf16=False):
    """fp32 model of seqnorm_bwd_kernel: dx before and after the store in the residual dtype,
    dgamma, dbeta (one fp32 addition per sample onto the initial values)."""
    dy, x, mean, rstd, gamma = (np.asarray(a, dtype=F32) for a in (dy, x, mean, rstd, gamma))
    B, L, D = x.shape
    n_rows = L if n_rows is None else n_rows
    div = F32(L if div is None else div)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    mg = _group_sum(g, L, n_rows) / div
    mgx = _group_sum(g * xh, L, n_rows) / div
    pg, pb = _group_sum(dy * xh, L, n_rows), _group_sum(dy, L, n_rows)
    dx32 = rstd[:, None] * (g - mg[:, None] - xh * mgx[:, None])
    if addend is not None:
        dx32 = dx32 + np.asarray(addend, dtype=F32)
    dgamma = np.zeros(D, F32) if dgamma0 is None else np.asarray(dgamma0, dtype=F32).copy()
    dbeta = np.zeros(D, F32) if dbeta0 is None else np.asarray(dbeta0, dtype=F32).copy()
    for b in range(B):
        dgamma = dgamma + pg[b]
        dbeta = dbeta + pb[b]
    return dx32, (bf16_round(dx32) if x_bf16 else dx32), dgamma, dbeta


def model_colsum(f, init=None, n_rows=None):
    """fp32 model of the fused column sums of f (B, L, D) fp32 (n_rows as above)."""
    f = np.asarray(f, dtype=F32)
    B, L, D = f.shape
    part = _group_sum(f, L, L if n_rows is None else n_rows)
    out = np.zeros(D, F32) if init is None else np.asarray(init, dtype=F32).copy()
    for b in range(B):
        out = out + part[b]
    return out
