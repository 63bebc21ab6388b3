"""Plain numpy references, derived error bounds and an fp32 model for the image stem
(csrc/stem.hip; DESIGN.md "Image stem contract"). Nothing here uses a kernel of the project or
the oracle package.

Bit-exact references (the kernels do no arithmetic whose order is free, or none at all):
patch im2col (fp32 normalisation 2*(x/255)-1 in the reference's order, one bf16 rounding, a
gather), the two max-pools (first maximum in raster order; the backward sums fp32 in window raster
order and rounds once to bf16), SAME im2col, col2im (fp32 sum in tap order).

Bounds: worst-case fp32 bounds that hold for ANY summation order, u = 2^-24 per rounding,
gam(n) = n u / (1 - n u) for n chained roundings. They are derived, not tuned to a kernel;
tests/test_stem_ref_cpu.py keeps them honest (an fp32 model of the general kernel's order stays
within half of each, every mutant exceeds one of them by 4x).

Stem conv, per output: the bf16 x bf16 products are exact in fp32, so only the additions round:
432 products and the bias, in any grouping (the MFMA's included):
  |conv - conv64| <= gam(433) (sum_k |a_k w_k| + |bias|)
Weight gradient, per (channel, k): one product per patch (G is non-zero at the argmax position
only), summed inside a workgroup, then over the slab rows, then onto the existing gradient:
  |dw - dw64| <= gam(patches + slabs + 1) (sum_p |g_p a_p| + |dw0|)

GroupNorm + gelu forward, N = R C / G values per (sample, group), T_R / T_T the assumed ulp errors
of the device rsqrtf / tanhf (1 ulp <= 2 u relative):
  mean   |mean - mean64| <= gam(N + 1) mean_N|x|     (N - 1 additions, one division)
  rstd   |rstd / rstd64 - 1| <= gam(1.5 N + 3) amp + 2 T_R u,  amp = (mu^2 + var + eps)/(var + eps)
         E[x^2]: N + 1 roundings of terms, sums and division, relative (all terms positive).
         mean^2: 2 |mean| dmean + u mean^2 <= (2 N + 3) u E[x^2] (|mean|, mean|x| <= sqrt E[x^2]).
         The subtraction and + eps: 2 u E[x^2]. All over var + eps — the cancellation of
         E[x^2] - mu^2 multiplies by amp — and halved by the -1/2 power.
  z      z = (x - mean) rstd gamma + beta:
         |dz| <= |gamma| rstd64 ((1 + rho + 3u) dmean + |x - mean64| (rho + 3 u)) + u |z64|
         (rho the rstd bound; three roundings of the difference and the two products, one of the
         final addition; a contracted multiply-add only removes roundings.)
  y      gelu(z) = z/2 (1 + tanh(a)), a = k0 (z + k1 z^3). Against the float64 gelu(z64):
         sup|gelu'| <= D1 = 1.13 times dz, plus the evaluation: a carries 7 u |a| (k1 and k0 as
         fp32 constants, three products and a sum; k0 k1 |z|^3 <= |a|), tanh moves by at most
         sech^2(a) 7 u |a| <= 3.2 u (sup |a| sech^2 a < 0.448), tanhf adds 2 T_T u |tanh| <= 2 T_T u:
         e_th = (3.2 + 2 T_T) u absolute. 1 + tanh rounds once; z/2 is exact, its product once, and
         one more is granted: gelu_eval = |z|/2 (e_th + u (1 + tanh a)) + 2 u |gelu|.
         |y - y64| <= 2^-8 |y64| + (1 + 2^-8) (D1 dz + gelu_eval)     (one bf16 rounding)

Backward, on the fp32 mean / rstd handed to the kernel (so the cancellation amplifies nothing),
xh = (x - mean) rstd, z = xh gamma + beta, dz = dy gelu'(z), dxh = dz gamma, m1 / m2 the group means
of dxh / dxh xh, dx = rstd (dxh - m1 - xh m2) (+ prior):
  xh: 2 u |xh|.  z: 3 u |xh gamma| + u |z| =: ez.
  gelu'(z) = (1 + th)/2 + z/2 (1 - th^2) a'(z), a' = k0 (1 + 3 k1 z^2):
         e_gp = D2 ez (sup|gelu''| <= D2 = 0.81) + e_th / 2 + u ((1 + th)/2)
                + |z|/2 a' (2 e_th + 2 u) (1 - th^2: th^2 moves by 2 e_th and rounds, the
                difference rounds) + 8 u |second term| (its eight products and sums) + u |gelu'|.
  dz: |dy| e_gp + u |dz| =: edz.   dxh: |gamma| edz + u |dxh| =: edxh.
  m1: mean(edxh) + gam(N) mean|dxh|.   m2: mean(edxh |xh| + 3 u |dxh xh|) + gam(N) mean|dxh xh|.
  dx: rstd (edxh + em1 + |xh| em2 + 3 u |xh m2| + 2 u S) + u rstd S, S = |dxh| + |m1| + |xh m2|
         (xh and the product xh m2; two subtractions; the product with rstd), + u (|dx| + |prior|)
         when accumulated onto prior.
  dgamma |dgamma - (init + sum dz xh)| <= sum(edz |xh| + 3 u |dz xh|) + gam(B R + 1) (sum|dz xh| + |init|)
  dbeta  |dbeta - (init + sum dz)| <= sum edz + gam(B R + 1) (sum|dz| + |init|)
         (B R additions in any order, the fp32 atomics of the B workgroups among them.)

Model: fp32 numpy in the general kernels' order — thread (r0, c) sums rows r0, r0 + 256/C, ...,
then thread g sums the 256/C partials x C/G channels of its group in order. Its mutants are flags."""
import numpy as np

U = 2.0 ** -24
BF = 2.0 ** -8            # bf16 unit roundoff
F32, F64 = np.float32, np.float64
EPS = 1e-6
ULP_RSQRT = 2.0           # assumed ulp error of the device rsqrtf (DESIGN.md "Image stem contract")
ULP_TANH = 2.0            # assumed ulp error of the device tanhf
GELU_D1 = 1.13            # sup |gelu'|  (checked numerically in tests/test_stem_ref_cpu.py)
GELU_D2 = 0.81            # sup |gelu''|
K0, K1 = 0.7978845608028654, 0.044715
E_TH = (3.2 + 2.0 * ULP_TANH) * U
GN_NT = 256               # threads of every GroupNorm kernel
CONV_TERMS = 433          # 432 products and the bias


def gam(n):
    return n * U / (1.0 - n * U)


def bf16_round(a):
    """fp32 -> nearest-even bf16, as fp32 (finite values)."""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
    r = ((b >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((b + r) & np.uint32(0xFFFF0000)).view(F32)


def ratio(got, ref, bound, relative=False):
    """max over elements of |got - ref| / bound (|got / ref - 1| / bound when relative); 0 where
    the difference is exactly 0, whatever the bound."""
    got, ref, bound = (np.asarray(a, dtype=F64) for a in (got, ref, bound))
    err = np.abs(got / ref - 1.0) if relative else np.abs(got - ref)
    assert np.isfinite(err).all(), "non-finite value"
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(q.max())


def gn_expected_nv(R, C):
    """NV of the register-resident GroupNorm kernels for (R, C), 0 for the general kernel: the one
    statement of the rule that gn_reg_nv (stem.hip) must agree with."""
    if C < 4 or C > 256 or C & (C - 1) or (R * C) % (GN_NT * 4):
        return 0
    nv = R * C // (GN_NT * 4)
    return nv if nv in (4, 8, 16, 32) else 0


def im2col_expected_form(u8, P, KW, C):
    """Form of mmt_patch_im2col: 0 generic, 1 row-segment, 2 LDS-staged (the rule of stem.hip)."""
    if KW * C != 36:
        return 0
    return 2 if u8 and (P * C) % 4 == 0 and P * P * C * 16 <= 65536 else 1


# ------------------------------------------------------------------ patch im2col (bit-exact)
def normalize_bf16(img, normalize):
    """uint8 or fp32 pixels -> fp32 2*(x/255)-1 in that order (or x itself) -> bf16, as fp32."""
    x = np.asarray(img).astype(F32)
    if normalize:
        x = F32(2) * (x / F32(255)) - F32(1)
    return bf16_round(x)


def patch_im2col_ref(img, P, KH, KW, S, normalize):
    """img (B, I, H, H, C) -> (B*I*NP*OH*OW, KH*KW*C) bf16 values as fp32, rows in (b, i, patch
    raster, oy, ox) order, columns (ky, kx, c)."""
    xb = normalize_bf16(img, normalize)
    B, I, H, _, C = xb.shape
    PPD = H // P
    OH, OW = (P - KH) // S + 1, (P - KW) // S + 1
    pt = xb.reshape(B, I, PPD, P, PPD, P, C).transpose(0, 1, 2, 4, 3, 5, 6)   # (B, I, py, px, y, x, C)
    iy = (np.arange(OH) * S)[:, None, None, None] + np.arange(KH)[None, None, :, None]
    ix = (np.arange(OW) * S)[None, :, None, None] + np.arange(KW)[None, None, None, :]
    win = pt[:, :, :, :, iy, ix, :]                      # (B, I, py, px, OH, OW, KH, KW, C)
    return np.ascontiguousarray(win).reshape(-1, KH * KW * C)


# ------------------------------------------------------------------ stem conv and weight gradient
def stem_conv_ref(A, w, bias):
    """A (npatch*9, 432) and w (64, 432) bf16 values, bias (64): float64 conv (npatch, 9, 64) and
    its elementwise bound."""
    A, w, bias = (np.asarray(a, dtype=F64) for a in (A, w, bias))
    ref = (A @ w.T + bias).reshape(-1, 9, 64)
    bound = gam(CONV_TERMS) * (np.abs(A) @ np.abs(w).T + np.abs(bias)).reshape(-1, 9, 64)
    return ref, bound


def pool_gradient(dpooled, arg, win):
    """G (npatch, win, C) fp32: bf16(dpooled) at the slot arg, else 0 (maxpool_patch_bwd)."""
    dpooled, arg = np.asarray(dpooled, dtype=F32), np.asarray(arg).astype(np.int64)
    n, C = dpooled.shape
    G = np.zeros((n, win, C), F32)
    np.put_along_axis(G, arg[:, None, :], bf16_round(dpooled)[:, None, :], axis=1)
    return G


def stem_wgrad_ref(A, dpooled, arg, base, slabs):
    """float64 base + G^T . A (64, 432) with its bound; slabs: rows of the final column sum."""
    G = pool_gradient(dpooled, arg, 9).reshape(-1, 64).astype(F64)
    A, base = np.asarray(A, dtype=F64), np.asarray(base, dtype=F64)
    npatch = dpooled.shape[0]
    ref = base + G.T @ A
    bound = gam(npatch + slabs + 1) * (np.abs(G).T @ np.abs(A) + np.abs(base))
    return ref, bound


# ------------------------------------------------------------------ max-pools (bit-exact)
def maxpool_patch_ref(conv, win):
    """conv (npatch*win, C) -> pooled (npatch, C), slot of the first maximum."""
    v = np.asarray(conv, dtype=F32).reshape(-1, win, conv.shape[-1])
    return v.max(1), v.argmax(1).astype(np.uint8)        # argmax: the first occurrence


def _windows(x, KP):
    n, OH, OW, C = x.shape
    PH, PW = OH - KP + 1, OW - KP + 1
    return np.stack([x[:, dy:dy + PH, dx:dx + PW] for dy in range(KP) for dx in range(KP)], 3)


def maxpool2d_ref(x, KP, last=False):
    """x (npatch, OH, OW, C) -> pooled (npatch, PH, PW, C) and the window slot dy*KP + dx of the
    first maximum in raster order (last=True: the mutant that takes the last one)."""
    w = _windows(np.asarray(x, dtype=F32), KP)
    if last:
        arg = KP * KP - 1 - w[:, :, :, ::-1].argmax(3)
    else:
        arg = w.argmax(3)
    return w.max(3), arg.astype(np.uint8)


def maxpool2d_bwd_ref(dy, arg, OH, OW, KP):
    """dy (npatch, PH, PW, C) fp32, arg its slots -> bf16 (npatch, OH, OW, C) as fp32: each input
    sums, in fp32 and in window raster order, the dy of the windows that chose it."""
    dy, arg = np.asarray(dy, dtype=F32), np.asarray(arg).astype(np.int64)
    n, PH, PW, C = dy.shape
    acc = np.zeros((n, OH, OW, C), F32)
    ni, ci = np.arange(n)[:, None], np.arange(C)[None, :]
    for py in range(PH):
        for px in range(PW):
            s = arg[:, py, px, :]
            acc[ni, py + s // KP, px + s % KP, ci] += dy[:, py, px, :]
    return bf16_round(acc)


# ------------------------------------------------------------------ SAME im2col / col2im (bit-exact)
def im2col_same_ref(x, KS):
    """x (npatch, H, W, C) -> (npatch*H*W, KS*KS*C), zero padding KS//2, columns (ky, kx, c)."""
    x = np.asarray(x)
    n, H, W, C = x.shape
    h = KS // 2
    xp = np.zeros((n, H + 2 * h, W + 2 * h, C), x.dtype)
    xp[:, h:h + H, h:h + W] = x
    cols = np.stack([xp[:, ky:ky + H, kx:kx + W] for ky in range(KS) for kx in range(KS)], 3)
    return cols.reshape(n * H * W, KS * KS * C)


def col2im_same_ref(dcols, n, H, W, C, KS):
    """dcols (npatch*H*W, KS*KS*C) fp32 -> (npatch*H*W, C): the fp32 sum over the taps in (ky, kx)
    order of dcols[(p, y - ky + KS//2, x - kx + KS//2)][(ky, kx, c)], taps outside the map skipped."""
    d = np.asarray(dcols, dtype=F32).reshape(n, H, W, KS, KS, C)
    acc = np.zeros((n, H, W, C), F32)
    h = KS // 2
    for ky in range(KS):
        oy = h - ky                                      # source row = y + oy
        y0, y1 = max(0, -oy), min(H, H - oy)
        for kx in range(KS):
            ox = h - kx
            x0, x1 = max(0, -ox), min(W, W - ox)
            if y0 < y1 and x0 < x1:
                acc[:, y0:y1, x0:x1] += d[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox, ky, kx]
    return acc.reshape(n * H * W, C)


# ------------------------------------------------------------------ GroupNorm + gelu, float64
def gelu(z):
    return 0.5 * z * (1.0 + np.tanh(K0 * (z + K1 * z * z * z)))


def gelu_grad(z):
    th = np.tanh(K0 * (z + K1 * z * z * z))
    return 0.5 * (1.0 + th) + 0.5 * z * (1.0 - th * th) * K0 * (1.0 + 3.0 * K1 * z * z)


def _per_channel(s, cpg):
    """(B, G) group values -> (B, 1, C)."""
    return np.repeat(s, cpg, axis=1)[:, None, :]


def gn_fwd_ref(x, G, gamma, beta, eps=EPS):
    """x (B, R, C), gamma / beta (C): float64 mean, rstd (B, G), y (B, R, C) and their bounds
    (rstd's is relative) as a dict."""
    x, gamma, beta = (np.asarray(a, dtype=F64) for a in (x, gamma, beta))
    B, R, C = x.shape
    cpg = C // G
    N = R * cpg
    xg = x.reshape(B, R, G, cpg)
    mean = xg.mean((1, 3))
    m2 = (xg * xg).mean((1, 3))
    var = np.maximum(0.0, m2 - mean * mean)
    rstd = 1.0 / np.sqrt(var + eps)
    amp = (m2 + eps) / (var + eps)
    mean_bound = gam(N + 1) * np.abs(xg).mean((1, 3))
    rho = gam(1.5 * N + 3) * amp + 2.0 * ULP_RSQRT * U
    mu_c, rs_c = _per_channel(mean, cpg), _per_channel(rstd, cpg)
    dmu_c, rho_c = _per_channel(mean_bound, cpg), _per_channel(rho, cpg)
    z = (x - mu_c) * rs_c * gamma + beta
    ez = np.abs(gamma) * rs_c * ((1 + rho_c + 3 * U) * dmu_c + np.abs(x - mu_c) * (rho_c + 3 * U)) \
        + U * np.abs(z)
    y = gelu(z)
    th = np.tanh(K0 * (z + K1 * z ** 3))
    ev = 0.5 * np.abs(z) * (E_TH + U * (1.0 + th)) + 2 * U * np.abs(y)
    y_f32 = GELU_D1 * ez + ev
    return {"mean": mean, "rstd": rstd, "y": y, "z": z,
            "mean_bound": mean_bound, "rstd_bound": rho,
            "y_f32_bound": y_f32,                       # before the bf16 rounding of the store
            "y_bound": BF * np.abs(y) + (1 + BF) * y_f32}


def gn_bwd_ref(dy, x, G, gamma, beta, mean, rstd, prior=None, dgamma0=None, dbeta0=None):
    """The backward on the given (fp32) mean / rstd (B, G) in float64, with the bounds. prior: the
    dx it is accumulated onto; dgamma0 / dbeta0: what the accumulated gradients start from."""
    dy, x, gamma, beta, mean, rstd = (np.asarray(a, dtype=F64)
                                      for a in (dy, x, gamma, beta, mean, rstd))
    B, R, C = x.shape
    cpg = C // G
    N = R * cpg
    zc = np.zeros(C)
    dgamma0 = zc if dgamma0 is None else np.asarray(dgamma0, dtype=F64)
    dbeta0 = zc if dbeta0 is None else np.asarray(dbeta0, dtype=F64)

    def gmean(v):                                        # group mean, back on (B, 1, C)
        return _per_channel(v.reshape(B, R, G, cpg).mean((1, 3)), cpg)

    mu, rs = _per_channel(mean, cpg), np.abs(_per_channel(rstd, cpg))
    xh = (x - mu) * rs
    z = xh * gamma + beta
    th = np.tanh(K0 * (z + K1 * z ** 3))
    da = K0 * (1.0 + 3.0 * K1 * z * z)
    t2 = 0.5 * z * (1.0 - th * th) * da
    gp = 0.5 * (1.0 + th) + t2
    dz = dy * gp
    dxh = dz * gamma
    m1, m2 = gmean(dxh), gmean(dxh * xh)
    dx = rs * (dxh - m1 - xh * m2)
    ez = 3 * U * np.abs(xh * gamma) + U * np.abs(z)
    e_gp = GELU_D2 * ez + 0.5 * E_TH + U * 0.5 * (1.0 + th) + 0.5 * np.abs(z) * da * (2 * E_TH + 2 * U) \
        + 8 * U * np.abs(t2) + U * np.abs(gp)
    edz = np.abs(dy) * e_gp + U * np.abs(dz)
    edxh = np.abs(gamma) * edz + U * np.abs(dxh)
    em1 = gmean(edxh) + gam(N) * gmean(np.abs(dxh))
    em2 = gmean(edxh * np.abs(xh) + 3 * U * np.abs(dxh * xh)) + gam(N) * gmean(np.abs(dxh * xh))
    S = np.abs(dxh) + np.abs(m1) + np.abs(xh * m2)
    dx_bound = rs * (edxh + em1 + np.abs(xh) * em2 + 3 * U * np.abs(xh * m2) + 2 * U * S) + U * rs * S
    if prior is not None:
        prior = np.asarray(prior, dtype=F64)
        dx_bound = dx_bound + U * (np.abs(dx) + np.abs(prior))
        dx = dx + prior
    n = B * R + 1
    return {"dx": dx, "dx_bound": dx_bound,
            "dgamma": dgamma0 + (dz * xh).sum((0, 1)),
            "dgamma_bound": (edz * np.abs(xh) + 3 * U * np.abs(dz * xh)).sum((0, 1))
            + gam(n) * (np.abs(dz * xh).sum((0, 1)) + np.abs(dgamma0)),
            "dbeta": dbeta0 + dz.sum((0, 1)),
            "dbeta_bound": edz.sum((0, 1)) + gam(n) * (np.abs(dz).sum((0, 1)) + np.abs(dbeta0))}


# ------------------------------------------------------------------ fp32 model of the general kernels
def _thread_sums(v, C):
    """v (B, R, C) fp32 -> (B, rstep, C): thread (r0, c) sums rows r0, r0 + rstep, ... in order."""
    B, R, _ = v.shape
    rstep = GN_NT // C
    part = np.zeros((B, rstep, C), F32)
    for r in range(R):
        part[:, r % rstep] += v[:, r]
    return part


def _group_sums(part, G, stride=None):
    """(B, rstep, C) -> (B, G): group g sums its partials t = 0.., channels g*cpg + j in order.
    stride: the mutant that takes group g's channels at g + j*stride (a wrong channel stride)."""
    B, rstep, C = part.shape
    cpg = C // G
    s = np.zeros((B, G), F32)
    g = np.arange(G)
    for t in range(rstep):
        for j in range(cpg):
            s = s + part[:, t, (g * cpg + j) if stride is None else (g + j * stride) % C]
    return s


def _gelu32(z):
    k0, k1 = F32(K0), F32(K1)
    return F32(0.5) * z * (F32(1) + np.tanh(k0 * (z + k1 * z * z * z)))


def _gelu_grad32(z, second=True):
    k0, k1 = F32(K0), F32(K1)
    th = np.tanh(k0 * (z + k1 * z * z * z))
    g = F32(0.5) * (F32(1) + th)
    if second:
        g = g + F32(0.5) * z * (F32(1) - th * th) * k0 * (F32(1) + F32(3) * k1 * z * z)
    return g


def model_fwd(x, G, gamma, beta, eps=EPS, nm1=False, wrong_stride=False, prev_sample=False):
    """fp32 model of groupnorm_gelu_fwd_kernel: mean, rstd, y before and after the bf16 store.
    Mutants: nm1 (variance over N - 1), wrong_stride (a group's channels taken G apart),
    prev_sample (the statistics of sample b - 1 applied to sample b)."""
    x, gamma, beta = (np.asarray(a, dtype=F32) for a in (x, gamma, beta))
    B, R, C = x.shape
    cpg = C // G
    n = F32(R * cpg)
    stride = G if wrong_stride else None
    a = _group_sums(_thread_sums(x, C), G, stride)
    q = _group_sums(_thread_sums(x * x, C), G, stride)
    mean = a / n
    var = np.maximum(F32(0), q / n - mean * mean)
    if nm1:
        var = var * (n / (n - F32(1)))
    rstd = F32(1) / np.sqrt(var + F32(eps))
    mu_c, rs_c = _per_channel(mean, cpg), _per_channel(rstd, cpg)
    if prev_sample:
        mu_c, rs_c = np.roll(mu_c, 1, axis=0), np.roll(rs_c, 1, axis=0)
    y32 = _gelu32((x - mu_c) * rs_c * gamma + beta)
    return mean, rstd, y32, bf16_round(y32)


def model_bwd(dy, x, G, gamma, beta, mean, rstd, prior=None, dgamma0=None, dbeta0=None,
              drop_m2=False, drop_gelu2=False):
    """fp32 model of groupnorm_gelu_bwd_kernel: dx, dgamma, dbeta (one fp32 addition per sample
    onto the initial values). Mutants: drop_m2 (the xhat * mean(dxhat * xhat) term dropped),
    drop_gelu2 (the second term of gelu' dropped)."""
    dy, x, gamma, beta, mean, rstd = (np.asarray(a, dtype=F32)
                                      for a in (dy, x, gamma, beta, mean, rstd))
    B, R, C = x.shape
    cpg = C // G
    n = F32(R * cpg)
    mu, rs = _per_channel(mean, cpg), _per_channel(rstd, cpg)
    xh = (x - mu) * rs
    dz = dy * _gelu_grad32(xh * gamma + beta, second=not drop_gelu2)
    dxh = dz * gamma
    m1 = _per_channel(_group_sums(_thread_sums(dxh, C), G) / n, cpg)
    m2 = _per_channel(_group_sums(_thread_sums(dxh * xh, C), G) / n, cpg)
    if drop_m2:
        m2 = np.zeros_like(m2)
    dx = rs * (dz * gamma - m1 - xh * m2)
    if prior is not None:
        dx = dx + np.asarray(prior, dtype=F32)
    dgamma = np.zeros(C, F32) if dgamma0 is None else np.asarray(dgamma0, dtype=F32).copy()
    dbeta = np.zeros(C, F32) if dbeta0 is None else np.asarray(dbeta0, dtype=F32).copy()
    p3, p4 = _thread_sums(dz * xh, C), _thread_sums(dz, C)
    s3, s4 = np.zeros((B, C), F32), np.zeros((B, C), F32)
    for t in range(p3.shape[1]):
        s3 = s3 + p3[:, t]
        s4 = s4 + p4[:, t]
    for b in range(B):
        dgamma = dgamma + s3[b]
        dbeta = dbeta + s4[b]
    return dx, dgamma, dbeta


def gn_data(B, R, C, G, seed):
    """Inputs with a different offset and scale per sample and per group, so that a wrong sample
    or group index shows: x, gamma, beta, dy, prior (fp32)."""
    g = np.random.default_rng(seed)
    cpg = C // G
    off = np.repeat(g.uniform(-1.5, 1.5, (B, G)), cpg, axis=1)[:, None, :]
    sc = np.repeat(g.uniform(0.5, 2.0, (B, G)), cpg, axis=1)[:, None, :]
    x = (g.standard_normal((B, R, C)) * sc + off).astype(F32)
    gamma = (1 + 0.2 * g.standard_normal(C)).astype(F32)
    beta = (0.2 * g.standard_normal(C)).astype(F32)
    dy = g.standard_normal((B, R, C)).astype(F32)
    prior = g.standard_normal((B, R, C)).astype(F32)
    return x, gamma, beta, dy, prior
