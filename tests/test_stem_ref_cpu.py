"""CPU: the references and error bounds of tests/stem_ref.py are neither loose nor tight by accident.

GroupNorm + gelu, for every shape below:
* the fp32 numpy model of the general kernel's summation order stays within HALF of each derived
  bound. Two terms are a single rounding that reaches its worst case whatever the order, so no
  model can stay under half of them: the bf16 store of y (2^-8 |y|) and the fp32 addition of the
  prior dx. There the half is asked of what the kernel accumulates — y before the store, dx
  without prior — and the whole bound of the stored value;
* each mutant of the model exceeds a bound by at least 4x somewhere: the variance over N - 1, a
  group's channels taken at the wrong stride, the statistics of sample b - 1, the
  xhat * mean(dxhat * xhat) term dropped, the second term of gelu' dropped.
Where a mutant cannot change a value there is nothing to exceed, and the case is left out by rule,
not by result: N - 1 leaves the mean alone, the neighbour's statistics leave mean and rstd (the
outputs) alone, the wrong stride is the right one when a group is one channel or all of them.

Max-pool: on tied data the last-maximum mutant differs from the bit-exact first-maximum reference.
The other references are checked against literal loops on tiny shapes."""
import numpy as np
import pytest

from tests import stem_ref as S

HALF, FOUR = 0.5, 4.0
SHAPES = [(3, 12, 16, 4), (3, 5, 64, 32), (3, 33, 8, 2), (3, 40, 8, 8), (2, 6, 4, 1), (3, 7, 2, 1),
          (2, 3, 256, 64)]


def _fwd_ratios(ref, out):
    mean, rstd, y32, y = out
    return {"mean": S.ratio(mean, ref["mean"], ref["mean_bound"]),
            "rstd": S.ratio(rstd, ref["rstd"], ref["rstd_bound"], relative=True),
            "y_f32": S.ratio(y32, ref["y"], ref["y_f32_bound"]),
            "y": S.ratio(y, ref["y"], ref["y_bound"])}


@pytest.mark.parametrize("B,R,C,G", SHAPES)
def test_groupnorm_forward_bounds_hold_for_the_model_and_catch_the_mutants(B, R, C, G):
    x, gamma, beta, _, _ = S.gn_data(B, R, C, G, seed=R * C + G)
    ref = S.gn_fwd_ref(x, G, gamma, beta)
    r = _fwd_ratios(ref, S.model_fwd(x, G, gamma, beta))
    assert r["mean"] <= HALF and r["rstd"] <= HALF and r["y_f32"] <= HALF and r["y"] <= 1.0, r
    mutants = [("variance over N - 1", {"nm1": True}, ("rstd", "y")),
               ("statistics of sample b - 1", {"prev_sample": True}, ("y",))]
    if 1 < G < C:
        mutants.append(("wrong channel stride", {"wrong_stride": True}, ("mean", "rstd", "y")))
    for name, kw, changed in mutants:
        m = _fwd_ratios(ref, S.model_fwd(x, G, gamma, beta, **kw))
        for q in changed:
            assert m[q] >= FOUR, (name, q, m)


def _bwd_ratios(ref, out):
    dx, dgam, dbet = out
    return {"dx": S.ratio(dx, ref["dx"], ref["dx_bound"]),
            "dgamma": S.ratio(dgam, ref["dgamma"], ref["dgamma_bound"]),
            "dbeta": S.ratio(dbet, ref["dbeta"], ref["dbeta_bound"])}


@pytest.mark.parametrize("B,R,C,G", SHAPES)
def test_groupnorm_backward_bounds_hold_for_the_model_and_catch_the_mutants(B, R, C, G):
    x, gamma, beta, dy, prior = S.gn_data(B, R, C, G, seed=R * C + G)
    g = np.random.default_rng(R + C)
    dg0, db0 = (g.standard_normal(C).astype(np.float32) for _ in range(2))
    mean, rstd, _, _ = S.model_fwd(x, G, gamma, beta)
    # what the kernel accumulates, held to half: dx without the prior
    bare = S.gn_bwd_ref(dy, x, G, gamma, beta, mean, rstd, None, dg0, db0)
    r = _bwd_ratios(bare, S.model_bwd(dy, x, G, gamma, beta, mean, rstd, None, dg0, db0))
    assert r["dx"] <= HALF and r["dgamma"] <= HALF and r["dbeta"] <= HALF, r
    # onto the prior the last rounding alone can use all of its term
    ref = S.gn_bwd_ref(dy, x, G, gamma, beta, mean, rstd, prior, dg0, db0)
    r = _bwd_ratios(ref, S.model_bwd(dy, x, G, gamma, beta, mean, rstd, prior, dg0, db0))
    assert r["dx"] <= 1.0 and r["dgamma"] <= HALF and r["dbeta"] <= HALF, r
    for name, kw, changed in [("xhat mean(dxhat xhat) dropped", {"drop_m2": True}, ("dx",)),
                              ("second term of gelu' dropped", {"drop_gelu2": True},
                               ("dx", "dgamma", "dbeta"))]:
        m = _bwd_ratios(ref, S.model_bwd(dy, x, G, gamma, beta, mean, rstd, prior, dg0, db0, **kw))
        for q in changed:
            assert m[q] >= FOUR, (name, q, m)


def test_gelu_constants_of_the_bounds():
    """sup|gelu'| <= D1, sup|gelu''| <= D2 and sup |a| sech^2(a) < 0.448 on a dense grid (gelu''
    by the central difference of the closed-form gelu', step 1e-5: error far below the margin)."""
    z = np.linspace(-12.0, 12.0, 2_400_001)
    assert np.abs(S.gelu_grad(z)).max() <= S.GELU_D1 - 1e-3
    h = 1e-5
    assert np.abs((S.gelu_grad(z + h) - S.gelu_grad(z - h)) / (2 * h)).max() <= S.GELU_D2 - 1e-3
    assert (np.abs(z) / np.cosh(z) ** 2).max() < 0.448
    # the closed-form gradient is the derivative of gelu
    num = (S.gelu(z + h) - S.gelu(z - h)) / (2 * h)
    assert np.abs(num - S.gelu_grad(z)).max() < 1e-8


def test_expected_forms_state_the_dispatch():
    want = {(16, 256): 4, (128, 64): 8, (4096, 4): 16, (1024, 32): 32, (256, 128): 32, (32, 64): 0,
            (48, 64): 0, (1024, 64): 0, (100, 64): 0, (3, 64): 0, (5, 256): 0, (7, 2): 0,
            (2048, 2): 0, (64, 64): 4}
    assert {k: S.gn_expected_nv(*k) for k in want} == want
    assert S.im2col_expected_form(True, 16, 12, 3) == 2 and S.im2col_expected_form(True, 36, 12, 3) == 2
    assert S.im2col_expected_form(True, 40, 12, 3) == 1 and S.im2col_expected_form(False, 16, 12, 3) == 1
    assert S.im2col_expected_form(True, 16, 9, 4) == 2 and S.im2col_expected_form(True, 8, 2, 4) == 0


def _tied(shape, seed, levels=3):
    return np.random.default_rng(seed).integers(0, levels, shape).astype(np.float32)


@pytest.mark.parametrize("OH,OW,KP", [(7, 5, 3), (3, 9, 2)])
def test_maxpool_reference_takes_the_first_maximum_and_rejects_the_last(OH, OW, KP):
    n, C = 2, 4
    x = _tied((n, OH, OW, C), OH * OW)
    y, arg = S.maxpool2d_ref(x, KP)
    PH, PW = OH - KP + 1, OW - KP + 1
    dy = np.random.default_rng(1).standard_normal((n, PH, PW, C)).astype(np.float32)
    G = S.maxpool2d_bwd_ref(dy, arg, OH, OW, KP)
    # literal loops: strict > keeps the first maximum; the gather of the kernel's comment
    want = np.zeros((n, OH, OW, C), np.float32)
    for p in range(n):
        for py in range(PH):
            for px in range(PW):
                for c in range(C):
                    best, bi = x[p, py, px, c], 0
                    for d in range(KP * KP):
                        v = x[p, py + d // KP, px + d % KP, c]
                        if v > best:
                            best, bi = v, d
                    assert y[p, py, px, c] == best and arg[p, py, px, c] == bi
                    want[p, py + bi // KP, px + bi % KP, c] += dy[p, py, px, c]
    assert np.array_equal(G, S.bf16_round(want))
    # the mutant: last maximum. Same pooled values, another slot on ties, another gradient.
    y2, arg2 = S.maxpool2d_ref(x, KP, last=True)
    assert np.array_equal(y2, y) and (arg2 != arg).any()
    assert not np.array_equal(S.maxpool2d_bwd_ref(dy, arg2, OH, OW, KP), G)
    # per-patch pool: the window as the middle axis
    v = _tied((5 * KP * KP, C), 3)
    p, a = S.maxpool_patch_ref(v, KP * KP)
    v3 = v.reshape(5, KP * KP, C)
    assert np.array_equal(p, v3.max(1))
    assert all(v3[i, :a[i, c], c].max(initial=-1) < p[i, c] == v3[i, a[i, c], c]
               for i in range(5) for c in range(C))


@pytest.mark.parametrize("H,W,KS", [(5, 3, 3), (1, 4, 5), (2, 2, 1)])
def test_same_im2col_and_col2im_references_against_loops(H, W, KS):
    n, C = 2, 3
    g = np.random.default_rng(H * W + KS)
    x = g.standard_normal((n, H, W, C)).astype(np.float32)
    cols = S.im2col_same_ref(x, KS).reshape(n, H, W, KS, KS, C)
    d = g.standard_normal((n * H * W, KS * KS * C)).astype(np.float32)
    dx = S.col2im_same_ref(d, n, H, W, C, KS).reshape(n, H, W, C)
    d6 = d.reshape(n, H, W, KS, KS, C)
    want = np.zeros((n, H, W, C), np.float32)
    for y in range(H):
        for xx in range(W):
            for ky in range(KS):
                for kx in range(KS):
                    sy, sx = y + ky - KS // 2, xx + kx - KS // 2
                    inside = 0 <= sy < H and 0 <= sx < W
                    assert np.array_equal(cols[:, y, xx, ky, kx], x[:, sy, sx] if inside else
                                          np.zeros((n, C), np.float32))
                    ty, tx = y - ky + KS // 2, xx - kx + KS // 2
                    if 0 <= ty < H and 0 <= tx < W:
                        want[:, y, xx] += d6[:, ty, tx, ky, kx]
    assert np.array_equal(dx, want)
    # adjoint identity in float64
    lhs = (cols.reshape(-1).astype(np.float64) * d.reshape(-1)).sum()
    rhs = (x.astype(np.float64) * dx).sum()
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))


def test_patch_im2col_reference_against_loops():
    g = np.random.default_rng(5)
    img = g.integers(0, 256, (2, 2, 16, 16, 3), dtype=np.uint8)
    P, KH, KW, S_ = 8, 4, 2, 2
    out = S.patch_im2col_ref(img, P, KH, KW, S_, True)
    xb = S.normalize_bf16(img, True)
    assert xb[0, 0, 0, 0, 0] == S.bf16_round(np.float32(2) * (np.float32(img[0, 0, 0, 0, 0]) / np.float32(255))
                                             - np.float32(1))
    OH, OW = (P - KH) // S_ + 1, (P - KW) // S_ + 1
    row = 0
    for b in range(2):
        for i in range(2):
            for py in range(2):
                for px in range(2):
                    for oy in range(OH):
                        for ox in range(OW):
                            y0, x0 = py * P + oy * S_, px * P + ox * S_
                            assert np.array_equal(out[row], xb[b, i, y0:y0 + KH, x0:x0 + KW].reshape(-1))
                            row += 1
    assert row == out.shape[0]


def test_conv_and_wgrad_references_on_a_hand_case():
    g = np.random.default_rng(9)
    A = S.bf16_round(g.standard_normal((2 * 9, 432)).astype(np.float32))
    w = S.bf16_round((0.05 * g.standard_normal((64, 432))).astype(np.float32))
    bias = g.standard_normal(64).astype(np.float32)
    ref, bound = S.stem_conv_ref(A, w, bias)
    assert ref.shape == bound.shape == (2, 9, 64)
    k = float(np.dot(A[10].astype(np.float64), w[5].astype(np.float64)) + bias[5])
    assert abs(ref[1, 1, 5] - k) < 1e-12 and (bound > 0).all()
    dp = g.standard_normal((2, 64)).astype(np.float32)
    arg = g.integers(0, 9, (2, 64)).astype(np.uint8)
    base = g.standard_normal((64, 432)).astype(np.float32)
    ref, bound = S.stem_wgrad_ref(A, dp, arg, base, slabs=2)
    want = base[7].astype(np.float64) + sum(
        float(S.bf16_round(dp[p:p + 1, 7])[0]) * A[p * 9 + arg[p, 7]].astype(np.float64) for p in range(2))
    assert np.abs(ref[7] - want).max() < 1e-12
    assert np.allclose(bound[7], S.gam(5) * (sum(
        abs(float(S.bf16_round(dp[p:p + 1, 7])[0])) * np.abs(A[p * 9 + arg[p, 7]]).astype(np.float64)
        for p in range(2)) + np.abs(base[7])))
