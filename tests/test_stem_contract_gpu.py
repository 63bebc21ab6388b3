"""GPU: the image stem (csrc/stem.hip) against the references and derived bounds of
tests/stem_ref.py (DESIGN.md "Image stem contract"). Every test asserts the kernel form that ran
(_C.stem_last_route()) after the call, having first left another entry's route behind, so a
missing route assignment cannot hide behind the previous case. The shapes are the smallest that
reach each path: the second iteration of the persistent tile loops, a full and a partial tile in
one launch, every GroupNorm form on both sides of its dispatch boundaries, every im2col form,
non-square maps, tied maxima. No comparison excludes elements; every tolerance is exact or derived
in stem_ref. Each test prints its largest error / bound ratio."""
import numpy as np
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
from tests import stem_ref as S

pytestmark = pytest.mark.gpu

PAD = 16                      # slack elements on either side of an operand (a multiple of 16 B)
SENT = 0x5A5B                 # bit pattern of the slack of bf16 / uint8-pair outputs


def _dirty(dev, avoid=None):
    """Leave the route of another stem entry behind (not the one of the entry `avoid`)."""
    if avoid == _C.STEM_ROUTE_MAXPOOL_PATCH:
        K.col2im_same(torch.zeros((1, 8), device=dev), 1, 1, 1, 8, 1)
        assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_COL2IM_SAME)
    else:
        K.maxpool_patch(torch.zeros((1, 8), device=dev), 1)
        assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_MAXPOOL_PATCH)


def _nan_padded(a, dev):
    """fp32 array -> (buffer, view): the view is a slice of a NaN-filled buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), device=dev)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _sentinel_f32(shape, dev, value=-7.25e9):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), value, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def _slack_f32_untouched(buf, value=-7.25e9):
    return bool((buf[:PAD] == value).all()) and bool((buf[-PAD:] == value).all())


def _sentinel_bf16(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.int16, device=dev)
    return buf, buf.view(torch.bfloat16)[PAD:PAD + n].view(shape)


def _slack_bf16_untouched(buf):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())


def _np(t):
    return t.detach().float().cpu().numpy()


# ================================================================== fused conv + pool, wgrad
def _conv_weights(seed, dev):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn((64, 432), generator=g) * 0.05).bfloat16()
    bias = torch.randn(64, generator=g) * 0.1
    return w.to(dev), bias.to(dev)


def _check_conv_pool(img, w, bias, pooled, arg, what):
    """|pooled - ref64[arg]| <= bound[arg] and ref64[arg] >= max(ref64) - 2 max(bound), every
    element. Returns the im2col reference for the weight-gradient checks."""
    A = S.patch_im2col_ref(img.cpu().numpy(), 16, 12, 12, 2, True)
    ref, bound = S.stem_conv_ref(A, _np(w), _np(bias))
    a = arg.cpu().numpy().astype(np.int64)
    assert a.max() <= 8
    sel = np.take_along_axis(ref, a[:, None, :], 1)[:, 0]
    bsel = np.take_along_axis(bound, a[:, None, :], 1)[:, 0]
    r = S.ratio(_np(pooled), sel, bsel)
    print(f"stem_conv_pool {what}: error/bound {r:.4f}")
    assert r <= 1.0, r
    assert (sel >= ref.max(1) - 2 * bound.max(1)).all()
    return A


def _check_wgrad(A, img, dpooled, arg, base, dev, what):
    B, I, H = img.shape[:3]
    slabs = _C.call("mmt_stem_conv_wgrad_slabs", B, I, H)
    wg = base.clone()
    _dirty(dev)
    K.stem_conv_wgrad(img, dpooled, arg, wg)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_CONV_WGRAD)
    assert tuple(wg.shape) == (64, 432)
    ref, bound = S.stem_wgrad_ref(A, _np(dpooled), arg.cpu().numpy(), _np(base), slabs)
    r = S.ratio(wg.cpu().numpy(), ref, bound)
    print(f"stem_conv_wgrad {what}: error/bound {r:.4f}")
    assert r <= 1.0, r


# (6, 1, 528): PPD = 33, so a patch row is three tiles of 16, 16 and 1 patches, 99 tiles per image,
# 594 in all on a grid of 512. Tile t is tile t % 99 of its image and piece (t % 99) % 3 of its row.
# Workgroup 0 takes tiles 0 (piece 0: full) and 512 (512 - 5*99 = 17, piece 2: one patch);
# workgroup 2 takes tiles 2 (piece 2: one patch) and 514 (19, piece 1: full).
@pytest.mark.parametrize("B,I,H", [(520, 1, 16), (6, 1, 528), (1, 2, 288)])
def test_conv_pool_and_wgrad_tile_loops(dev, B, I, H):
    """(520, 1, 16): 520 one-patch tiles, eight workgroups run the loop twice. (6, 1, 528): a full
    then a one-patch tile in one workgroup and the reverse in another. (1, 2, 288): PPD = 18, a
    full then a partial tile within a row, one loop iteration."""
    g = torch.Generator().manual_seed(B * H + I)
    img = torch.randint(0, 256, (B, I, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    w, bias = _conv_weights(H, dev)
    _dirty(dev)
    pooled, arg = K.stem_conv_pool(img, w, bias)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_CONV_POOL)
    A = _check_conv_pool(img, w, bias, pooled, arg, (B, I, H))
    # weight gradient at the forward's argmax, accumulated into a non-zero gradient
    n = arg.shape[0]
    dpooled = torch.randn((n, 64), generator=g).to(dev)
    base = torch.randn((64, 432), generator=g).to(dev)
    _check_wgrad(A, img, dpooled, arg, base, dev, (B, I, H))


def test_conv_pool_constant_images(dev):
    """One image of a constant colour per channel, an all-0 and an all-255 image: all nine
    positions see identical operands, so the first maximum is position 0 everywhere and the pooled
    value is identical across the patches of an image."""
    H = 64
    img = torch.zeros((3, 1, H, H, 3), dtype=torch.uint8)
    img[0, 0, :, :, 0], img[0, 0, :, :, 1], img[0, 0, :, :, 2] = 10, 200, 77
    img[2] = 255
    img = img.to(dev)
    w, bias = _conv_weights(3, dev)
    _dirty(dev)
    pooled, arg = K.stem_conv_pool(img, w, bias)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_CONV_POOL)
    _check_conv_pool(img, w, bias, pooled, arg, "constant")
    assert int(arg.max()) == 0
    p = pooled.view(3, 16, 64)
    assert bool((p == p[:, :1]).all())
    assert not bool((p[0, 0] == p[1, 0]).all()) and not bool((p[1, 0] == p[2, 0]).all())


def test_wgrad_hand_made_argmax_and_slab_extent(dev):
    """A hand-made argmax: every channel of patch 0 at position 0, every channel of patch 1 at
    position 8, random elsewhere. Called on a sentinel slab: every element of the slab rows the
    launch owns is written (432 columns per channel, the k padding e >= 36 never among them), the
    row after them is untouched, and the column sum matches G^T . A within the bound."""
    B, I, H = 2, 1, 288                                   # 72 tiles: partial and full pieces
    g = torch.Generator().manual_seed(41)
    img = torch.randint(0, 256, (B, I, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    n = B * I * (H // 16) ** 2
    arg = torch.randint(0, 9, (n, 64), generator=g).to(torch.uint8)
    arg[0], arg[1] = 0, 8
    arg = arg.to(dev)
    dpooled = torch.randn((n, 64), generator=g).to(dev)
    base = torch.randn((64, 432), generator=g).to(dev)
    A = S.patch_im2col_ref(img.cpu().numpy(), 16, 12, 12, 2, True)
    _check_wgrad(A, img, dpooled, arg, base, dev, "hand-made argmax")
    slabs = _C.call("mmt_stem_conv_wgrad_slabs", B, I, H)
    assert slabs == 72
    slab = torch.full((slabs + 1, 64 * 432), float("nan"), device=dev)
    _dirty(dev)
    _C.call("mmt_stem_conv_wgrad", _C.ptr(img), B, I, H, _C.ptr(dpooled), _C.ptr(arg), _C.ptr(slab),
            slabs * 64 * 432, _C.stream_ptr())
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_CONV_WGRAD)
    assert bool(torch.isfinite(slab[:slabs]).all()) and bool(torch.isnan(slab[slabs]).all())
    got = base.double() + slab[:slabs].double().sum(0).view(64, 432)
    ref, bound = S.stem_wgrad_ref(A, _np(dpooled), arg.cpu().numpy(), _np(base), slabs)
    assert S.ratio(got.cpu().numpy(), ref, bound) <= 1.0


# ================================================================== GroupNorm + gelu
GN_CASES = [(16, 256, 32), (128, 64, 32), (4096, 4, 2), (1024, 32, 32), (256, 128, 1), (32, 64, 32),
            (48, 64, 32), (1024, 64, 32), (100, 64, 32), (3, 64, 32), (5, 256, 64), (7, 2, 1)]
GN_FORMS = [4, 8, 16, 32, 32, 0, 0, 0, 0, 0, 0, 0]


def _gn_run(dev, x, gamma, beta, dy, prior, G, accumulate, nv, what):
    """Forward and backward on NaN-padded inputs and sentinel-padded outputs, checked elementwise
    against float64 at the derived bounds. Returns the device results."""
    B, R, C = x.shape
    xb, xd = _nan_padded(x, dev)
    db, dyd = _nan_padded(dy, dev)
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    ybuf, y = _sentinel_bf16((B, R, C), dev)
    _dirty(dev)
    y, mean, rstd = K.groupnorm_gelu_fwd(xd, G, gd, bd, S.EPS, out=y)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_GN_GELU_FWD, nv)
    assert _slack_bf16_untouched(ybuf)
    ref = S.gn_fwd_ref(x, G, gamma, beta)
    r = {"mean": S.ratio(_np(mean), ref["mean"], ref["mean_bound"]),
         "rstd": S.ratio(_np(rstd), ref["rstd"], ref["rstd_bound"], relative=True),
         "y": S.ratio(_np(y), ref["y"], ref["y_bound"])}
    dg0 = np.linspace(-1, 1, C).astype(np.float32)
    db0 = np.linspace(2, -2, C).astype(np.float32)
    dgam, dbet = torch.from_numpy(dg0).to(dev), torch.from_numpy(db0).to(dev)
    if accumulate:
        dxbuf, dx = _nan_padded(prior, dev)
    else:
        dxbuf, dx = _sentinel_f32((B, R, C), dev)
    _dirty(dev)
    K.groupnorm_gelu_bwd(dyd, xd, G, gd, bd, mean, rstd, dgam, dbet, dx=dx, accumulate=accumulate)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_GN_GELU_BWD, nv)
    slack = torch.cat([dxbuf[:PAD], dxbuf[-PAD:]])
    assert bool(torch.isnan(slack).all()) if accumulate else _slack_f32_untouched(dxbuf)
    bref = S.gn_bwd_ref(dy, x, G, gamma, beta, _np(mean), _np(rstd), prior if accumulate else None,
                        dg0, db0)
    r.update({"dx": S.ratio(_np(dx), bref["dx"], bref["dx_bound"]),
              "dgamma": S.ratio(_np(dgam), bref["dgamma"], bref["dgamma_bound"]),
              "dbeta": S.ratio(_np(dbet), bref["dbeta"], bref["dbeta_bound"])})
    print(f"groupnorm_gelu {what} nv={nv} accumulate={accumulate}: error/bound "
          + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    return y, mean, rstd, dx, dgam, dbet


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("RCG,nv", list(zip(GN_CASES, GN_FORMS)), ids=[str(c) for c in GN_CASES])
def test_groupnorm_gelu_forms(dev, RCG, nv, accumulate):
    """Every form (general; register-resident with NV = 4 / 8 / 16 / 32), C = 256 (no shuffle),
    C = 4 (the longest shuffle chain), one channel per group, one group, and R*C / 1024 = 2, 3 and
    64 on the general side of the dispatch. B = 3 with a different offset and scale per sample and
    group."""
    R, C, G = RCG
    assert S.gn_expected_nv(R, C) == nv
    x, gamma, beta, dy, prior = S.gn_data(3, R, C, G, seed=R * C + G)
    _gn_run(dev, x, gamma, beta, dy, prior, G, accumulate, nv, (R, C, G))


def test_groupnorm_gelu_general_and_register_forms_agree(dev):
    """With one group and channel-uniform gamma / beta the operation does not depend on how the
    R*C values of a sample are split into rows: (256, 128) runs the NV = 32 register kernel,
    (16384, 2) the general one. Both within the bounds; whether they agree bit for bit is printed,
    not required (the summation orders differ)."""
    B, R, C = 3, 256, 128
    x, _, _, dy, prior = S.gn_data(B, R, C, 1, seed=77)
    out = {}
    for r, c in ((R, C), (R * C // 2, 2)):
        nv = S.gn_expected_nv(r, c)
        gamma, beta = np.full(c, 1.25, np.float32), np.full(c, -0.125, np.float32)
        res = _gn_run(dev, x.reshape(B, r, c), gamma, beta, dy.reshape(B, r, c),
                      prior.reshape(B, r, c), 1, False, nv, (r, c, 1))
        out[nv] = [t.reshape(-1).clone() for t in res[:4]]
    assert set(out) == {32, 0}
    same = {k: bool(torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                b.view(torch.int16) if b.dtype == torch.bfloat16 else b))
            for k, a, b in zip(("y", "mean", "rstd", "dx"), out[32], out[0])}
    print(f"groupnorm_gelu register vs general bit-identical: {same}")


# ================================================================== patch im2col
GEN, ROWS, LDS = _C.STEM_IM2COL_GENERIC, _C.STEM_IM2COL_ROWS, _C.STEM_IM2COL_LDS
I2C_CASES = [
    # dtype, B, I, H, P, KH, KW, S, C, normalize, form
    ("u8", 1, 2, 48, 16, 12, 12, 2, 3, True, LDS),      # I = 2, 18 patches: a partial group of 8
    ("u8", 1, 1, 32, 16, 8, 9, 1, 4, True, LDS),        # C != 3, OH = 9 != OW = 8
    ("u8", 1, 1, 72, 36, 12, 12, 2, 3, True, LDS),      # the largest P the LDS form takes
    ("u8", 1, 1, 80, 40, 12, 12, 2, 3, True, ROWS),     # past the LDS budget: row segments
    ("f32", 2, 1, 32, 16, 12, 12, 2, 3, False, ROWS),   # the model's call: fp32, not normalised
    ("f32", 2, 1, 32, 16, 12, 12, 2, 3, True, ROWS),
    ("u8", 2, 1, 16, 8, 4, 2, 2, 4, True, GEN),
    ("f32", 2, 1, 16, 8, 4, 2, 2, 4, False, GEN),
]


@pytest.mark.parametrize("dtype,B,I,H,P,KH,KW,S_,C,normalize,form", I2C_CASES)
def test_patch_im2col_forms(dev, dtype, B, I, H, P, KH, KW, S_, C, normalize, form):
    """Bit-exact against the gather reference, into a slice of a sentinel buffer, per form."""
    u8 = dtype == "u8"
    assert S.im2col_expected_form(u8, P, KW, C) == form
    g = np.random.default_rng(H + KW + C)
    if u8:
        img = g.integers(0, 256, (B, I, H, H, C), dtype=np.uint8)
    else:                                                # non-integer pixel values
        img = (g.random((B, I, H, H, C)) * 255.0 - (0.0 if normalize else 127.3)).astype(np.float32)
    ref = S.patch_im2col_ref(img, P, KH, KW, S_, normalize)
    buf, out = _sentinel_bf16(ref.shape, dev)
    _dirty(dev)
    K.patch_im2col(torch.from_numpy(img).to(dev), P, KH, KW, S_, normalize=normalize, out=out)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_PATCH_IM2COL, form, in_u8=u8)
    assert _slack_bf16_untouched(buf)
    want = torch.from_numpy(ref).bfloat16()
    assert torch.equal(want.float(), torch.from_numpy(ref))           # ref holds bf16 values
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


# ================================================================== general-map kernels
def _tied(shape, seed, levels=3):
    """Values on a few levels, so most windows hold ties."""
    return np.random.default_rng(seed).integers(0, levels, shape).astype(np.float32) - 1.0


@pytest.mark.parametrize("KP", [3, 2])
@pytest.mark.parametrize("OH,OW", [(7, 5), (3, 9)])
def test_maxpool2d_non_square_with_ties(dev, OH, OW, KP):
    n, C = 3, 16
    PH, PW = OH - KP + 1, OW - KP + 1
    x = _tied((n, OH, OW, C), 10 * OH + KP)
    _dirty(dev)
    y, arg = K.maxpool2d(torch.from_numpy(x).reshape(-1, C).to(dev), n, OH, OW, KP)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_MAXPOOL2D)
    want_y, want_arg = S.maxpool2d_ref(x, KP)
    assert (want_arg != S.maxpool2d_ref(x, KP, last=True)[1]).mean() > 0.25     # the data has ties
    assert np.array_equal(y.cpu().numpy().reshape(n, PH, PW, C), want_y)
    assert np.array_equal(arg.cpu().numpy().reshape(n, PH, PW, C), want_arg)
    dy = np.random.default_rng(OW).standard_normal((n, PH, PW, C)).astype(np.float32)
    _dirty(dev)
    G = K.maxpool2d_bwd(torch.from_numpy(dy).reshape(-1, C).to(dev), arg, n, OH, OW, KP)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_MAXPOOL2D_BWD)
    want = torch.from_numpy(S.maxpool2d_bwd_ref(dy, want_arg, OH, OW, KP)).bfloat16().reshape(-1, C)
    assert torch.equal(G.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("win", [9, 4])
def test_maxpool_patch_with_ties(dev, win, C):
    npatch = 37
    conv = _tied((npatch * win, C), win * C)
    _dirty(dev, avoid=_C.STEM_ROUTE_MAXPOOL_PATCH)
    pooled, arg = K.maxpool_patch(torch.from_numpy(conv).to(dev), win)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_MAXPOOL_PATCH)
    want_p, want_a = S.maxpool_patch_ref(conv, win)
    assert np.array_equal(pooled.cpu().numpy(), want_p) and np.array_equal(arg.cpu().numpy(), want_a)
    dp = np.random.default_rng(C).standard_normal((npatch, C)).astype(np.float32)
    buf, out = _sentinel_bf16((npatch * win, C), dev)
    _dirty(dev)
    K.maxpool_patch_bwd(torch.from_numpy(dp).to(dev), arg, win, out=out)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_MAXPOOL_PATCH_BWD)
    assert _slack_bf16_untouched(buf)
    want = torch.from_numpy(S.pool_gradient(dp, want_a, win)).bfloat16().reshape(-1, C)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("KS", [1, 3, 5])
@pytest.mark.parametrize("H,W", [(5, 3), (1, 4)])
def test_same_im2col_col2im_non_square(dev, H, W, KS, C):
    n = 3
    g = np.random.default_rng(H * 100 + W * 10 + KS + C)
    x = S.bf16_round(g.standard_normal((n, H, W, C)).astype(np.float32))
    xd = torch.from_numpy(x).bfloat16().reshape(-1, C).to(dev)
    _dirty(dev)
    cols = K.im2col_same(xd, n, H, W, KS)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_IM2COL_SAME)
    want = S.im2col_same_ref(x, KS)
    assert np.array_equal(cols.float().cpu().numpy(), want)
    d = g.standard_normal((n * H * W, KS * KS * C)).astype(np.float32)
    _dirty(dev)
    dx = K.col2im_same(torch.from_numpy(d).to(dev), n, H, W, C, KS)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_COL2IM_SAME)
    assert np.array_equal(dx.cpu().numpy(), S.col2im_same_ref(d, n, H, W, C, KS))
    # col2im is the adjoint of im2col: <im2col(x), d> == <x, col2im(d)> in float64, up to the
    # fp32 roundings of the at most KS*KS taps col2im adds per element
    lhs = float((want.astype(np.float64) * d).sum())
    rhs = float((x.reshape(-1, C).astype(np.float64) * dx.cpu().numpy()).sum())
    scale = float(np.abs(want.astype(np.float64) * d).sum())
    assert abs(lhs - rhs) <= S.gam(KS * KS) * scale, (lhs, rhs)


# ================================================================== every entry reports its route
def test_every_entry_sets_its_route_and_a_rejection_clears_it(dev):
    """After a launch the route names the entry; after a call rejected before its launch it reads
    NONE (the CPU argument tests cannot see that: without a launch the value never leaves NONE)."""
    lib = _C.lib()
    rng = torch.tensor([11, 3], dtype=torch.int32, device=dev)
    K.patch_positions(2, 1, 64, 16, 128, True, rng)
    assert _C.stem_last_route() == _C.stem_route(_C.STEM_ROUTE_PATCH_POSITIONS)
    assert lib.mmt_patch_positions(None, 0, 2, 1, 64, 16, 128, 1, 0, 16, 16, None) == -1
    assert _C.stem_last_route() == _C.STEM_ROUTE_NONE
    P = 1 << 20
    rejected = [
        lambda: lib.mmt_patch_im2col(None, 2, 1, 1, 16, 3, 16, 12, 12, 2, 1, P, None),
        lambda: lib.mmt_stem_conv_pool(None, 1, 1, 16, P, P, P, P, None),
        lambda: lib.mmt_stem_conv_wgrad(None, 1, 1, 16, P, P, P, 1 << 30, None),
        lambda: lib.mmt_maxpool_patch(None, 1, 1, 8, P, P, None),
        lambda: lib.mmt_maxpool_patch_bwd(None, P, 1, 1, 8, P, None),
        lambda: lib.mmt_groupnorm_gelu_fwd(None, 1, 1, 8, 1, 1e-6, P, P, P, P, P, None),
        lambda: lib.mmt_groupnorm_gelu_bwd(None, P, 1, 1, 8, 1, P, P, P, P, P, 0, P, P, None),
        lambda: lib.mmt_maxpool2d(None, 1, 3, 3, 8, 3, P, P, None),
        lambda: lib.mmt_maxpool2d_bwd(None, P, 1, 3, 3, 8, 3, P, None),
        lambda: lib.mmt_im2col_same(None, 1, 1, 1, 8, 1, P, None),
        lambda: lib.mmt_col2im_same(None, 1, 1, 1, 8, 1, P, None),
    ]
    for call in rejected:
        _dirty(dev)
        assert call() == -1
        assert _C.stem_last_route() == _C.STEM_ROUTE_NONE
