"""CPU: the argument checks of the image stem (csrc/stem.hip; the operand rules of
include/mmt_api.h, "image tokenizer stem"). Every combination below is rejected by the host
wrapper before any HIP call: the return value is -1 (MMT_ERR_INVALID), mmt_last_error() names the
entry point, mmt_stem_last_route() is MMT_STEM_ROUTE_NONE and nothing is launched. The pointers
are never dereferenced on these paths, so any aligned non-null value serves. Only rejected
combinations appear here: a call that passed validation would try to launch."""
import pytest

PTR = 1 << 20          # non-null, 16-B aligned
F32, U8 = 0, 2


def _i2c(lib, img=PTR, dt=U8, B=2, I=1, H=64, C=3, P=16, KH=12, KW=12, S=2, out=PTR):
    return lib.mmt_patch_im2col(img, dt, B, I, H, C, P, KH, KW, S, 1, out, None)


def _cp(lib, img=PTR, B=2, I=1, H=64, w=PTR, bias=PTR, pooled=PTR, arg=PTR):
    return lib.mmt_stem_conv_pool(img, B, I, H, w, bias, pooled, arg, None)


def _wg(lib, img=PTR, B=2, I=1, H=64, dp=PTR, arg=PTR, slab=PTR, elems=None):
    elems = 8 * 64 * 432 if elems is None else elems     # 2 images x 4 patch rows x 1 tile
    return lib.mmt_stem_conv_wgrad(img, B, I, H, dp, arg, slab, elems, None)


def _mp(lib, conv=PTR, n=8, win=9, C=64, pooled=PTR, arg=PTR):
    return lib.mmt_maxpool_patch(conv, n, win, C, pooled, arg, None)


def _mpb(lib, dp=PTR, arg=PTR, n=8, win=9, C=64, G=PTR):
    return lib.mmt_maxpool_patch_bwd(dp, arg, n, win, C, G, None)


def _gnf(lib, x=PTR, B=2, R=16, C=64, G=32, gamma=PTR, beta=PTR, y=PTR, mean=PTR, rstd=PTR):
    return lib.mmt_groupnorm_gelu_fwd(x, B, R, C, G, 1e-6, gamma, beta, y, mean, rstd, None)


def _gnb(lib, dy=PTR, x=PTR, B=2, R=16, C=64, G=32, gamma=PTR, beta=PTR, mean=PTR, rstd=PTR, dx=PTR,
         dgamma=PTR, dbeta=PTR):
    return lib.mmt_groupnorm_gelu_bwd(dy, x, B, R, C, G, gamma, beta, mean, rstd, dx, 0, dgamma,
                                      dbeta, None)


def _pos(lib, rng=PTR, B=2, I=1, H=64, P=16, Q=128, train=1, rt=PTR, ct=PTR):
    return lib.mmt_patch_positions(rng, 0, B, I, H, P, Q, train, 0, rt, ct, None)


def _p2(lib, x=PTR, n=2, OH=7, OW=5, C=16, KP=3, y=PTR, arg=PTR):
    return lib.mmt_maxpool2d(x, n, OH, OW, C, KP, y, arg, None)


def _p2b(lib, dy=PTR, arg=PTR, n=2, OH=7, OW=5, C=16, KP=3, G=PTR):
    return lib.mmt_maxpool2d_bwd(dy, arg, n, OH, OW, C, KP, G, None)


def _i2s(lib, x=PTR, n=2, H=5, W=3, C=8, KS=3, cols=PTR):
    return lib.mmt_im2col_same(x, n, H, W, C, KS, cols, None)


def _c2i(lib, dcols=PTR, n=2, H=5, W=3, C=8, KS=3, dx=PTR):
    return lib.mmt_col2im_same(dcols, n, H, W, C, KS, dx, None)


I2C, CP, WG = "mmt_patch_im2col", "mmt_stem_conv_pool", "mmt_stem_conv_wgrad"
MP, MPB = "mmt_maxpool_patch", "mmt_maxpool_patch_bwd"
GNF, GNB, POS = "mmt_groupnorm_gelu_fwd", "mmt_groupnorm_gelu_bwd", "mmt_patch_positions"
P2, P2B, I2S, C2I = "mmt_maxpool2d", "mmt_maxpool2d_bwd", "mmt_im2col_same", "mmt_col2im_same"

# rejections the wrappers already made: they must survive the tightening
KEPT = [
    ("i2c-null-img", I2C, lambda l: _i2c(l, img=None)),
    ("i2c-null-out", I2C, lambda l: _i2c(l, out=None)),
    ("i2c-B-0", I2C, lambda l: _i2c(l, B=0)),
    ("i2c-I-0", I2C, lambda l: _i2c(l, I=0)),
    ("i2c-H-0", I2C, lambda l: _i2c(l, H=0)),
    ("i2c-C-0", I2C, lambda l: _i2c(l, C=0)),
    ("i2c-P-0", I2C, lambda l: _i2c(l, P=0)),
    ("i2c-H-not-multiple-of-P", I2C, lambda l: _i2c(l, H=72)),
    ("i2c-KH-gt-P", I2C, lambda l: _i2c(l, KH=17)),
    ("i2c-KW-gt-P", I2C, lambda l: _i2c(l, KW=17)),
    ("i2c-S-0", I2C, lambda l: _i2c(l, S=0)),
    ("i2c-K-not-multiple-of-8", I2C, lambda l: _i2c(l, KH=3, KW=3)),
    ("i2c-dtype-1", I2C, lambda l: _i2c(l, dt=1)),
    ("i2c-dtype-neg", I2C, lambda l: _i2c(l, dt=-1)),
    ("cp-null-img", CP, lambda l: _cp(l, img=None)),
    ("cp-null-w", CP, lambda l: _cp(l, w=None)),
    ("cp-null-bias", CP, lambda l: _cp(l, bias=None)),
    ("cp-null-pooled", CP, lambda l: _cp(l, pooled=None)),
    ("cp-null-argmax", CP, lambda l: _cp(l, arg=None)),
    ("cp-B-0", CP, lambda l: _cp(l, B=0)),
    ("cp-I-neg", CP, lambda l: _cp(l, I=-1)),
    ("cp-H-8", CP, lambda l: _cp(l, H=8)),
    ("cp-H-40", CP, lambda l: _cp(l, H=40)),
    ("wg-null-img", WG, lambda l: _wg(l, img=None)),
    ("wg-null-dpooled", WG, lambda l: _wg(l, dp=None)),
    ("wg-null-argmax", WG, lambda l: _wg(l, arg=None)),
    ("wg-null-slab", WG, lambda l: _wg(l, slab=None)),
    ("wg-B-0", WG, lambda l: _wg(l, B=0)),
    ("wg-H-40", WG, lambda l: _wg(l, H=40)),
    ("wg-slab-too-small", WG, lambda l: _wg(l, elems=8 * 64 * 432 - 1)),
    ("mp-null-conv", MP, lambda l: _mp(l, conv=None)),
    ("mp-null-argmax", MP, lambda l: _mp(l, arg=None)),
    ("mp-npatch-0", MP, lambda l: _mp(l, n=0)),
    ("mp-win-0", MP, lambda l: _mp(l, win=0)),
    ("mp-win-256", MP, lambda l: _mp(l, win=256)),
    ("mp-C-0", MP, lambda l: _mp(l, C=0)),
    ("mpb-null-dpooled", MPB, lambda l: _mpb(l, dp=None)),
    ("mpb-null-G", MPB, lambda l: _mpb(l, G=None)),
    ("mpb-npatch-0", MPB, lambda l: _mpb(l, n=0)),
    ("mpb-win-0", MPB, lambda l: _mpb(l, win=0)),
    ("mpb-C-12", MPB, lambda l: _mpb(l, C=12)),
    ("mpb-C-0", MPB, lambda l: _mpb(l, C=0)),
    ("gnf-null-x", GNF, lambda l: _gnf(l, x=None)),
    ("gnf-null-y", GNF, lambda l: _gnf(l, y=None)),
    ("gnf-null-gamma", GNF, lambda l: _gnf(l, gamma=None)),
    ("gnf-null-mean", GNF, lambda l: _gnf(l, mean=None)),
    ("gnf-null-rstd", GNF, lambda l: _gnf(l, rstd=None)),
    ("gnf-B-0", GNF, lambda l: _gnf(l, B=0)),
    ("gnf-R-0", GNF, lambda l: _gnf(l, R=0)),
    ("gnf-C-0", GNF, lambda l: _gnf(l, C=0, G=1)),
    ("gnf-C-48", GNF, lambda l: _gnf(l, C=48, G=16)),
    ("gnf-C-512", GNF, lambda l: _gnf(l, C=512)),
    ("gnf-G-0", GNF, lambda l: _gnf(l, G=0)),
    ("gnf-G-not-dividing-C", GNF, lambda l: _gnf(l, G=24)),
    ("gnb-null-dy", GNB, lambda l: _gnb(l, dy=None)),
    ("gnb-null-dx", GNB, lambda l: _gnb(l, dx=None)),
    ("gnb-null-mean", GNB, lambda l: _gnb(l, mean=None)),
    ("gnb-null-dgamma", GNB, lambda l: _gnb(l, dgamma=None)),
    ("gnb-null-dbeta", GNB, lambda l: _gnb(l, dbeta=None)),
    ("gnb-B-0", GNB, lambda l: _gnb(l, B=0)),
    ("gnb-C-48", GNB, lambda l: _gnb(l, C=48, G=16)),
    ("gnb-G-0", GNB, lambda l: _gnb(l, G=0)),
    ("gnb-G-not-dividing-C", GNB, lambda l: _gnb(l, G=24)),
    ("pos-null-row", POS, lambda l: _pos(l, rt=None)),
    ("pos-null-col", POS, lambda l: _pos(l, ct=None)),
    ("pos-B-0", POS, lambda l: _pos(l, B=0)),
    ("pos-P-0", POS, lambda l: _pos(l, P=0)),
    ("pos-H-not-multiple-of-P", POS, lambda l: _pos(l, H=72)),
    ("pos-Q-1", POS, lambda l: _pos(l, Q=1)),
    ("pos-train-without-rng", POS, lambda l: _pos(l, rng=None)),
    ("p2-null-x", P2, lambda l: _p2(l, x=None)),
    ("p2-null-argmax", P2, lambda l: _p2(l, arg=None)),
    ("p2-npatch-0", P2, lambda l: _p2(l, n=0)),
    ("p2-C-0", P2, lambda l: _p2(l, C=0)),
    ("p2-KP-0", P2, lambda l: _p2(l, KP=0)),
    ("p2-KP-16", P2, lambda l: _p2(l, OH=20, OW=20, KP=16)),
    ("p2-OH-lt-KP", P2, lambda l: _p2(l, OH=2)),
    ("p2-OW-lt-KP", P2, lambda l: _p2(l, OW=2)),
    ("p2b-null-dy", P2B, lambda l: _p2b(l, dy=None)),
    ("p2b-null-G", P2B, lambda l: _p2b(l, G=None)),
    ("p2b-npatch-0", P2B, lambda l: _p2b(l, n=0)),
    ("p2b-KP-0", P2B, lambda l: _p2b(l, KP=0)),
    ("p2b-OH-lt-KP", P2B, lambda l: _p2b(l, OH=2)),
    ("p2b-OW-lt-KP", P2B, lambda l: _p2b(l, OW=2)),
    ("i2s-null-x", I2S, lambda l: _i2s(l, x=None)),
    ("i2s-null-cols", I2S, lambda l: _i2s(l, cols=None)),
    ("i2s-npatch-0", I2S, lambda l: _i2s(l, n=0)),
    ("i2s-H-0", I2S, lambda l: _i2s(l, H=0)),
    ("i2s-W-0", I2S, lambda l: _i2s(l, W=0)),
    ("i2s-C-12", I2S, lambda l: _i2s(l, C=12)),
    ("i2s-KS-2", I2S, lambda l: _i2s(l, KS=2)),
    ("i2s-KS-0", I2S, lambda l: _i2s(l, KS=0)),
    ("c2i-null-dcols", C2I, lambda l: _c2i(l, dcols=None)),
    ("c2i-null-dx", C2I, lambda l: _c2i(l, dx=None)),
    ("c2i-npatch-0", C2I, lambda l: _c2i(l, n=0)),
    ("c2i-W-0", C2I, lambda l: _c2i(l, W=0)),
    ("c2i-C-0", C2I, lambda l: _c2i(l, C=0)),
    ("c2i-KS-4", C2I, lambda l: _c2i(l, KS=4)),
]

# the rejections added with this file: a base pointer that a kernel moves as 16-B, 8-B or dword
# vectors and that is not aligned to that width; KH, KW <= 0; R <= 0 in the GroupNorm backward;
# a window that does not fit the byte slot in the two max-pool backwards
TIGHTENED = [
    ("i2c-KH-0", I2C, lambda l: _i2c(l, KH=0)),
    ("i2c-KW-0", I2C, lambda l: _i2c(l, KW=0)),
    ("i2c-KH-neg", I2C, lambda l: _i2c(l, KH=-12, KW=-12)),
    ("i2c-out-unaligned-8", I2C, lambda l: _i2c(l, out=PTR + 8)),
    ("i2c-out-unaligned-2", I2C, lambda l: _i2c(l, out=PTR + 2)),
    ("i2c-u8-img-unaligned-1", I2C, lambda l: _i2c(l, img=PTR + 1)),
    ("i2c-u8-img-unaligned-2", I2C, lambda l: _i2c(l, img=PTR + 2)),
    ("i2c-f32-img-unaligned-2", I2C, lambda l: _i2c(l, dt=F32, img=PTR + 2)),
    ("cp-img-unaligned-1", CP, lambda l: _cp(l, img=PTR + 1)),
    ("cp-img-unaligned-2", CP, lambda l: _cp(l, img=PTR + 2)),
    ("wg-img-unaligned-3", WG, lambda l: _wg(l, img=PTR + 3)),
    ("wg-img-unaligned-2", WG, lambda l: _wg(l, img=PTR + 2)),
    ("mpb-win-256", MPB, lambda l: _mpb(l, win=256)),
    ("mpb-dpooled-unaligned-4", MPB, lambda l: _mpb(l, dp=PTR + 4)),
    ("mpb-dpooled-unaligned-8", MPB, lambda l: _mpb(l, dp=PTR + 8)),
    ("mpb-argmax-unaligned-4", MPB, lambda l: _mpb(l, arg=PTR + 4)),
    ("mpb-argmax-unaligned-1", MPB, lambda l: _mpb(l, arg=PTR + 1)),
    ("mpb-G-unaligned-8", MPB, lambda l: _mpb(l, G=PTR + 8)),
    ("mpb-G-unaligned-2", MPB, lambda l: _mpb(l, G=PTR + 2)),
    ("gnf-x-unaligned-4", GNF, lambda l: _gnf(l, x=PTR + 4)),
    ("gnf-x-unaligned-8", GNF, lambda l: _gnf(l, x=PTR + 8)),
    ("gnf-y-unaligned-2", GNF, lambda l: _gnf(l, y=PTR + 2)),
    ("gnf-y-unaligned-4", GNF, lambda l: _gnf(l, y=PTR + 4)),
    ("gnb-R-0", GNB, lambda l: _gnb(l, R=0)),
    ("gnb-R-neg", GNB, lambda l: _gnb(l, R=-16)),
    ("gnb-dy-unaligned-4", GNB, lambda l: _gnb(l, dy=PTR + 4)),
    ("gnb-x-unaligned-8", GNB, lambda l: _gnb(l, x=PTR + 8)),
    ("gnb-dx-unaligned-12", GNB, lambda l: _gnb(l, dx=PTR + 12)),
    ("p2b-KP-16", P2B, lambda l: _p2b(l, OH=20, OW=20, KP=16)),
    ("i2s-x-unaligned-8", I2S, lambda l: _i2s(l, x=PTR + 8)),
    ("i2s-x-unaligned-2", I2S, lambda l: _i2s(l, x=PTR + 2)),
    ("i2s-cols-unaligned-8", I2S, lambda l: _i2s(l, cols=PTR + 8)),
]


def _rejected(name, call):
    from multi_modal_transformers_tokenmerge_amd import _C
    lib = _C.lib()
    # leave another entry point's message behind first, so a stale one cannot satisfy the check
    assert lib.mmt_step_advance(None, None) == -1 and b"mmt_step_advance" in lib.mmt_last_error()
    assert call(lib) == -1                       # MMT_ERR_INVALID
    msg = lib.mmt_last_error()
    assert msg and name.encode() + b":" in msg, msg
    assert _C.stem_last_route() == _C.STEM_ROUTE_NONE


@pytest.mark.parametrize("name,call", [c[1:] for c in TIGHTENED], ids=[c[0] for c in TIGHTENED])
def test_stem_entry_points_reject_tightened_arguments_without_gpu(name, call):
    """The checks added with this file: a base pointer moved as 16-B / 8-B / dword vectors that
    is not aligned to that width, KH or KW <= 0 in mmt_patch_im2col, R <= 0 in
    mmt_groupnorm_gelu_bwd, win > 255 in mmt_maxpool_patch_bwd and KP*KP > 255 in
    mmt_maxpool2d_bwd. Each returns MMT_ERR_INVALID with a message naming its entry point, and
    the route reads NONE."""
    _rejected(name, call)


@pytest.mark.parametrize("name,call", [c[1:] for c in KEPT], ids=[c[0] for c in KEPT])
def test_stem_entry_points_keep_rejecting_without_gpu(name, call):
    """Null pointers, non-positive extents, an image that is no multiple of the patch, a kernel
    larger than the patch, K % 8, a bad dtype code, C % 8, C not dividing 256, G not dividing C,
    an even KS, a pooling window larger than the map or the byte slot, a slab that is too small,
    train mode without the rng state."""
    _rejected(name, call)


def test_wgrad_slab_count_without_gpu():
    """mmt_stem_conv_wgrad_slabs: min(tiles, 512) with tiles = B*I*PPD*ceil(PPD/16), 0 for a shape
    the entry rejects; it launches nothing."""
    from multi_modal_transformers_tokenmerge_amd import _C
    lib = _C.lib()
    assert lib.mmt_stem_conv_wgrad_slabs(520, 1, 16) == 512
    assert lib.mmt_stem_conv_wgrad_slabs(6, 1, 528) == 512       # 6 * 33 * 3 = 594 tiles
    assert lib.mmt_stem_conv_wgrad_slabs(1, 2, 288) == 72        # 2 * 18 * 2
    assert lib.mmt_stem_conv_wgrad_slabs(2, 1, 40) == 0
    assert lib.mmt_stem_conv_wgrad_slabs(0, 1, 64) == 0


def test_stem_route_helper_matches_the_header_encoding():
    from multi_modal_transformers_tokenmerge_amd import _C
    assert _C.stem_route(_C.STEM_ROUTE_PATCH_IM2COL, _C.STEM_IM2COL_LDS, in_u8=True) == 1 | 2 << 8 | 0x10000
    assert _C.stem_route(_C.STEM_ROUTE_PATCH_IM2COL, _C.STEM_IM2COL_ROWS) == 1 | 1 << 8
    assert _C.stem_route(_C.STEM_ROUTE_GN_GELU_BWD, 32) == 7 | 32 << 8
    assert _C.stem_route(_C.STEM_ROUTE_GN_GELU_FWD) == 6
    assert (_C.STEM_ROUTE_CONV_POOL, _C.STEM_ROUTE_CONV_WGRAD, _C.STEM_ROUTE_MAXPOOL_PATCH,
            _C.STEM_ROUTE_MAXPOOL_PATCH_BWD, _C.STEM_ROUTE_PATCH_POSITIONS, _C.STEM_ROUTE_MAXPOOL2D,
            _C.STEM_ROUTE_MAXPOOL2D_BWD, _C.STEM_ROUTE_IM2COL_SAME, _C.STEM_ROUTE_COL2IM_SAME) == \
        (2, 3, 4, 5, 8, 9, 10, 11, 12)
