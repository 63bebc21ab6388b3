"""CPU: the argument checks of the sequence-axis LayerNorm family (csrc/norm.hip and the fused
forward of csrc/tome.hip; the operand rules of include/mmt_api.h). Every combination below is
rejected by the host wrapper before any HIP call: the return value is -1 (MMT_ERR_INVALID),
mmt_last_error() names the entry point, mmt_norm_last_route() is MMT_NORM_ROUTE_NONE and nothing is
launched. The pointers are never dereferenced on these paths, so any aligned non-null value
serves. Only rejected combinations appear here: a call that passed validation would try to launch."""
import pytest

PTR = 1 << 20          # non-null, 16-B aligned
B, L, D = 2, 40, 72
SB, ST = 48 * 80, 80   # batch and row strides of a padded operand
F32, BF16 = 0, 1


def _fwd(lib, x=PTR, dt=F32, xs=(SB, ST), B=B, L=L, D=D, gamma=PTR, beta=PTR, y=PTR, ys=(SB, ST),
         mean=PTR, rstd=PTR):
    return lib.mmt_seqnorm_fwd(x, dt, *xs, B, L, D, gamma, beta, 1e-6, y, *ys, mean, rstd, None)


def _bwd(lib, dy=PTR, ddt=BF16, ds=(SB, ST), x=PTR, xdt=F32, xs=(SB, ST), B=B, L=L, D=D, mean=PTR,
         rstd=PTR, gamma=PTR, addend=PTR, as_=(SB, ST), dx=PTR, dxs=(SB, ST), dgamma=PTR, dbeta=PTR):
    return lib.mmt_seqnorm_bwd(dy, ddt, *ds, x, xdt, *xs, B, L, D, mean, rstd, gamma, addend, *as_,
                               dx, *dxs, dgamma, dbeta, None)


def _dbwd(lib, dy=PTR, ds=(SB, ST), x=PTR, xs=(SB, ST), B=B, L=L, D=D, mean=PTR, gamma=PTR,
          addend=PTR, as_=(SB, ST), dx=PTR, dxs=(SB, ST), dgamma=PTR, rng=PTR, keep=0.9, z=PTR,
          zs=(SB, ST)):
    return lib.mmt_seqnorm_dropout_bwd(dy, *ds, x, *xs, B, L, D, mean, PTR, gamma, addend, *as_, dx,
                                       *dxs, dgamma, PTR, rng, 1, 3, keep, 0, z, *zs, PTR, None)


def _unm(lib, dy=PTR, ds=(SB, ST), x=PTR, xs=(SB, ST), B=B, L2=L, D=D, mean=PTR, addend=PTR,
         as_=(SB, ST), dgamma=PTR, L=L + 4, s0=4, t=32, r=4, pos=PTR, g_in=PTR, gs=(SB, ST), rng=PTR,
         keep=0.9, z=PTR, zs=(SB, ST)):
    return lib.mmt_ln_unmerge_dropout_bwd(dy, *ds, x, *xs, B, L2, D, mean, PTR, PTR, addend, *as_,
                                          dgamma, PTR, L, s0, t, r, PTR, PTR, pos, g_in, *gs, rng,
                                          1, 1, keep, 0, z, *zs, PTR, None)


def _mrg(lib, x=PTR, n=B, L=L + 4, D=D, xs=(SB, ST), s0=4, t=32, r=4, src=PTR, out=PTR, os_=(SB, ST),
         gamma=PTR, y=PTR, ys=(SB, ST), mean=PTR):
    return lib.mmt_tome_merge_seqnorm_fwd(x, n, L, D, *xs, s0, t, r, 0, None, PTR, src, PTR, out,
                                          *os_, PTR, PTR, gamma, PTR, 1e-6, y, *ys, mean, PTR, None)


FWD, BWD, DBWD = "mmt_seqnorm_fwd", "mmt_seqnorm_bwd", "mmt_seqnorm_dropout_bwd"
UNM, MRG = "mmt_ln_unmerge_dropout_bwd", "mmt_tome_merge_seqnorm_fwd"

# rejections the wrappers already made: they must survive the tightening
KEPT = [
    ("fwd-null-x", FWD, lambda l: _fwd(l, x=None)),
    ("fwd-null-y", FWD, lambda l: _fwd(l, y=None)),
    ("fwd-null-gamma", FWD, lambda l: _fwd(l, gamma=None)),
    ("fwd-null-mean", FWD, lambda l: _fwd(l, mean=None)),
    ("fwd-dtype-2", FWD, lambda l: _fwd(l, dt=2)),
    ("fwd-dtype-neg", FWD, lambda l: _fwd(l, dt=-1)),
    ("fwd-D-12", FWD, lambda l: _fwd(l, D=12)),
    ("fwd-D-0", FWD, lambda l: _fwd(l, D=0)),
    ("fwd-D-neg", FWD, lambda l: _fwd(l, D=-8)),
    ("fwd-L-0", FWD, lambda l: _fwd(l, L=0)),
    ("fwd-B-0", FWD, lambda l: _fwd(l, B=0)),
    ("fwd-xs_t-76", FWD, lambda l: _fwd(l, xs=(SB, 76))),
    ("fwd-ys_t-76", FWD, lambda l: _fwd(l, ys=(SB, 76))),
    ("fwd-xs_b-4", FWD, lambda l: _fwd(l, xs=(SB + 4, ST))),
    ("fwd-ys_b-4", FWD, lambda l: _fwd(l, ys=(SB + 4, ST))),
    ("bwd-null-dy", BWD, lambda l: _bwd(l, dy=None)),
    ("bwd-null-dx", BWD, lambda l: _bwd(l, dx=None)),
    ("bwd-null-dgamma", BWD, lambda l: _bwd(l, dgamma=None)),
    ("bwd-null-dbeta", BWD, lambda l: _bwd(l, dbeta=None)),
    ("bwd-dy-dtype-2", BWD, lambda l: _bwd(l, ddt=2)),
    ("bwd-x-dtype-2", BWD, lambda l: _bwd(l, xdt=2)),
    ("bwd-D-12", BWD, lambda l: _bwd(l, D=12)),
    ("bwd-D-0", BWD, lambda l: _bwd(l, D=0)),
    ("bwd-L-neg", BWD, lambda l: _bwd(l, L=-1)),
    ("bwd-B-0", BWD, lambda l: _bwd(l, B=0)),
    ("bwd-ds_t-76", BWD, lambda l: _bwd(l, ds=(SB, 76))),
    ("bwd-xs_t-76", BWD, lambda l: _bwd(l, xs=(SB, 76))),
    ("bwd-as_t-76", BWD, lambda l: _bwd(l, as_=(SB, 76))),
    ("bwd-dxs_t-76", BWD, lambda l: _bwd(l, dxs=(SB, 76))),
    ("dbwd-null-x", DBWD, lambda l: _dbwd(l, x=None)),
    ("dbwd-null-z", DBWD, lambda l: _dbwd(l, z=None)),
    ("dbwd-D-12", DBWD, lambda l: _dbwd(l, D=12)),
    ("dbwd-L-0", DBWD, lambda l: _dbwd(l, L=0)),
    ("dbwd-B-neg", DBWD, lambda l: _dbwd(l, B=-2)),
    ("dbwd-zs_t-76", DBWD, lambda l: _dbwd(l, zs=(SB, 76))),
    ("dbwd-ds_t-76", DBWD, lambda l: _dbwd(l, ds=(SB, 76))),
    ("dbwd-keep-0", DBWD, lambda l: _dbwd(l, keep=0.0)),
    ("dbwd-keep-neg", DBWD, lambda l: _dbwd(l, keep=-0.5)),
    ("dbwd-keep-gt-1", DBWD, lambda l: _dbwd(l, keep=1.5)),
    ("unm-null-pos_map", UNM, lambda l: _unm(l, pos=None)),
    ("unm-null-g_in", UNM, lambda l: _unm(l, g_in=None)),
    ("unm-null-mean", UNM, lambda l: _unm(l, mean=None)),
    ("unm-D-12", UNM, lambda l: _unm(l, D=12)),
    ("unm-D-0", UNM, lambda l: _unm(l, D=0)),
    ("unm-B-0", UNM, lambda l: _unm(l, B=0)),
    ("unm-L2-0", UNM, lambda l: _unm(l, L2=0, L=4)),
    ("unm-L-ne-L2-plus-r", UNM, lambda l: _unm(l, L=L + 5)),
    ("unm-L-513", UNM, lambda l: _unm(l, L2=383, L=513, r=130, t=400, s0=0)),
    ("unm-L2-385", UNM, lambda l: _unm(l, L2=385, L=389)),
    ("unm-gs_t-76", UNM, lambda l: _unm(l, gs=(SB, 76))),
    ("unm-zs_t-76", UNM, lambda l: _unm(l, zs=(SB, 76))),
    ("unm-keep-0", UNM, lambda l: _unm(l, keep=0.0)),
    ("unm-keep-gt-1", UNM, lambda l: _unm(l, keep=1.25)),
    ("mrg-null-x", MRG, lambda l: _mrg(l, x=None)),
    ("mrg-null-src", MRG, lambda l: _mrg(l, src=None)),
    ("mrg-null-gamma", MRG, lambda l: _mrg(l, gamma=None)),
    ("mrg-null-mean", MRG, lambda l: _mrg(l, mean=None)),
    ("mrg-D-12", MRG, lambda l: _mrg(l, D=12)),
    ("mrg-D-0", MRG, lambda l: _mrg(l, D=0)),
    ("mrg-n-0", MRG, lambda l: _mrg(l, n=0)),
    ("mrg-L-minus-r-513", MRG, lambda l: _mrg(l, L=517, t=500)),
    ("mrg-xs_t-76", MRG, lambda l: _mrg(l, xs=(SB, 76))),
    ("mrg-os_n-4", MRG, lambda l: _mrg(l, os_=(SB + 4, ST))),
    ("mrg-ys_t-76", MRG, lambda l: _mrg(l, ys=(SB, 76))),
]

# the rejections added with this file: batch strides % 8 in the three backward entries, a row
# stride smaller than D, a base pointer of a 16-B-vector operand that is not 16-B aligned
TIGHTENED = [
    ("bwd-ds_b-4", BWD, lambda l: _bwd(l, ds=(SB + 4, ST))),
    ("bwd-xs_b-4", BWD, lambda l: _bwd(l, xs=(SB + 4, ST))),
    ("bwd-as_b-4", BWD, lambda l: _bwd(l, as_=(SB + 4, ST))),
    ("bwd-dxs_b-4", BWD, lambda l: _bwd(l, dxs=(SB + 4, ST))),
    ("dbwd-ds_b-4", DBWD, lambda l: _dbwd(l, ds=(SB + 4, ST))),
    ("dbwd-xs_b-4", DBWD, lambda l: _dbwd(l, xs=(SB + 4, ST))),
    ("dbwd-as_b-4", DBWD, lambda l: _dbwd(l, as_=(SB + 4, ST))),
    ("dbwd-dxs_b-4", DBWD, lambda l: _dbwd(l, dxs=(SB + 4, ST))),
    ("dbwd-zs_b-4", DBWD, lambda l: _dbwd(l, zs=(SB + 4, ST))),
    ("unm-ds_b-4", UNM, lambda l: _unm(l, ds=(SB + 4, ST))),
    ("unm-xs_b-4", UNM, lambda l: _unm(l, xs=(SB + 4, ST))),
    ("unm-as_b-4", UNM, lambda l: _unm(l, as_=(SB + 4, ST))),
    ("unm-gs_b-4", UNM, lambda l: _unm(l, gs=(SB + 4, ST))),
    ("unm-zs_b-4", UNM, lambda l: _unm(l, zs=(SB + 4, ST))),
    ("fwd-xs_t-lt-D", FWD, lambda l: _fwd(l, xs=(SB, D - 8))),
    ("fwd-ys_t-lt-D", FWD, lambda l: _fwd(l, ys=(SB, D - 8))),
    ("fwd-xs_t-0", FWD, lambda l: _fwd(l, xs=(SB, 0))),
    ("bwd-ds_t-lt-D", BWD, lambda l: _bwd(l, ds=(SB, D - 8))),
    ("bwd-xs_t-lt-D", BWD, lambda l: _bwd(l, xs=(SB, D - 8))),
    ("bwd-as_t-lt-D", BWD, lambda l: _bwd(l, as_=(SB, D - 8))),
    ("bwd-dxs_t-lt-D", BWD, lambda l: _bwd(l, dxs=(SB, D - 8))),
    ("dbwd-xs_t-lt-D", DBWD, lambda l: _dbwd(l, xs=(SB, D - 8))),
    ("dbwd-dxs_t-neg", DBWD, lambda l: _dbwd(l, dxs=(SB, -ST))),
    ("dbwd-zs_t-lt-D", DBWD, lambda l: _dbwd(l, zs=(SB, D - 8))),
    ("unm-ds_t-lt-D", UNM, lambda l: _unm(l, ds=(SB, D - 8))),
    ("unm-gs_t-lt-D", UNM, lambda l: _unm(l, gs=(SB, D - 8))),
    ("unm-zs_t-0", UNM, lambda l: _unm(l, zs=(SB, 0))),
    ("mrg-xs_t-lt-D", MRG, lambda l: _mrg(l, xs=(SB, D - 8))),
    ("mrg-os_t-lt-D", MRG, lambda l: _mrg(l, os_=(SB, D - 8))),
    ("mrg-ys_t-lt-D", MRG, lambda l: _mrg(l, ys=(SB, D - 8))),
    ("fwd-x-unaligned", FWD, lambda l: _fwd(l, x=PTR + 8)),
    ("fwd-y-unaligned", FWD, lambda l: _fwd(l, y=PTR + 2)),
    ("bwd-dy-unaligned", BWD, lambda l: _bwd(l, dy=PTR + 4)),
    ("bwd-x-unaligned", BWD, lambda l: _bwd(l, x=PTR + 8)),
    ("bwd-addend-unaligned", BWD, lambda l: _bwd(l, addend=PTR + 4)),
    ("bwd-dx-unaligned", BWD, lambda l: _bwd(l, dx=PTR + 12)),
    ("dbwd-dy-unaligned", DBWD, lambda l: _dbwd(l, dy=PTR + 2)),
    ("dbwd-addend-unaligned", DBWD, lambda l: _dbwd(l, addend=PTR + 8)),
    ("dbwd-dx-unaligned", DBWD, lambda l: _dbwd(l, dx=PTR + 4)),
    ("dbwd-z-unaligned", DBWD, lambda l: _dbwd(l, z=PTR + 8)),
    ("unm-dy-unaligned", UNM, lambda l: _unm(l, dy=PTR + 8)),
    ("unm-x-unaligned", UNM, lambda l: _unm(l, x=PTR + 4)),
    ("unm-addend-unaligned", UNM, lambda l: _unm(l, addend=PTR + 8)),
    ("unm-g_in-unaligned", UNM, lambda l: _unm(l, g_in=PTR + 4)),
    ("unm-z-unaligned", UNM, lambda l: _unm(l, z=PTR + 2)),
    ("mrg-x-unaligned", MRG, lambda l: _mrg(l, x=PTR + 4)),
    ("mrg-x_out-unaligned", MRG, lambda l: _mrg(l, out=PTR + 8)),
    ("mrg-y-unaligned", MRG, lambda l: _mrg(l, y=PTR + 2)),
]


def _rejected(name, call):
    from multi_modal_transformers_tokenmerge_amd import _C
    lib = _C.lib()
    # leave another entry point's message behind first, so a stale one cannot satisfy the check
    assert lib.mmt_step_advance(None, None) == -1 and b"mmt_step_advance" in lib.mmt_last_error()
    assert call(lib) == -1                       # MMT_ERR_INVALID
    msg = lib.mmt_last_error()
    assert msg and name.encode() + b":" in msg, msg
    assert _C.norm_last_route() == _C.NORM_ROUTE_NONE


@pytest.mark.parametrize("name,call", [c[1:] for c in TIGHTENED], ids=[c[0] for c in TIGHTENED])
def test_norm_entry_points_reject_tightened_arguments_without_gpu(name, call):
    """The checks added with this file: a batch stride of a backward entry that is no multiple of
    8, a row stride below D (zero and negative ones with it), and a base pointer of a 16-B-vector
    operand that is not 16-B aligned. Each returns MMT_ERR_INVALID with a message naming its
    entry point, and the route reads NONE."""
    _rejected(name, call)


@pytest.mark.parametrize("name,call", [c[1:] for c in KEPT], ids=[c[0] for c in KEPT])
def test_norm_entry_points_keep_rejecting_without_gpu(name, call):
    """Null pointers, D % 8, row strides % 8, B / L / D <= 0, a bad dtype code, keep_prob outside
    (0, 1], and for the fused entries L != L2 + r, L > 512, L2 > 384 and L - r > 512."""
    _rejected(name, call)


def test_norm_route_helper_matches_the_header_encoding():
    from multi_modal_transformers_tokenmerge_amd import _C
    assert _C.norm_route(_C.NORM_ROUTE_SEQ_BWD, 10, dy_bf16=True) == 2 | 10 << 8 | 0x20000
    assert _C.norm_route(_C.NORM_ROUTE_SEQ_FWD, 0, x_bf16=True) == 1 | 0x10000
    assert (_C.NORM_ROUTE_SEQ_DROPOUT_BWD, _C.NORM_ROUTE_LN_UNMERGE_BWD,
            _C.NORM_ROUTE_MERGE_SEQ_FWD) == (3, 4, 5)
