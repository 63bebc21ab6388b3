"""CPU: the C oracle's tie and NaN rules on exactly the inputs of tests/test_tome_contract_gpu.py,
pinned without its C rank and argmax code, and the Python statement of the mmt_tome_match dispatch
(tests/tome_ref.expected_route) at the boundary shapes.

On tests/tome_ref.tie_metric data the oracle's src and unm must be
np.argsort(node_max, kind="stable")[::-1] (numpy sorts NaN last, so it comes first after the
reversal, ties with the higher index first: the kernels' sort_key order) and its dst the
first-index argmax of float64 scores, NaN first. check_tie_properties asserts that the data still
ties: a shape whose data stopped tying fails here."""
import numpy as np
import pytest

from oracle import tome as O
from tests import tome_ref as R

# (n, t, heads, c, r, flags): the tie_metric shapes of the GPU contract tests
TIE_SHAPES = [(2, 512, 1, 64, 32, 0), (2, 513, 1, 64, 32, 0), (2, 514, 1, 64, 32, 0),
              (2, 1153, 1, 64, 32, 0), (2, 1154, 1, 64, 32, 0), (29, 514, 1, 64, 32, 0),
              (3, 130, 1, 24, 16, 0), (3, 64, 3, 40, 16, 0), (3, 258, 1, 96, 16, 0),
              (3, 64, 1, 512, 16, 0), (3, 130, 1, 512, 16, 0), (3, 300, 2, 256, 16, 0),
              (3, 300, 1, 12, 16, 0), (3, 301, 1, 7, 16, 0), (3, 31, 1, 6, 12, 0),
              (3, 512, 1, 64, 32, 0), (3, 1024, 1, 64, 32, 0), (3, 1000, 1, 64, 50, 3),
              (2, 2048, 1, 64, 64, 0), (2, 2048, 1, 64, 64, 1), (2, 512, 1, 64, 256, 0)]


@pytest.mark.parametrize("n,t,heads,c,r,flags", TIE_SHAPES)
def test_oracle_tie_rule_is_numpys(n, t, heads, c, r, flags):
    m = R.tie_metric(n, t, heads, c)
    unm, src, dst, nmax = O.canon_match(m, r, flags)
    R.check_tie_properties(nmax, dst, r)
    for s in range(n):
        order = np.argsort(nmax[s], kind="stable")[::-1]
        np.testing.assert_array_equal(src[s], order[:r])
        np.testing.assert_array_equal(unm[s], order[r:])
        assert sorted(np.concatenate([src[s], unm[s]]).tolist()) == list(range((t + 1) // 2))
    if flags == 0:  # (the protected-token flags overwrite scores: the oracle's own tests)
        arg = R.f64_first_argmax(m)
        np.testing.assert_array_equal(dst, np.take_along_axis(arg, src.astype(np.int64), axis=1))


def test_tie_metric_is_bf16_exact_and_holds_the_zero_rows():
    import torch
    m = R.tie_metric(3, 64, 3, 40)
    assert torch.equal(torch.from_numpy(m).bfloat16().float(), torch.from_numpy(m))
    tok = m.sum(2)
    zero = (tok == 0).all(-1)
    assert zero[0].sum() == 0 and zero[1].sum() == 1 and zero[2].sum() == 1
    assert np.flatnonzero(zero[1])[0] % 2 == 0 and np.flatnonzero(zero[2])[0] % 2 == 1
    assert len(np.unique(tok[0], axis=0)) <= 6
    assert all((m[0, :, h] != 0).any() for h in range(3)), "a head that holds nothing"


def test_sort_key_order():
    v = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf], np.float32)
    k = R.sort_key(v)
    assert (np.diff(k.astype(np.int64)) < 0).all()


def test_expected_route_boundaries_c64():
    """The boundaries the forms have at c = 64, from scanning the helper: fused to t = 513, the
    b-resident score kernel to 1153 (two a tiles per workgroup to 1089), tiled beyond."""
    assert R.form_boundaries(64) == (513, 1153, 1089)
    f = lambda n, t, **kw: R.expected_route(n, t, 64, "float32", **kw)
    vec8 = 8 << 8
    assert f(2, 512) == f(2, 513) == R.FUSED | vec8
    assert f(2, 514) == f(2, 1153) == R.BIG_AG1 | vec8
    assert f(2, 1154) == R.TILED_MFMA | vec8 | 4 << 20
    assert f(29, 514) == R.BIG_AG2 | vec8 and f(28, 514) == R.BIG_AG1 | vec8
    assert f(29, 1089) == R.BIG_AG2 | vec8 and f(29, 1090) == R.BIG_AG1 | vec8
    assert f(2, 512, use_mfma=False) == R.TILED_VALU | vec8 | 4 << 20
    assert R.expected_route(2, 512, 64, "bfloat16") == R.FUSED | vec8 | R.IN_BF16


def test_expected_route_lane_layouts_and_views():
    e = R.expected_route
    assert e(3, 130, 24, "float32") == R.FUSED | 4 << 8
    assert e(3, 64, 40, "float32", (64 * 120, 120, 40)) == R.FUSED | 8 << 8
    assert e(3, 258, 96, "float32") == R.FUSED | 16 << 8
    assert e(3, 64, 512, "float32") == R.FUSED | 64 << 8
    assert e(3, 130, 512, "float32") == R.TILED_MFMA | 64 << 8 | 1 << 20
    assert e(3, 300, 256, "float32", (300 * 512, 512, 256)) == R.TILED_MFMA | 32 << 8 | 3 << 20
    assert e(3, 300, 12, "float32") == R.BIG_AG1 | R.NORM_SCALAR
    assert e(3, 301, 7, "float32") == R.TILED_VALU | R.NORM_SCALAR | 4 << 20
    assert e(3, 31, 6, "float32") == R.TILED_MFMA | R.NORM_SCALAR | 4 << 20
    assert e(3, 31, 6, "float32", use_mfma=False) == R.TILED_VALU | R.NORM_SCALAR | 4 << 20
    # a base or stride that is no multiple of 16 B: the scalar norm, the same score form
    assert e(2, 66, 64, "float32", base_align=4) == R.BIG_AG1 | R.NORM_SCALAR
    assert e(2, 66, 64, "float32", (66 * 66, 66, 0)) == R.BIG_AG1 | R.NORM_SCALAR
    assert e(2, 66, 64, "bfloat16", (66 * 68, 68, 0)) == R.BIG_AG1 | R.NORM_SCALAR | R.IN_BF16
    assert e(2, 66, 64, "float32", (66 * 68, 68, 0)) == R.FUSED | 8 << 8


def test_route_constants_match_the_binding():
    from multi_modal_transformers_tokenmerge_amd import _C
    assert (R.FUSED, R.BIG_AG1, R.BIG_AG2, R.TILED_MFMA, R.TILED_VALU) == (
        _C.TOME_ROUTE_FUSED, _C.TOME_ROUTE_BIG_AG1, _C.TOME_ROUTE_BIG_AG2,
        _C.TOME_ROUTE_TILED_MFMA, _C.TOME_ROUTE_TILED_VALU)
    assert (R.NORM_SCALAR, R.IN_BF16) == (_C.TOME_ROUTE_NORM_SCALAR, _C.TOME_ROUTE_IN_BF16)
    assert _C.tome_route(_C.TOME_ROUTE_TILED_MFMA, 8, 4, True) == R.expected_route(
        2, 1154, 64, "bfloat16")
    assert _C.tome_route(_C.TOME_ROUTE_BIG_AG1) == R.expected_route(3, 300, 12, "float32")
    # a refusal before any launch (no GPU needed: the arguments are checked first)
    assert _C.lib().mmt_tome_match(None, 0, 1, 8, 1, 4, 32, 4, 0, 2, 0, None, None, None, None,
                                   None, 0, None) == -1
    assert _C.tome_last_route() == _C.TOME_ROUTE_NONE
