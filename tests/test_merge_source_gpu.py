"""GPU: the merge source (ToMe's merge_source as an index map), its CSR inverse and the unmerge
kernels (csrc/tome.hip: mmt_tome_pos_map, _source_step, _source_groups, _unmerge_fwd, _unmerge_bwd).

Everything integer is compared bit for bit with numpy restatements written here on top of the
canonical oracle (oracle.tome.canon_match / canon_pos_map); the unmerge forward is a gather
(bitwise), the backward a fixed-order fp32 segmented sum (bitwise against a float32 loop in the
same order). The one floating-point bar (test_value_invariant) is derived in its docstring."""
import numpy as np
import pytest
import torch

from oracle import tome as O

pytestmark = pytest.mark.gpu

N = 3
FLAG_CLASS, FLAG_DISTILL = 1, 2


def _tt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    """The raw bits of a float tensor as a numpy integer array."""
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy()
    return t.contiguous().view(torch.int32).cpu().numpy()


def _clamped_r(t, r, flags):
    """The r the reference's bipartite_soft_matching uses (token_compression.py:66-70):
    min(r, (t - protected) // 2). The class / distill cases of the (t, r) list go through it, as
    they do in the public API: the matcher and the distill layout are undefined past it."""
    prot = int(bool(flags & FLAG_CLASS)) + int(bool(flags & FLAG_DISTILL))
    return min(r, (t - prot) // 2)


def _compose(pos_maps):
    """numpy: source[b, p] = pos_L[b, ... pos_1[b, pos_0[b, p]]]."""
    src = pos_maps[0].copy()
    for pm in pos_maps[1:]:
        src = np.take_along_axis(pm, src.astype(np.int64), axis=1).astype(np.int32)
    return src


def _canon_chain(t0, rs, seed, n=N, c=8):
    """Per-layer canonical (unm, src, dst, t, r) and pos_maps of a chain over random fp32 metrics."""
    rng = np.random.default_rng(seed)
    t, idx, pms = t0, [], []
    for r in rs:
        metric = rng.standard_normal((n, t, c)).astype(np.float32)
        cu, cs, cd, _ = O.canon_match(metric, r)
        idx.append((cu, cs, cd, t, r))
        pms.append(O.canon_pos_map(cu, cs, cd, t, r))
        t -= r
    return idx, pms, t


def _halving(t0):
    rs, t = [], t0
    while t >= 2:
        rs.append(t // 2)
        t -= t // 2
    return rs


CHAINS = {7: [2, 1], 64: _halving(64), 65: [3] * 5, 256: [16] * 12, 2048: [512, 256]}
_CHAIN_CACHE = {}


def _chain(t0):
    if t0 not in _CHAIN_CACHE:
        _CHAIN_CACHE[t0] = _canon_chain(t0, CHAINS[t0], seed=1000 + t0)
    return _CHAIN_CACHE[t0]


# ----------------------------------------------------------------------------- pos_map parity
@pytest.mark.parametrize("flags", [0, FLAG_CLASS, FLAG_DISTILL, FLAG_CLASS | FLAG_DISTILL],
                         ids=["plain", "class", "distill", "both"])
@pytest.mark.parametrize("t,r", [(5, 2), (7, 1), (16, 8), (65, 3), (300, 16)])
def test_pos_map_parity(dev, t, r, flags):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    r = _clamped_r(t, r, flags)
    rng = np.random.default_rng(17 * t + r + flags)
    metric = rng.standard_normal((N, t, 8)).astype(np.float32)
    cu, cs, cd, _ = O.canon_match(metric, r, flags)
    ref = O.canon_pos_map(cu, cs, cd, t, r, flags)
    assert ref.min() >= 0 and ref.max() == t - r - 1
    du, ds, dd = _tt(cu, dev), _tt(cs, dev), _tt(cd, dev)
    pm = K.tome_pos_map(du, ds, dd, t, r, flags)
    x = torch.rand((N, t, 8), device=dev)
    _, _, pm_merge = K.tome_merge_fwd(x, 0, t, r, du, ds, dd, flags=flags)
    K.device_status()
    np.testing.assert_array_equal(_np(pm), ref)
    np.testing.assert_array_equal(_np(pm_merge), ref)
    assert pm.dtype == torch.int32 and tuple(pm.shape) == (N, t)


# ------------------------------------------------------------------------------------ chains
@pytest.mark.parametrize("t0", sorted(CHAINS))
def test_chain_equals_composition(dev, t0):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    idx, pms, tf = _chain(t0)
    source = torch.empty((N, t0), dtype=torch.int32, device=dev)
    for k, (cu, cs, cd, t, r) in enumerate(idx):
        pm = K.tome_pos_map(_tt(cu, dev), _tt(cs, dev), _tt(cd, dev), t, r)
        np.testing.assert_array_equal(_np(pm), pms[k])
        out = K.tome_source_step(pm, r, source, first=(k == 0))
        assert out is source                      # in place
    K.device_status()
    ref = _compose(pms)
    np.testing.assert_array_equal(_np(source), ref)
    assert ref.min() == 0 and ref.max() == tf - 1
    if t0 == 64:
        assert tf == 1 and not ref.any()          # 64 patches in one group


def test_public_merge_source_chain(dev):
    """merge_source(merge, source) over bipartite_soft_matching: the functional form (the given
    source is left unchanged), do_nothing, and as_matrix against ToMe's definition."""
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_compression import (
        MergeSource, bipartite_soft_matching, do_nothing, merge_source)
    g = torch.Generator().manual_seed(5)
    t, src, pms = 65, None, []
    for r in (3, 3, 3):
        metric = torch.randn((N, t, 8), generator=g)
        merge = bipartite_soft_matching(metric.to(dev), r)
        cu, cs, cd, _ = O.canon_match(metric.numpy(), r)
        pms.append(O.canon_pos_map(cu, cs, cd, t, r))
        prev = None if src is None else src.source.clone()
        new = merge_source(merge, src)
        if src is not None:
            assert torch.equal(src.source, prev) and new.source is not src.source
        src, t = new, t - r
    assert isinstance(src, MergeSource) and src.t == t == 56 and src.t0 == 65 and src.n == N
    ref = _compose(pms)
    np.testing.assert_array_equal(_np(src.source), ref)
    assert merge_source(do_nothing, src) is src
    ident = merge_source(do_nothing, None, shape=(N, 9), device=dev)
    np.testing.assert_array_equal(_np(ident.source), np.tile(np.arange(9, dtype=np.int32), (N, 1)))
    with pytest.raises(ValueError):
        merge_source(do_nothing, None)
    mat = _np(src.as_matrix())
    exp = (ref[:, None, :] == np.arange(t)[None, :, None]).astype(np.float32)
    np.testing.assert_array_equal(mat, exp)


# ------------------------------------------------------------------------------------ groups
def _groups_ref(source, tf):
    n, t0 = source.shape
    gs = np.zeros((n, tf + 1), np.int32)
    mem = np.zeros((n, t0), np.int32)
    for b in range(n):
        mem[b] = np.argsort(source[b], kind="stable")
        gs[b, 1:] = np.cumsum(np.bincount(source[b], minlength=tf))
    return gs, mem


EMPTY_GROUPS = np.array([[0, 0, 3, 3, 3, 0, 3], [1, 1, 1, 1, 1, 1, 1], [2, 0, 2, 0, 2, 0, 2]],
                        np.int32)  # t0 = 7, tf = 4: groups 1 and 2 / all but 1 / 1 and 3 empty


def _group_cases():
    yield "empty-groups", EMPTY_GROUPS, 4
    yield "one-group", np.zeros((N, 64), np.int32), 1
    yield "chain-64", _compose(_chain(64)[1]), 1
    yield "chain-65", _compose(_chain(65)[1]), 50
    yield "chain-256", _compose(_chain(256)[1]), 64
    yield "chain-2048", _compose(_chain(2048)[1]), 1280
    yield "random-2048-3", np.random.default_rng(3).integers(0, 3, (N, 2048)).astype(np.int32), 3
    yield "random-1000-999", np.random.default_rng(4).integers(0, 999, (N, 1000)).astype(np.int32), 999


@pytest.mark.parametrize("case", ["empty-groups", "one-group", "chain-64", "chain-65", "chain-256",
                                  "chain-2048", "random-2048-3", "random-1000-999"])
def test_groups_equal_stable_sort(dev, case):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_compression import MergeSource
    source, tf = next((s, t) for name, s, t in _group_cases() if name == case)
    gs_ref, mem_ref = _groups_ref(source, tf)
    d = _tt(source, dev)
    gs, mem = K.tome_source_groups(d, tf)
    gs2, mem2 = K.tome_source_groups(d, tf)       # a second launch: the same order
    K.device_status()
    np.testing.assert_array_equal(_np(gs), gs_ref)
    np.testing.assert_array_equal(_np(mem), mem_ref)
    assert torch.equal(mem, mem2) and torch.equal(gs, gs2)
    ms = MergeSource(d, tf)
    counts = ms.counts()
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (source.shape[0], tf)
    hist = np.stack([np.bincount(row, minlength=tf) for row in source]).astype(np.int32)
    np.testing.assert_array_equal(_np(counts), hist)
    assert ms.group_start is ms.group_start       # built once


# ----------------------------------------------------------------- size and value invariants
def _public_chain(dev, t0, rs, D, seed):
    """bipartite_soft_matching + merge_wavg from size=None with the source alongside. Returns
    (x0 numpy, x_final, size (n, t), MergeSource, per-layer pos_maps numpy)."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_compression import (
        bipartite_soft_matching, merge_source, merge_wavg)
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand((N, t0, D), generator=g) + 1.0          # [1, 2): positive, no cancellation
    x, size, src, pms, t = x0.to(dev), None, None, [], t0
    for r in rs:
        metric = torch.randn((N, t, 8), generator=g).to(dev)
        merge = bipartite_soft_matching(metric, r)
        x, size = merge_wavg(merge, x, size)
        src = merge_source(merge, src)
        pms.append(_np(K.tome_pos_map(merge.unm_idx, merge.src_idx, merge.dst_idx, t, r)))
        t -= r
    K.device_status()
    return x0.numpy(), x, size[..., 0], src, pms


@pytest.fixture(scope="module")
def wavg_chain(dev):
    return _public_chain(dev, 256, [16] * 12, 8, seed=21)


def test_size_invariant(wavg_chain):
    """The members of token j number exactly size[j]: the carried sizes (fp32 sums of ones,
    integers <= 2048, exact) equal the source's counts, over the whole chain."""
    _, x, size, src, pms = wavg_chain
    assert src.t == 64 and tuple(size.shape) == (N, 64) and size.dtype == torch.float32
    assert torch.equal(size, src.counts().float())
    assert int(src.counts().sum()) == N * 256
    np.testing.assert_array_equal(_np(src.source), _compose(pms))


def test_value_invariant(wavg_chain):
    """x_final[j] * size[j] against the float64 sum of the member rows of x0.

    The bar, from the merge kernel's arithmetic (tome_merge_fwd_kernel, compiled without FMA
    contraction). In one layer an output row that gathers m input rows (its primary row and
    m - 1 scattered ones) is  fl(fl(...fl(fl(x_1 s_1) + fl(x_2 s_2))... + fl(x_m s_m)) / S):
    the term that travels furthest is rounded once by its product, m - 1 times by the adds and
    once by the division, m + 1 roundings (an unmerged row: product and division, m = 1); the
    sizes s and S are exact integers. All values are positive, so the relative error of a sum is
    at most the largest relative error of its terms, and the roundings on a patch's way through
    the chain add up: k = max over patches of sum over layers of (m_layer + 1), counted below from
    the chain's own pos_maps. Each rounding is at most u = 2^-24 relative (round to nearest), so
    the bar is (1 + u)^k - 1; the final product x * size and the reference are formed in float64
    (the reference's own error, 256 float64 adds, is added: 256 * 2^-53)."""
    x0, x, size, src, pms = wavg_chain
    n, t0, _ = x0.shape
    cur = np.tile(np.arange(t0), (n, 1))
    cost = np.zeros((n, t0), np.int64)
    for pm in pms:
        m = np.stack([np.bincount(row, minlength=pm.shape[1]) for row in pm])   # rows per output
        cur = np.take_along_axis(pm.astype(np.int64), cur, axis=1)
        cost += np.take_along_axis(m, cur, axis=1) + 1
    k = int(cost.max())
    u = 2.0 ** -24
    bar = (1.0 + u) ** k - 1.0 + t0 * 2.0 ** -53
    source = _np(src.source).astype(np.int64)
    ref = np.zeros((n, src.t, x0.shape[2]), np.float64)
    for b in range(n):
        np.add.at(ref[b], source[b], x0[b].astype(np.float64))
    got = _np(x).astype(np.float64) * _np(size).astype(np.float64)[..., None]
    rel = float(np.max(np.abs(got - ref) / ref))
    print(f"value invariant: k = {k} roundings, bar = {bar:.3e}, measured max rel err = {rel:.3e}")
    assert 2 * len(pms) <= k <= sum(16 + 2 for _ in pms)
    assert rel <= bar


# --------------------------------------------------------------------------- unmerge fwd / bwd
SHAPES = [(7, 4), (65, 50), (256, 64)]
BEHIND = 4


def _seq(dev, n, L, D, dtype, seed, pad_rows=3):
    """An (n, L, D) view with a non-contiguous batch stride, and its numpy bits (float32 values)."""
    g = torch.Generator().manual_seed(seed)
    full = torch.randn((n, L + pad_rows, D), generator=g).to(dtype)
    d = full.to(dev)[:, :L]
    assert d.stride(0) == (L + pad_rows) * D and not d.is_contiguous()
    return d, full[:, :L].float().numpy()


def _fwd_ref(x, source, set_start, tf):
    t0 = source.shape[1]
    mid = np.take_along_axis(x[:, set_start:set_start + tf], source[..., None].astype(np.int64), axis=1)
    assert mid.shape[1] == t0
    return np.concatenate([x[:, :set_start], mid, x[:, set_start + tf:]], axis=1)


def _bwd_ref(g, source, set_start, tf, dtype):
    """float32 loop: every group's rows added in ascending patch order, from zero; bf16 rounded
    once through torch's CPU cast."""
    n, _, D = g.shape
    t0 = source.shape[1]
    acc = np.zeros((n, tf, D), np.float32)
    rows = np.arange(n)
    for p in range(t0):                                    # ascending patch order
        acc[rows, source[:, p]] = acc[rows, source[:, p]] + g[:, set_start + p]
    out = np.concatenate([g[:, :set_start], acc, g[:, set_start + t0:]], axis=1).astype(np.float32)
    return torch.from_numpy(out).to(dtype)


def _random_source(t0, tf, seed):
    return np.random.default_rng(seed).integers(0, tf, (N, t0)).astype(np.int32)


@pytest.mark.parametrize("t0,tf", SHAPES)
@pytest.mark.parametrize("set_start", [0, 5])
@pytest.mark.parametrize("D", [8, 40, 384])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_unmerge_fwd_is_a_gather(dev, dtype, D, set_start, t0, tf):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    L = set_start + tf + BEHIND
    x, xn = _seq(dev, N, L, D, dtype, seed=t0 + D + set_start)
    source = _random_source(t0, tf, seed=t0 * 7 + D)
    out = K.tome_unmerge_fwd(x, set_start, tf, _tt(source, dev))
    K.device_status()
    assert tuple(out.shape) == (N, L - tf + t0, D) and out.dtype == dtype
    ref = torch.from_numpy(_fwd_ref(xn, source, set_start, tf)).to(dtype)
    np.testing.assert_array_equal(_bits(out), _bits(ref))


BWD_EXTRA = [("empty-groups", EMPTY_GROUPS, 4), ("one-group", np.zeros((N, 64), np.int32), 1)]


def _check_bwd(dev, dtype, D, set_start, source, tf, seed):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_compression import (
        MergeSource, unmerge)
    t0 = source.shape[1]
    L = set_start + tf + BEHIND
    g, gn = _seq(dev, N, L - tf + t0, D, dtype, seed=seed)
    ms = MergeSource(_tt(source, dev), tf)
    gs, mem = ms.groups()
    gx = K.tome_unmerge_bwd(g, set_start, tf, gs, mem)
    gx2 = K.tome_unmerge_bwd(g, set_start, tf, gs, mem)
    K.device_status()
    assert tuple(gx.shape) == (N, L, D) and gx.dtype == dtype
    ref = _bwd_ref(gn, source, set_start, tf, dtype)
    np.testing.assert_array_equal(_bits(gx), _bits(ref))
    assert torch.equal(gx, gx2)                            # identical across two launches
    x = torch.zeros((N, L, D), dtype=dtype, device=dev, requires_grad=True)
    y = unmerge(x, ms, set_start)
    assert tuple(y.shape) == tuple(g.shape)
    y.backward(g)
    assert x.grad.dtype == dtype and torch.equal(x.grad, gx)
    return gx


@pytest.mark.parametrize("t0,tf", SHAPES)
@pytest.mark.parametrize("set_start", [0, 5])
@pytest.mark.parametrize("D", [8, 40, 384])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_unmerge_bwd_fixed_order_sum(dev, dtype, D, set_start, t0, tf):
    _check_bwd(dev, dtype, D, set_start, _random_source(t0, tf, seed=t0 * 7 + D), tf,
               seed=t0 + D + set_start + 1)


@pytest.mark.parametrize("name,source,tf", BWD_EXTRA, ids=[c[0] for c in BWD_EXTRA])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_unmerge_bwd_empty_and_single_group(dev, dtype, name, source, tf):
    gx = _check_bwd(dev, dtype, 40, 5, source, tf, seed=99)
    if name == "empty-groups":   # sample 0: groups 1 and 2 are empty -> exact zeros
        assert not _bits(gx[0, 5 + 1:5 + 3]).any()


def test_unmerge_is_the_adjoint_shape_of_merge(dev):
    """merge -> unmerge round trip through the public API: every patch row of the result is the
    merged row that stands for it."""
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_compression import (
        bipartite_soft_matching, merge_source, merge_wavg, unmerge)
    g = torch.Generator().manual_seed(8)
    x = torch.randn((N, 16, 8), generator=g).to(dev)
    merge = bipartite_soft_matching(torch.randn((N, 16, 8), generator=g).to(dev), 5)
    xm, _ = merge_wavg(merge, x)
    src = merge_source(merge)
    back = unmerge(xm, src)
    assert tuple(back.shape) == (N, 16, 8)
    ref = np.take_along_axis(_np(xm), _np(src.source)[..., None].astype(np.int64), axis=1)
    np.testing.assert_array_equal(_np(back), ref)


# ---------------------------------------------------- out-of-range maps: reported, not followed
# The bad entries (one equal to the bound, one -1) sit in sample 1 of 3 with rows behind the set,
# so even an unclamped access would stay inside the same tensor.
def _expect_fault(K):
    from multi_modal_transformers_tokenmerge_amd._C import MMTError
    with pytest.raises(MMTError):
        K.device_status()
    K.device_status()            # the word was cleared by the report


@pytest.mark.parametrize("bad_in", ["source", "pos_map"])
def test_source_step_reports_out_of_range(dev, bad_in):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    t0, t, r = 20, 12, 4
    rng = np.random.default_rng(1)
    pm = rng.integers(0, t - r, (N, t)).astype(np.int32)
    source = rng.integers(0, t, (N, t0)).astype(np.int32)
    if bad_in == "source":
        source[1, 3], source[1, 5] = t, -1
    else:
        pm[1, 2], pm[1, 4] = t - r, -1
        source[1, 0], source[1, 1] = 2, 4                  # both bad entries are looked up
    K.device_status()
    out = K.tome_source_step(_tt(pm, dev), r, _tt(source, dev))
    _expect_fault(K)
    o = _np(out)
    assert o.min() >= 0 and o.max() < t - r
    good = np.ones((N, t0), bool)
    good[1] = (source[1] >= 0) & (source[1] < t)
    exp = np.take_along_axis(pm, np.clip(source, 0, t - 1).astype(np.int64), axis=1)
    ok = good & (exp >= 0) & (exp < t - r)
    np.testing.assert_array_equal(o[ok], exp[ok])          # everything valid is still exact


def test_source_groups_reports_out_of_range(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    t0, tf = 20, 6
    source = np.random.default_rng(2).integers(0, tf, (N, t0)).astype(np.int32)
    source[1, 3], source[1, 5] = tf, -1
    K.device_status()
    gs, mem = K.tome_source_groups(_tt(source, dev), tf)
    _expect_fault(K)
    gs, mem = _np(gs), _np(mem)
    for b in range(N):
        assert sorted(mem[b].tolist()) == list(range(t0))  # still a permutation of the patches
        assert gs[b, 0] == 0 and gs[b, -1] == t0 and (np.diff(gs[b]) >= 0).all()
    gs_ref, mem_ref = _groups_ref(source[[0, 2]], tf)
    np.testing.assert_array_equal(gs[[0, 2]], gs_ref)
    np.testing.assert_array_equal(mem[[0, 2]], mem_ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_unmerge_reports_out_of_range(dev, dtype):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    t0, tf, set_start, D = 20, 6, 5, 40
    L = set_start + tf + BEHIND
    source = _random_source(t0, tf, seed=6)
    bad = source.copy()
    bad[1, 3], bad[1, 5] = tf, -1
    x, xn = _seq(dev, N, L, D, dtype, seed=12)
    K.device_status()
    out = K.tome_unmerge_fwd(x, set_start, tf, _tt(bad, dev))
    _expect_fault(K)
    assert torch.isfinite(out.float()).all()
    ref = torch.from_numpy(_fwd_ref(xn, source, set_start, tf)).to(dtype)
    keep = np.ones(t0 + set_start + BEHIND, bool)
    keep[[set_start + 3, set_start + 5]] = False
    np.testing.assert_array_equal(_bits(out)[[0, 2]], _bits(ref)[[0, 2]])
    np.testing.assert_array_equal(_bits(out)[1][keep], _bits(ref)[1][keep])
    # backward: members with an entry t0 and an entry -1
    gs, mem = K.tome_source_groups(_tt(source, dev), tf)
    K.device_status()
    memb = mem.clone()
    memb[1, 3], memb[1, 5] = t0, -1
    g, _ = _seq(dev, N, L - tf + t0, D, dtype, seed=13)
    gx = K.tome_unmerge_bwd(g, set_start, tf, gs, memb)
    _expect_fault(K)
    assert torch.isfinite(gx.float()).all()
    good = K.tome_unmerge_bwd(g, set_start, tf, gs, mem)
    K.device_status()
    assert torch.equal(gx[[0, 2]], good[[0, 2]])
    # a group_start row that is no CSR row (start past its end): an empty group, reported
    gsb = gs.clone()
    gsb[1, 2] = gsb[1, 3] + 1
    gx = K.tome_unmerge_bwd(g, set_start, tf, gsb, mem)
    _expect_fault(K)
    assert torch.isfinite(gx.float()).all() and torch.equal(gx[[0, 2]], good[[0, 2]])


def test_wrappers_reject_bad_tensors(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    src = torch.zeros((N, 8), dtype=torch.int32, device=dev)
    x = torch.zeros((N, 10, 8), device=dev)
    with pytest.raises(ValueError):
        K.tome_unmerge_fwd(x, 0, 4, src.long())                       # int64 map
    with pytest.raises(ValueError):
        K.tome_unmerge_fwd(x, 8, 4, src)                              # the set leaves the sequence
    with pytest.raises(ValueError):
        K.tome_unmerge_fwd(torch.zeros((N, 10, 12), device=dev), 0, 4, src)   # D % 8
    with pytest.raises(ValueError):
        K.tome_source_step(src[:, :6], 2, src, first=True)            # pos_map view, not contiguous
    with pytest.raises(ValueError):
        K.tome_source_step(torch.zeros((N, 6), dtype=torch.int32, device=dev), 2, src, first=True)
    with pytest.raises(ValueError):
        K.tome_source_groups(src.t().contiguous().t(), 4)             # not contiguous
    with pytest.raises(TypeError):
        K.tome_unmerge_fwd(x.half(), 0, 4, src)
