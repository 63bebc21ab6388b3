"""GPU: the point-cloud kernels (csrc/pointcloud.hip: mmt_pc_sample_group, mmt_pc_embed_fwd /
_bwd) against the numpy restatement tests/pointcloud_ref.py, and the sequence assembly's early-out
for the rows they own (kind 4).

Indices are demanded exactly: the distance is individually rounded fp32 on both sides. The
embedding is compared with the float64 restatement under the bound derived in pointcloud_ref.py,
|got - ref64| <= 4 (N + 2) 2^-24 A with A the propagated sum of magnitudes per element and N the
longest sum along the chain (pointcloud_ref.chain_lengths); every test prints its worst
err / bound per tensor before it asserts. Figures measured on an MI355X: DESIGN.md §3 "Point-cloud
tokens"."""
import numpy as np
import pytest
import torch

from tests import pointcloud_ref as R

pytestmark = pytest.mark.gpu

#          B  S  P     C  n    k
SHAPES = [(1, 1, 8, 3, 4, 3),          # the smallest case
          (2, 1, 64, 3, 8, 4),         # one wave
          (3, 2, 257, 6, 33, 16),      # a tail past four waves, extra features
          (2, 1, 1000, 3, 64, 32),     # non-power-of-two P, the largest k
          (1, 1, 4096, 8, 256, 32)]    # every limit at once
SENTINEL = -12345.5
_REF = {}


def _K():
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    return K


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cloud(shape):
    B, S, P, C, n, k = shape
    return np.random.default_rng([B, S, P, C]).standard_normal((B, S, P, C)).astype(np.float32)


def _ref(shape, mode):
    """The restatement's indices of a shape and start mode, computed once for the file."""
    key = (shape, mode)
    if key not in _REF:
        B, S, P, C, n, k = shape
        pts = _cloud(shape)
        start = None
        if mode == "injected":
            start = np.random.default_rng(P).integers(0, P, (B, S)).astype(np.int32)
            start[0, 0] = P - 1
        elif mode == "drawn":
            start = R.drawn_start(11, 5, B, S, P, sample_offset=3)
        _REF[key] = (pts, start, *R.sample_group(pts, n, k, start))
    return _REF[key]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("mode", ["eval", "injected", "drawn"])
def test_indices_equal_the_restatement(dev, shape, mode):
    K = _K()
    B, S, P, C, n, k = shape
    pts, start, cref, nref = _ref(shape, mode)
    kw = {}
    if mode == "injected":
        kw = dict(start=_t(start, dev))
    elif mode == "drawn":
        kw = dict(rng=torch.tensor([11, 5], dtype=torch.int32, device=dev), sample_offset=3)
    cidx, nidx = K.pc_sample_group(_t(pts, dev), n, k, **kw)
    # the same clouds as a view with a padded batch stride
    buf = torch.full((B, S * P * C + 7), SENTINEL, device=dev)
    view = buf[:, :S * P * C].view(B, S, P, C)
    view.copy_(_t(pts, dev))
    cidx2, nidx2 = K.pc_sample_group(view, n, k, **kw)
    torch.cuda.synchronize()
    assert cidx.dtype == torch.int32 and tuple(cidx.shape) == (B, S, n)
    assert nidx.dtype == torch.int32 and tuple(nidx.shape) == (B, S, n, k)
    if start is not None:
        np.testing.assert_array_equal(cidx[:, :, 0].cpu().numpy(), start)
    np.testing.assert_array_equal(cidx.cpu().numpy(), cref)
    np.testing.assert_array_equal(nidx.cpu().numpy(), nref)
    assert torch.equal(cidx, cidx2) and torch.equal(nidx, nidx2)
    K.device_status()


def test_known_answer_clouds(dev):
    from multi_modal_transformers_tokenmerge_amd.tokenizers.pointclouds.point_cloud_tokenizer \
        import PointCloudTokenizer
    K = _K()
    tok = PointCloudTokenizer(num_neighbours_knn=3)
    c, nb = tok.sample_and_group(_t(R.line_cloud(), dev), 4, 0)
    assert c.tolist() == [0, 7, 3, 5]
    assert nb.tolist() == [[0, 1, 2], [7, 6, 5], [3, 2, 4], [5, 4, 6]]
    ones = torch.ones((10, 3), device=dev)
    c, nb = tok.sample_and_group(ones, 5, 2)
    assert c.tolist() == [2, 0, 1, 3, 4] and nb.tolist() == [[0, 1, 2]] * 5
    assert tok.farthest_point_sampling(ones, 5, 2).tolist() == [2, 0, 1, 3, 4]
    lat = _t(R.lattice_cloud(), dev)
    assert tok.farthest_point_sampling(lat, 10, 62).tolist() == \
        [62, 0, 4, 20, 24, 100, 104, 120, 124, 7]
    assert tok.knn(lat, 62, 7).tolist() == [62, 37, 57, 61, 63, 67, 87]
    assert tok.knn(lat, 62).tolist() == [62, 37, 57]
    K.device_status()


@pytest.mark.parametrize("P,n,k", [(64, 16, 8), (600, 40, 32)])
def test_duplicated_points_break_ties_by_index(dev, P, n, k):
    """Every point twice (shuffled): each distance occurs at least twice, so sampling and grouping
    are decided by the index rule throughout."""
    K = _K()
    rng = np.random.default_rng(P)
    half = rng.standard_normal((2, 1, P // 2, 3)).astype(np.float32)
    pts = np.concatenate([half, half], axis=2)[:, :, rng.permutation(P)]
    cref, nref = R.sample_group(pts, n, k)
    cidx, nidx = K.pc_sample_group(_t(pts, dev), n, k)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cidx.cpu().numpy(), cref)
    np.testing.assert_array_equal(nidx.cpu().numpy(), nref)
    K.device_status()


def test_non_finite_clouds_stay_in_bounds(dev):
    K = _K()
    P = 300
    pts = np.random.default_rng(2).standard_normal((3, 1, P, 4)).astype(np.float32)
    pts[0, 0, ::7, 0] = np.nan
    pts[0, 0, 5] = np.inf
    pts[1, 0, ::3, 2] = -np.inf
    pts[1, 0, 1::3, 1] = np.inf
    pts[2] = np.nan
    cidx, nidx = K.pc_sample_group(_t(pts, dev), 40, 16)
    torch.cuda.synchronize()
    for a in (cidx, nidx):
        assert int(a.min()) >= 0 and int(a.max()) < P
    K.device_status()


# ---------------------------------------------------------------------------- embedding
def _rows(S, n, L0):
    rows = np.array([2 + j + 3 * (j // 2) for j in range(S * n)], np.int32)
    assert rows[-1] < L0
    return rows


def _report(what, got, ref, bnd):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / (bnd + 1e-300)).max())
    print(f"{what}: worst err / bound = {ratio:.4f} (max err {err.max():.3e})")
    return ratio


def _fwd_on_gpu(dev, c, pad=0):
    K = _K()
    B, S, n, k, F1, F2, D = c["shape"]
    pts = _t(c["points"], dev)
    cidx, nidx = K.pc_sample_group(pts, n, k)
    L0 = 2 + S * n + 3 * ((S * n) // 2) + 3
    rows = _rows(S, n, L0)
    pe = np.random.default_rng(1).standard_normal((L0, D)).astype(np.float32)
    buf = torch.full((B, L0 + pad, D), SENTINEL, device=dev)
    x0 = buf[:, :L0]
    w = {key: _t(v, dev) for key, v in c["params"].items()}
    argmax = K.pc_embed_fwd(pts, cidx, nidx, w["w1"], w["b1"], w["w2"], w["b2"], w["w_out"],
                            w["b_out"], _t(pe, dev), _t(rows, dev), x0)
    torch.cuda.synchronize()
    return dict(pts=pts, cidx=cidx, nidx=nidx, rows=rows, pe=pe, buf=buf, w=w, argmax=argmax, L0=L0)


@pytest.mark.parametrize("name", sorted(R.BWD_CASES))
def test_forward_rows_and_nothing_else(dev, name):
    K = _K()
    c = R.bwd_case(name)
    B, S, n, k, F1, F2, D = c["shape"]
    g = _fwd_on_gpu(dev, c, pad=2)
    np.testing.assert_array_equal(g["cidx"].cpu().numpy(), c["cidx"])
    np.testing.assert_array_equal(g["nidx"].cpu().numpy(), c["nidx"])
    feat = R.features(c["points"], g["cidx"].cpu().numpy(), g["nidx"].cpu().numpy())
    fw = R.embed_fwd(feat, c["params"])
    N = R.chain_lengths(B * S * n, k, c["C"], F1, F2, D)
    rows, pe = g["rows"], g["pe"].astype(np.float64)
    got = g["buf"].cpu().numpy()
    want = fw["out"].reshape(B, S * n, D) + pe[rows]
    bnd = R.bound(N["out"], fw["Aout"].reshape(B, S * n, D) + np.abs(pe[rows]))
    assert _report("x0 rows", got[:, rows], want, bnd) <= 1.0
    other = np.ones(got.shape[1], bool)
    other[rows] = False
    assert (got[:, other] == np.float32(SENTINEL)).all()          # no other row touched
    # the saved arg-max attains the restatement's maximum within the bound of z2
    am = g["argmax"].cpu().numpy().astype(np.int64)
    assert am.shape == (B, S, n, F2) and am.max() < k
    at = np.take_along_axis(fw["h2"], am[..., None, :], axis=-2)[..., 0, :]
    assert ((fw["h2"].max(-2) - at) <= R.bound(N["z2"], fw["Ag"])).all()
    K.device_status()


def _bwd_on_gpu(dev, c, g, dx0, grads=None):
    K = _K()
    w = g["w"]
    if grads is None:
        grads = tuple(torch.zeros_like(w[key]) for key in
                      ("w1", "b1", "w2", "b2", "w_out", "b_out"))
    K.pc_embed_bwd(dx0, _t(g["rows"], dev), g["pts"], g["cidx"], g["nidx"], g["argmax"], w["w1"],
                   w["b1"], w["w2"], w["b2"], w["w_out"], grads)
    torch.cuda.synchronize()
    return dict(zip(("w1", "b1", "w2", "b2", "w_out", "b_out"), grads))


def _check_grads(c, g, got, dy, what):
    B, S, n, k, F1, F2, D = c["shape"]
    feat = R.features(c["points"], g["cidx"].cpu().numpy(), g["nidx"].cpu().numpy())
    am = g["argmax"].cpu().numpy().astype(np.int64)
    ref, mag = R.embed_bwd(feat, c["params"], dy, am)
    N = R.chain_lengths(B * S * n, k, c["C"], F1, F2, D)
    worst = {key: _report(f"{what} d{key}", got[key].cpu().numpy(), ref[key],
                          R.bound(N[key], mag[key])) for key in ref}
    assert max(worst.values()) <= 1.0, worst
    return ref


@pytest.mark.parametrize("name", sorted(R.BWD_CASES))
def test_backward_matches_the_restatement(dev, name):
    K = _K()
    c = R.bwd_case(name)
    B, S, n, k, F1, F2, D = c["shape"]
    g = _fwd_on_gpu(dev, c)
    rows, L0 = g["rows"], g["L0"]
    full = np.random.default_rng(3).standard_normal((B, L0 + 2, D)).astype(np.float32)
    full[:, rows] = c["dy"].reshape(B, S * n, D)
    dx0 = _t(full, dev)[:, :L0]                                    # a padded batch stride
    got = _bwd_on_gpu(dev, c, g, dx0)
    ref = _check_grads(c, g, got, c["dy"], name)
    assert all(np.abs(v).sum() > 0 for v in ref.values())
    K.device_status()


@pytest.mark.parametrize("name", sorted(R.BWD_CASES))
@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_backward_one_token_at_a_time(dev, name, which):
    """dx0 non-zero on a single row: a dropped or doubled contribution is an O(1) error."""
    K = _K()
    c = R.bwd_case(name)
    B, S, n, k, F1, F2, D = c["shape"]
    g = _fwd_on_gpu(dev, c)
    T = B * S * n
    t = {"first": 0, "middle": T // 2, "last": T - 1}[which]
    dy = np.zeros((T, D), np.float32)
    dy[t] = c["dy"].reshape(T, D)[t]
    dy = dy.reshape(B, S, n, D)
    full = np.zeros((B, g["L0"], D), np.float32)
    full[:, g["rows"]] = dy.reshape(B, S * n, D)
    got = _bwd_on_gpu(dev, c, g, _t(full, dev))
    ref = _check_grads(c, g, got, dy, f"{name}/{which}")
    assert np.abs(ref["w_out"]).sum() > 0 and np.abs(ref["b_out"]).sum() > 0
    K.device_status()


def test_backward_is_bitwise_reproducible_and_adds_once(dev):
    """(B, S, n, k, F1, F2, D) = (8, 2, 64, 16, 64, 64, 384): two runs into fresh buffers are
    bitwise equal; a run into a non-zero buffer adds the same gradient exactly once; inside a
    store in deterministic mode the bits are the same and the fixed-point shadow stays empty."""
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    from multi_modal_transformers_tokenmerge_amd.tokenizers.pointclouds.point_cloud_tokenizer \
        import PointCloudTokenizer
    K = _K()
    B, S, n, k, F1, F2, D, P = 8, 2, 64, 16, 64, 64, 384, 256
    rng = np.random.default_rng(4)
    c = dict(shape=(B, S, n, k, F1, F2, D), C=3,
             points=rng.standard_normal((B, S, P, 3)).astype(np.float32),
             params=R.init_params(rng, 3, F1, F2, D))
    g = _fwd_on_gpu(dev, c)
    dx0 = _t(rng.standard_normal((B, g["L0"], D)).astype(np.float32), dev)
    a = _bwd_on_gpu(dev, c, g, dx0)
    b = _bwd_on_gpu(dev, c, g, dx0)
    init = {key: torch.randn_like(v) for key, v in a.items()}
    acc = _bwd_on_gpu(dev, c, g, dx0, tuple(init[key].clone() for key in a))
    for key in a:
        assert float(a[key].abs().sum()) > 0, key
        assert torch.equal(a[key], b[key]), key
        assert torch.equal(acc[key], init[key] + a[key]), key
    store = ParamStore()
    tok = PointCloudTokenizer(k, 3, (F1, F2)).bind(store, "PointCloudTokenizer_0", D)
    store.materialize(dev, 0)
    with torch.no_grad():
        for p, key in zip(tok._all(), ("w1", "b1", "w2", "b2", "w_out", "b_out")):
            p.data.copy_(g["w"][key])
    sv = dict(points=g["pts"], cidx=g["cidx"], nidx=g["nidx"], argmax=g["argmax"])
    rows = _t(g["rows"], dev)
    with store.deterministic():
        store.zero_grad()
        tok.backward(dx0, sv, rows)
        torch.cuda.synchronize()
        assert not store.det_fx.any()
        store.det_flush()
        torch.cuda.synchronize()
        for p, key in zip(tok._all(), a):
            assert torch.equal(p.grad, a[key]), key
    K.device_status()


def test_assemble_leaves_pointcloud_rows_alone(dev):
    """mmt_seq_assemble_fwd does not write a row of kind 4 and mmt_seq_assemble_bwd does not read
    one: the sentinel survives, and d(readout_pe) sums the readout rows only."""
    from multi_modal_transformers_tokenmerge_amd import _C
    B, D, T, NI, NV, NPC, NR = 2, 64, 2, 3, 2, 4, 2
    kinds = [(0, j) for j in range(T)] + [(1, j) for j in range(NI)] + \
            [(4, j) for j in range(NPC)] + [(3, j) for j in range(NV)] + [(2, j) for j in range(NR)]
    L = len(kinds)
    row_src = torch.tensor([(k << 24) | j for k, j in kinds], dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(0)
    text = torch.randn((B, T, D), generator=g).bfloat16().to(dev)
    img = torch.randn((B, NI, D), generator=g).bfloat16().to(dev)
    Q = 4
    rt = torch.randint(0, Q, (B, NI), generator=g, dtype=torch.int32).to(dev)
    ct = torch.randint(0, Q, (B, NI), generator=g, dtype=torch.int32).to(dev)
    row_emb = torch.randn((Q, D), generator=g).to(dev)
    col_emb = torch.randn((Q, D), generator=g).to(dev)
    rpe = torch.randn((NR, D), generator=g).to(dev)            # fewer rows than point slots
    pe = torch.randn((L, D), generator=g).to(dev)
    x0 = torch.full((B, L, D), SENTINEL, device=dev)
    _C.call("mmt_seq_assemble_fwd", B, L, D, _C.ptr(row_src), _C.ptr(text), T, _C.ptr(img), NI,
            _C.ptr(rt), _C.ptr(ct), _C.ptr(row_emb), _C.ptr(col_emb), _C.ptr(rpe), _C.ptr(pe),
            _C.ptr(x0), _C.stream_ptr())
    torch.cuda.synchronize()
    skipped = [l for l, (k, _) in enumerate(kinds) if k >= 3]
    rrows = [l for l, (k, _) in enumerate(kinds) if k == 2]
    assert (x0[:, skipped] == SENTINEL).all()
    assert torch.equal(x0[:, rrows], (rpe + pe[rrows])[None].expand(B, -1, -1))
    assert torch.equal(x0[:, :T], text.float() + pe[:T])
    assert not (x0[:, T:T + NI] == SENTINEL).any()
    dx0 = torch.randn((B, L, D), generator=g).to(dev)
    dtext = torch.zeros((B, T, D), dtype=torch.bfloat16, device=dev)
    dimg = torch.zeros((B, NI, D), dtype=torch.bfloat16, device=dev)
    img_rows = torch.arange(T, T + NI, dtype=torch.int32, device=dev)
    dbuf = torch.full((NR + NPC + 2, D), SENTINEL, device=dev)
    drpe = dbuf[1:1 + NR]
    drpe.zero_()
    _C.call("mmt_seq_assemble_bwd", B, L, D, _C.ptr(row_src), _C.ptr(dx0), _C.ptr(dtext), T,
            _C.ptr(dimg), NI, _C.ptr(rt), _C.ptr(ct), _C.ptr(img_rows), Q, None, None,
            _C.ptr(drpe), _C.stream_ptr())
    torch.cuda.synchronize()
    want = dx0[:, rrows].double().sum(0)
    np.testing.assert_allclose(drpe.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=1e-6)
    assert (dbuf[0] == SENTINEL).all() and (dbuf[1 + NR:] == SENTINEL).all()
    assert torch.equal(dimg, dx0[:, T:T + NI].bfloat16())
    _C.call("mmt_device_status", _C.stream_ptr())
