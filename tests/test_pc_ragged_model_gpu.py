"""GPU: `point_cloud_counts` in the Octo model on a tiny configuration, D = 192, two blocks,
[Image{16};PointCloud{4};Readout{4}], 64 x 64 images, P = 32, k = 3: full counts against an
all-present set mask, a thin cloud against the set mask that flags it absent, the invisibility of
the tail rows (all bit for bit, deterministic mode), the train step and the captured DDPStep
following new contents of the counts buffer, the argument checks and the depth pipeline."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, P, N, KNN = 4, 32, 4, 3
SEQ = dict(input_sequence="[Image{16};PointCloud{4};Readout{4}]",
           point_cloud_tokenizer=dict(num_points=P, num_neighbours_knn=KNN))
TOME = "[Image{2};PointCloud{0};Readout{0}]"
IMG, PC, READ = range(3)
LEAVES = ("LBR_1/kernel", "LBR_1/bias", "LBR_2/kernel", "LBR_2/bias", "output_dense/kernel",
          "output_dense/bias")
_MODELS = {}


def _model(dev, **kw):
    """One model per configuration for the whole file (tests leave the parameters as found)."""
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    key = tuple(sorted(kw.items()))
    if key not in _MODELS:
        m = O.Octo(get_config("octo-tiny", num_blocks=2, **{**SEQ, **kw}), dev, seed=0)
        t = m.point_cloud_tokenizer
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():      # non-zero biases: their gradients are exercised
            for p in (t.b1, t.b2, t.b_out):
                p.data.copy_(0.1 * torch.randn(p.shape, generator=g))
        _MODELS[key] = m
    return _MODELS[key], O


def _batch(dev, m, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (B, 1, 64, 64, 3), generator=g, dtype=torch.uint8).to(dev)
    actions = torch.randn((B, m.cfg.action_space_dim), generator=g).to(dev)
    clouds = torch.randn((B, 1, P, 3), generator=g).to(dev)
    return images, actions, clouds


def _rng(dev):
    return torch.tensor([11, 0], dtype=torch.int32, device=dev)


def _i32(rows, dev):
    return torch.tensor(rows, dtype=torch.int32, device=dev).view(B, 1)


def _run(m, images, actions, **kw):
    """(final sequence, loss, all gradients, saved state) of one loss + backward."""
    m.store.zero_grad()
    loss, st = m.compute_diffusion_denoise_loss(None, images, actions, True,
                                                _rng(images.device), **kw)
    m.backward(st)
    torch.cuda.synchronize()
    return st["xL"].clone(), loss.clone(), m.store.flat_grad.clone(), st


def _pc_grads(m, flat):
    out = {}
    for leaf in LEAVES:
        p = m.store.by_name[f"PointCloudTokenizer_0/{leaf}"]
        out[leaf] = flat[p.offset:p.offset + p.numel]
    return out


@pytest.fixture()
def det(dev):
    m = _model(dev)[0]
    m.store.set_deterministic(True)
    yield m
    m.store.set_deterministic(False)


def test_full_counts_equal_an_all_present_set_mask(dev, det, monkeypatch):
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    m = det
    images, actions, clouds = _batch(dev, m)
    names = []
    call = _C.call
    monkeypatch.setattr(_C, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    a = _run(m, images, actions, point_clouds=clouds, point_cloud_counts=_i32([P] * B, dev))
    with_counts, names[:] = list(names), []
    ones = torch.ones((B, m.n_sets), dtype=torch.bool, device=dev)
    b = _run(m, images, actions, point_clouds=clouds, set_pad_mask=ones)
    swap = {"mmt_pad_mask_pack_counts": "mmt_pad_mask_pack",
            "mmt_pc_sample_group_counts": "mmt_pc_sample_group"}
    # the same launches but for the two entry points with counts, and no zeroed image copy
    assert [swap.get(n, n) for n in with_counts] == [n for n in names if n != "mmt_pad_mask_images"]
    assert "mmt_pad_mask_pack_counts" in with_counts and "mmt_pc_sample_group_counts" in with_counts
    assert "mmt_pad_mask_images" not in with_counts and "mmt_pad_mask_images" in names
    for x, y, what in zip(a[:3], b[:3], ("xL", "loss", "grads")):
        assert torch.equal(x, y), what
    assert np.isfinite(float(a[1])) and float(a[2].abs().sum()) > 0
    for key in ("cidx", "nidx", "argmax"):
        assert torch.equal(a[3]["pc_sv"][key], b[3]["pc_sv"][key]), key
    K.device_status()


def test_a_thin_cloud_is_an_absent_set(dev, det):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    m = det
    images, actions, clouds = _batch(dev, m)
    thin = _run(m, images, actions, point_clouds=clouds,
                point_cloud_counts=_i32([3, P, 20, N], dev))           # 3 < n = 4: absent
    mask = torch.ones((B, m.n_sets), dtype=torch.bool, device=dev)
    mask[0, PC] = False
    flagged = _run(m, images, actions, point_clouds=clouds, set_pad_mask=mask,
                   point_cloud_counts=_i32([P, P, 20, N], dev))
    for x, y, what in zip(thin[:3], flagged[:3], ("xL", "loss", "grads")):
        assert torch.equal(x, y), what
    g = _pc_grads(m, thin[2])
    assert all(float(v.abs().sum()) > 0 for v in g.values())           # the other samples' clouds
    for leaf, v in _pc_grads(m, flagged[2]).items():
        assert torch.equal(v, g[leaf]), leaf
    assert thin[3]["pad"][0].tolist() == [0b101, 0b111, 0b111, 0b111]
    # and it differs from the call that takes sample 0's cloud as present
    full = _run(m, images, actions, point_clouds=clouds,
                point_cloud_counts=_i32([P, P, 20, N], dev))
    assert not torch.equal(full[1], thin[1])
    K.device_status()


def test_tail_rows_change_no_bit(dev, det):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    m = det
    images, actions, clouds = _batch(dev, m)
    rows = [N, 9, 20, P - 1]                                            # n <= c < P
    counts = _i32(rows, dev)
    a = _run(m, images, actions, point_clouds=clouds, point_cloud_counts=counts)
    other = clouds.clone()
    for b, c in enumerate(rows):
        other[b, 0, c:] = torch.tensor([float("nan"), float("inf"), 1e30], device=dev)
    b_ = _run(m, images, actions, point_clouds=other, point_cloud_counts=counts)
    for x, y, what in zip(a[:3], b_[:3], ("xL", "loss", "grads")):
        assert torch.equal(x, y), what
    assert np.isfinite(float(a[1])) and torch.isfinite(a[2]).all()
    head = clouds.clone()
    head[1, 0, 0] += 1.0                                                # a valid row does matter
    assert not torch.equal(_run(m, images, actions, point_clouds=head,
                                point_cloud_counts=counts)[1], a[1])
    K.device_status()


def _state_guard(m, O):
    state = O.create_octo_train_state(m, seed=7)
    st = m.store
    kept = (st.flat, st.flat_bf16, st.m, st.v, state.rng)
    start = [t.clone() for t in kept]

    def restore():
        for d, v in zip(kept, start):
            d.copy_(v)
        st.refresh_transposed()
        st.refresh_fp8()
    return state, restore


def test_train_step_follows_the_counts_buffer(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    m, O = _model(dev)
    images, actions, clouds = _batch(dev, m)
    state, restore = _state_guard(m, O)
    first, second = _i32([P, 2, 17, N], dev), _i32([1, P, N, 30], dev)
    try:
        m.store.set_deterministic(True)
        want = []
        for c in (first, second):                                      # fresh tensors
            state, _ = O.diffusion_train_step(m, state, None, images, actions,
                                              point_clouds=clouds, point_cloud_counts=c)
            torch.cuda.synchronize()
            want.append((state.last_loss.clone(), m.store.flat.clone()))
            restore()
        assert not torch.equal(want[0][0], want[1][0])
        buf = first.clone()
        for c, (loss, flat) in zip((first, second), want):             # one buffer, rewritten
            buf.copy_(c)
            state, grads = O.diffusion_train_step(m, state, None, images, actions,
                                                  point_clouds=clouds, point_cloud_counts=buf)
            torch.cuda.synchronize()
            assert np.isfinite(float(state.last_loss))
            assert torch.equal(state.last_loss, loss) and torch.equal(m.store.flat, flat)
            restore()
        K.device_status()
    finally:
        m.store.set_deterministic(False)
        restore()


def test_captured_step_reads_the_counts_buffer(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    m, O = _model(dev, token_compression_sequence=TOME)
    images, actions, clouds = _batch(dev, m)
    state, restore = _state_guard(m, O)
    first, second = _i32([P, 2, 17, N], dev), _i32([1, P, N, 30], dev)
    st = m.store
    try:
        st.set_deterministic(True)
        eager = []
        for c in (first, second):
            state, _ = O.diffusion_train_step(m, state, None, images, actions,
                                              point_clouds=clouds, point_cloud_counts=c)
            torch.cuda.synchronize()
            eager.append((state.last_loss.clone(), st.flat.clone()))
            restore()
        assert not torch.equal(eager[0][0], eager[1][0])
        with pytest.raises(ValueError):
            DDPStep(m, state, None, images, actions, None, use_graph=True,
                    point_cloud_counts=first)                          # counts without clouds
        with pytest.raises(ValueError):
            DDPStep(m, state, None, images, actions, None, use_graph=True, point_clouds=clouds,
                    point_cloud_counts=first.long())
        cbuf = first.clone()
        step = DDPStep(m, state, None, images, actions, None, use_graph=True,
                       point_clouds=clouds, point_cloud_counts=cbuf).build()
        assert len(step.graphs) == 1 and step.point_cloud_counts is cbuf
        step()
        torch.cuda.synchronize()
        assert torch.equal(step.loss_buf.view(-1), eager[0][0].view(-1))
        assert torch.equal(st.flat, eager[0][1])
        restore()
        cbuf.copy_(second)       # the loader rewrites the static buffer: the replay reads it
        step()
        torch.cuda.synchronize()
        assert torch.equal(step.loss_buf.view(-1), eager[1][0].view(-1))
        assert torch.equal(st.flat, eager[1][1])
        K.device_status()
    finally:
        st.set_deterministic(False)
        restore()


def test_point_cloud_counts_keyword_is_checked(dev):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    m, O = _model(dev)
    images, actions, clouds = _batch(dev, m)
    rng = _rng(dev)
    ok = _i32([P] * B, dev)
    loss = lambda **kw: m.compute_diffusion_denoise_loss(None, images, actions, True, rng, **kw)[0]
    with pytest.raises(ValueError, match="without point_clouds"):
        m.generate_readouts(None, images, True, rng, point_cloud_counts=ok)
    wide = torch.full((B, 2), P, dtype=torch.int32, device=dev)
    for bad in (ok.long(), ok.float(), ok.view(B), ok[:2], wide, ok.cpu(), [P] * B):
        with pytest.raises(ValueError, match="point_cloud_counts"):
            loss(point_clouds=clouds, point_cloud_counts=bad)
    assert np.isfinite(float(loss(point_clouds=clouds, point_cloud_counts=ok)))
    plain = O.Octo(get_config("octo-tiny", num_blocks=1), dev, seed=0)
    with pytest.raises(ValueError, match="no PointCloud set"):
        plain.compute_diffusion_denoise_loss(None, images, actions, True, rng,
                                             point_cloud_counts=ok)
    prune = O.Octo(get_config("octo-tiny", num_blocks=1, compression="prune", **SEQ), dev, seed=0)
    with pytest.raises(ValueError, match="prune"):
        prune.compute_diffusion_denoise_loss(None, images, actions, True, rng,
                                             point_clouds=clouds, point_cloud_counts=ok)
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    K.device_status()


def test_other_heads_and_train_steps_take_the_counts(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    m, O = _model(dev, input_sequence="[Image{16};PointCloud{4};Readout{8}]", tokens_per_readout=8,
                  action_heads=("diffusion", "continuous", "categorical"))
    images, actions, clouds = _batch(dev, m)
    actions = actions.clamp(-1, 1)
    rng = _rng(dev)
    kw = dict(point_clouds=clouds, point_cloud_counts=_i32([P, 2, 17, N], dev))
    full = dict(point_clouds=clouds)
    for fn in (m.predict_continuous_action, m.predict_action_logits, m.predict_categorical_action):
        x, y = fn(None, images, rng, **kw), fn(None, images, rng, **full)
        assert torch.isfinite(x).all() and x.shape == y.shape
        if fn != m.predict_categorical_action:                         # (decoded bins may coincide)
            assert not torch.equal(x[1], y[1])                         # the sample with a thin cloud
    t = torch.zeros((B,), dtype=torch.int32, device=dev)
    assert torch.isfinite(m.predict_diffusion_denoise_term(None, images, t, actions, rng,
                                                           **kw)).all()
    assert torch.isfinite(m.predict_diffusion_action(None, images, rng, **kw)).all()
    snap = m.store.flat.clone()
    try:
        for step in (O.continuous_train_step, O.categorical_train_step, O.diffusion_train_step):
            state = O.create_octo_train_state(m, seed=7)
            state, grads = step(m, state, None, images, actions, **kw)
            assert state.step == 1 and np.isfinite(float(state.last_loss))
    finally:
        m.store.flat.copy_(snap)
        m.store.sync_shadow()
    K.device_status()


def test_depth_pipeline_with_an_empty_frame(dev, monkeypatch):
    """depth_to_point_cloud -> the loss, one frame without a valid pixel: a finite loss, that
    sample's cloud rows of x0 are pos_embedding alone, the saved state is kept."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.tokenizers.pointclouds import depth_to_point_cloud
    m, _ = _model(dev)
    images, actions, _ = _batch(dev, m)
    depth = np.random.default_rng(5).integers(400, 2600, (B, 1, 24, 40)).astype(np.uint16)
    depth[depth % 5 == 0] = 0                                           # holes
    depth[2] = 0                                                        # no valid pixel
    depth[3] = 0
    depth[3, 0, 0, :3] = 1000                                           # three valid pixels: < n
    depth = torch.from_numpy(depth).to(dev)
    intr = torch.tensor([36.0, 36.0, 20.0, 12.0], device=dev).expand(B, 1, 4).contiguous()
    clouds, counts = depth_to_point_cloud(depth, intr, P)
    assert counts.view(-1).tolist()[:1] == [P] and counts.view(-1).tolist()[2] == 0
    assert int(counts[3, 0]) == 3
    seen = {}
    fwd = m.stack.forward
    monkeypatch.setattr(m.stack, "forward",
                        lambda x0, ctxs: (seen.__setitem__("x0", x0.clone()), fwd(x0, ctxs))[1])
    m.store.zero_grad()
    loss, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev),
                                                point_clouds=clouds, point_cloud_counts=counts)
    m.backward(st)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and torch.isfinite(m.store.flat_grad).all()
    rows = m.pc_rows.long()
    pe = m.pos_embed.data[rows]
    for b in (2, 3):
        assert torch.equal(seen["x0"][b, rows], pe), b
    for b in (0, 1):
        assert not torch.equal(seen["x0"][b, rows], pe), b
    sv = st["pc_sv"]
    assert set(sv) >= {"points", "cidx", "nidx", "argmax"} and sv["points"] is clouds
    assert not sv["cidx"][2].any() and not sv["nidx"][2].any()          # the empty cloud: index 0
    assert int(sv["cidx"].max()) < P and int(sv["nidx"].max()) < P
    assert st["pad"][0].tolist() == [0b111, 0b111, 0b101, 0b101]
    K.device_status()
