"""GPU: PointCloud token sets in the Octo model (tokenizers/pointclouds/point_cloud_tokenizer.py)
on a tiny model, D = 192, two blocks, [Image{16};PointCloud{8};Value{2};Readout{4}], P = 64: the
point-cloud rows of the assembled sequence and the tokenizer's gradients in situ against the
standalone tokenizer (bit for bit), a diffusion train step, the frozen backbone, the staged
backward, the `point_clouds` keyword's checks and the YAML configuration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, P = 3, 64
SEQ = dict(input_sequence="[Image{16};PointCloud{8};Value{2};Readout{4}]",
           point_cloud_tokenizer=dict(num_points=P, num_neighbours_knn=8))
LEAVES = ("LBR_1/kernel", "LBR_1/bias", "LBR_2/kernel", "LBR_2/bias", "output_dense/kernel",
          "output_dense/bias")
_MODELS = {}


def _model(dev, **kw):
    """One model for the whole file (tests leave its parameters as they found them)."""
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    key = tuple(sorted(kw.items()))
    if key not in _MODELS:
        m = O.Octo(get_config("octo-tiny", num_blocks=2, **{**SEQ, **kw}), dev, seed=0)
        t = m.point_cloud_tokenizer
        if t is not None:       # non-zero biases: their gradients and the bias adds are exercised
            g = torch.Generator().manual_seed(3)
            with torch.no_grad():
                for p in (t.b1, t.b2, t.b_out):
                    p.data.copy_(0.1 * torch.randn(p.shape, generator=g))
        _MODELS[key] = m
    return _MODELS[key], O


def _batch(dev, m, seed=0):
    cfg = m.cfg
    g = torch.Generator().manual_seed(seed)
    S = cfg.image_size[0]
    images = torch.randint(0, 256, (B, m.n_images, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    actions = torch.randn((B, cfg.action_space_dim), generator=g).to(dev)
    values = (torch.rand((B, m.n_value_sets, 2), generator=g) * 1.8 - 0.9).to(dev)
    clouds = torch.randn((B, m.n_pc_sets, P, 3), generator=g).to(dev)
    return images, actions, values, clouds


def _rng(dev):
    return torch.tensor([11, 0], dtype=torch.int32, device=dev)


def _grads(m):
    return {leaf: m.store.by_name[f"PointCloudTokenizer_0/{leaf}"].grad for leaf in LEAVES}


def test_rows_and_gradients_in_situ(dev, monkeypatch):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from tests import pointcloud_ref as R
    m, _ = _model(dev)
    images, actions, values, clouds = _batch(dev, m)
    seen = {}
    fwd, bwd = m.stack.forward, m._backward_tokens
    monkeypatch.setattr(m.stack, "forward",
                        lambda x0, ctxs: (seen.__setitem__("x0", x0.clone()), fwd(x0, ctxs))[1])
    monkeypatch.setattr(m, "_backward_tokens",
                        lambda st, dx0: (seen.__setitem__("dx0", dx0.clone()), bwd(st, dx0))[1])
    m.store.zero_grad()
    loss, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev),
                                                sample_offset=2, values=values,
                                                point_clouds=clouds)
    m.backward(st)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    t = m.point_cloud_tokenizer
    rows = m.pc_rows.long()
    assert rows.tolist() == list(range(16, 24))
    # train mode: the first centroid is the counter-RNG draw for the global cloud index
    np.testing.assert_array_equal(st["pc_sv"]["cidx"][:, :, 0].cpu().numpy(),
                                  R.drawn_start(11, 0, B, 1, P, sample_offset=2))
    # the rows: the standalone tokenizer's output (same start) plus pos_embed, bit for bit
    alone = t(clouds[:, 0], 8, start=st["pc_sv"]["cidx"][:, :, 0].contiguous())
    torch.cuda.synchronize()
    assert tuple(alone.shape) == (B, 8, m.D) and float(alone.abs().sum()) > 0
    assert torch.equal(seen["x0"][:, rows], alone + m.pos_embed.data[rows])
    assert torch.equal(t.last_saved["nidx"], st["pc_sv"]["nidx"])
    # the gradients: non-zero, and the standalone backward fed the model's dx0, bit for bit
    got = {leaf: g.clone() for leaf, g in _grads(m).items()}
    assert all(float(g.abs().sum()) > 0 for g in got.values())
    assert float(seen["dx0"][:, rows].abs().sum()) > 0
    fresh = tuple(torch.zeros_like(p.data) for p in t._all())
    sv = st["pc_sv"]
    K.pc_embed_bwd(seen["dx0"], m.pc_rows, clouds, sv["cidx"], sv["nidx"], sv["argmax"],
                   t.w1.data, t.b1.data, t.w2.data, t.b2.data, t.w_out.data, fresh)
    torch.cuda.synchronize()
    for leaf, f in zip(LEAVES, fresh):
        assert torch.equal(got[leaf], f), leaf
    K.device_status()


def test_eval_mode_and_injected_start(dev):
    m, _ = _model(dev)
    images, actions, values, clouds = _batch(dev, m)
    kw = dict(values=values, point_clouds=clouds)
    _, st = m.generate_readouts(None, images, False, None, **kw)
    assert not st["pc_sv"]["cidx"][:, :, 0].any()                 # eval: point 0
    start = torch.tensor([[5], [63], [0]], dtype=torch.int32, device=dev)
    _, st = m.generate_readouts(None, images, True, _rng(dev), fps_start=start, **kw)
    assert torch.equal(st["pc_sv"]["cidx"][:, :, 0], start)
    a = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev),
                                         inject=dict(fps_start=start), **kw)[0]
    b = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev), **kw)[0]
    torch.cuda.synchronize()
    assert np.isfinite(float(a)) and not torch.equal(a, b)


def test_diffusion_train_step_is_finite_and_updates_the_tokenizer(dev):
    m, O = _model(dev)
    images, actions, values, clouds = _batch(dev, m)
    snap = m.store.flat.clone()
    try:
        state = O.create_octo_train_state(m, seed=7)
        with pytest.raises(ValueError):
            O.diffusion_train_step(m, state, None, images, actions, values=values)
        state, grads = O.diffusion_train_step(m, state, None, images, actions, values=values,
                                              point_clouds=clouds)
        torch.cuda.synchronize()
        assert state.step == 1 and np.isfinite(float(state.last_loss))
        for leaf in LEAVES:
            assert float(grads[f"PointCloudTokenizer_0/{leaf}"].abs().sum()) > 0, leaf
        w = m.point_cloud_tokenizer.w2
        assert not torch.equal(w.data, snap[w.offset:w.offset + w.numel].view(w.shape))
        assert torch.isfinite(m.store.flat).all()
    finally:
        m.store.flat.copy_(snap)
        m.store.sync_shadow()


def test_frozen_backbone_leaves_the_tokenizer_alone(dev):
    m, O = _model(dev)
    images, actions, values, clouds = _batch(dev, m)
    try:
        O.create_octo_train_state(m, O.AdamW(frozen_keys="head_only"))
        assert m._cut == (m.cfg.num_blocks, True)                 # the cut lies above the tokens
        m.store.zero_grad()
        _, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev),
                                                 values=values, point_clouds=clouds)
        m.backward(st)
        torch.cuda.synchronize()
        assert all(not g.any() for g in _grads(m).values())
        assert float(m.head.d2.w.grad.abs().sum()) > 0
        names = [p.name for p in m.store.params if not p.name.startswith("PointCloudTokenizer_0/")]
        O.create_octo_train_state(m, O.AdamW(frozen_keys=names))
        assert m._cut == (0, False)                               # the tokenizer alone trained
    finally:
        O.create_octo_train_state(m, O.AdamW())


def test_staged_backward_equals_the_unstaged_one(dev):
    m, _ = _model(dev)
    images, actions, values, clouds = _batch(dev, m)
    kw = dict(values=values, point_clouds=clouds)
    t = m.point_cloud_tokenizer
    assert m.tail_region() == (m.value_tokenizer.embedding.offset, m.store.n)   # both tokenizers
    assert m.tail_region()[0] < t.first_offset < m.store.n
    regions = m.grad_regions(2)
    assert regions[0][1] == m.tail_region()[0] and regions[-1][0] == 0
    m.store.zero_grad()
    _, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev), **kw)
    m.backward(st)
    ref = m.store.flat_grad.clone()
    m.store.zero_grad()
    _, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev), **kw)
    for k in range(2):
        m.backward_stage(st, k, 2)
    torch.cuda.synchronize()
    lo = t.first_offset
    assert float(ref[lo:].abs().sum()) > 0
    assert torch.equal(m.store.flat_grad[lo:], ref[lo:])          # no atomics: the same bits
    torch.testing.assert_close(m.store.flat_grad, ref, rtol=1e-4, atol=1e-6)
    only, _ = _model(dev, input_sequence="[Image{16};PointCloud{8};Readout{4}]")
    assert only.tail_region() == (only.point_cloud_tokenizer.first_offset, only.store.n)


def test_point_clouds_keyword_is_checked(dev):
    m, _ = _model(dev)
    images, actions, values, clouds = _batch(dev, m)
    rng = _rng(dev)
    loss = lambda **kw: m.compute_diffusion_denoise_loss(None, images, actions, True, rng,
                                                         values=values, **kw)[0]
    bad = [None, clouds.double(), clouds.cpu(), clouds[:2], clouds[:, :, :60], clouds[:, 0],
           torch.cat([clouds, clouds], 3), torch.cat([clouds, clouds], 1)]
    for pc in bad:
        with pytest.raises(ValueError):
            loss(point_clouds=pc)
    with pytest.raises(ValueError):
        m.predict_diffusion_action(None, images, rng, values=values)
    out = m.predict_diffusion_action(None, images, rng, values=values, point_clouds=clouds)
    assert tuple(out.shape) == (B, m.cfg.action_space_dim) and torch.isfinite(out).all()
    plain, _ = _model(dev, input_sequence="[Image{16};Value{2};Readout{4}]",
                      point_cloud_tokenizer=None)
    with pytest.raises(ValueError, match="no PointCloud set"):
        plain.compute_diffusion_denoise_loss(None, images, actions, True, rng, values=values,
                                             point_clouds=clouds)


def test_yaml_config_loads_and_builds(dev):
    from multi_modal_transformers_tokenmerge_amd import checkpoint as C
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    from multi_modal_transformers_tokenmerge_amd.tokenizers.text.t5_base import T5Config
    cfg = get_config("octo_small_tome16_pc64", num_blocks=1, t5=T5Config(num_layers=1))
    m = O.Octo(cfg, dev, seed=0)
    t = m.point_cloud_tokenizer
    assert (m.pc_points, m.pc_tokens, t.k, t.C, t.F1, t.F2) == (1024, 64, 16, 3, 64, 64)
    assert m.pc_rows.tolist() == list(range(32 + 256, 32 + 256 + 64))
    assert m.layer_sets[0][0].lens == [32, 256, 64, 4]
    tree = C.to_flax_params(m)["PointCloudTokenizer_0"]
    assert tree["LBR_2"]["kernel"].shape == (64, 64)
    assert tree["output_dense"]["kernel"].shape == (64, 384)


def test_ddp_step_captures_with_point_clouds(dev):
    """The one-graph training step with a static `point_clouds` buffer: the captured replay
    repeats the eager step bitwise (deterministic mode) and reads the buffer on every replay."""
    from multi_modal_transformers_tokenmerge_amd import _C
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    m, O = _model(dev, token_compression_sequence="[Image{2};PointCloud{0};Value{0};Readout{0}]")
    images, actions, values, clouds = _batch(dev, m)
    other = _batch(dev, m, seed=1)[3]
    buf = clouds.clone()
    state = O.create_octo_train_state(m, seed=7)
    st = m.store
    kept = (st.flat, st.flat_bf16, st.m, st.v, state.rng)
    start = [t.clone() for t in kept]

    def restore():
        for d, v in zip(kept, start):
            d.copy_(v)
        st.refresh_transposed()
        st.refresh_fp8()
    try:
        st.set_deterministic(True)
        state, _ = O.diffusion_train_step(m, state, None, images, actions, values=values,
                                          point_clouds=clouds)
        torch.cuda.synchronize()
        eager_loss, eager_flat = state.last_loss.clone(), st.flat.clone()
        restore()
        with pytest.raises(ValueError):
            DDPStep(m, state, None, images, actions, None, use_graph=True, values=values)
        step = DDPStep(m, state, None, images, actions, None, use_graph=True, values=values,
                       point_clouds=buf).build()
        step()
        torch.cuda.synchronize()
        assert np.isfinite(float(eager_loss)) and float(eager_loss) > 0
        assert torch.equal(step.loss_buf.view(-1), eager_loss.view(-1))
        assert torch.equal(st.flat, eager_flat)
        restore()
        buf.copy_(other)
        step()
        torch.cuda.synchronize()
        assert not torch.equal(step.loss_buf.view(-1), eager_loss.view(-1))
    finally:
        st.set_deterministic(False)
        restore()
    _C.call("mmt_device_status", _C.stream_ptr())
