"""GPU: Value token sets in the Octo model (tokenizers/numeric_values/value_tokenizer.py): the
value rows of the assembled sequence and the embedding's gradient in situ, the `values` keyword of
the losses and train steps, the static tables next to ToMe, the frozen backbone, the captured step
(DDPStep(values=...)) and the checkpoint tree. The numpy reference is tests/value_tokens_ref.py."""
import numpy as np
import pytest
import torch

from tests import value_tokens_ref as R

pytestmark = pytest.mark.gpu

B = 3
ONE = dict(input_sequence="[Image{16};Value{5};Readout{4}]")
TWO = dict(input_sequence="[Image{16};Value{3};Readout{4}]*2", num_observation_blocks=2)
TOME = dict(input_sequence="[Image{16};Value{5};Readout{4}]",
            token_compression_sequence="[Image{2};Value{0};Readout{0}]")
VARIANTS = {"one": ONE, "two-steps": TWO, "tome": TOME}
_MODELS = {}


def _model(dev, key="one", **kw):
    """One model per variant for the whole file (tests leave its parameters as they found them)."""
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    if kw or key not in _MODELS:
        cfg = get_config("octo-tiny", num_blocks=2, **{**VARIANTS[key], **kw})
        m = O.Octo(cfg, dev, seed=0)
        if kw:
            return m, O
        _MODELS[key] = m
    return _MODELS[key], O


def _batch(dev, m, seed=0):
    cfg = m.cfg
    g = torch.Generator().manual_seed(seed)
    S = cfg.image_size[0]
    images = torch.randint(0, 256, (B, m.n_images, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    actions = torch.randn((B, cfg.action_space_dim), generator=g).to(dev)
    N = m.value_tokenizer.num_bins
    rng = np.random.default_rng(seed)
    tok = rng.integers(0, N, (B, m.n_value_sets, m.n_values // m.n_value_sets))
    vals = R.bin_centre_values(tok, N, m.value_tokenizer.mu, m.value_tokenizer.encoding, rng)
    return images, actions, torch.from_numpy(vals).to(dev), tok.reshape(B, -1).astype(np.int32)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rng(dev):
    return torch.tensor([11, 0], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("key", list(VARIANTS))
def test_value_rows_and_embedding_gradient_in_situ(dev, key, monkeypatch):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    m, _ = _model(dev, key)
    images, actions, values, tok = _batch(dev, m)
    seen = {}
    fwd, bwd = m.stack.forward, m._backward_tokens
    monkeypatch.setattr(m.stack, "forward",
                        lambda x0, ctxs: (seen.__setitem__("x0", x0.clone()), fwd(x0, ctxs))[1])
    monkeypatch.setattr(m, "_backward_tokens",
                        lambda st, dx0: (seen.__setitem__("dx0", dx0.clone()), bwd(st, dx0))[1])
    m.store.zero_grad()
    loss, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev),
                                                values=values)
    m.backward(st)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    rows = m.value_rows.cpu().numpy()
    N = m.value_tokenizer.num_bins
    np.testing.assert_array_equal(st["val_tok"].cpu().numpy(), tok)
    np.testing.assert_array_equal(R.tokens(values.cpu().numpy().reshape(B, -1), N), tok)
    emb, pe = m.value_tokenizer.embedding, m.pos_embed
    x0 = seen["x0"].cpu().numpy()
    np.testing.assert_array_equal(
        _bits(x0[:, rows]), _bits(R.forward_rows(tok, emb.data.cpu().numpy(),
                                                 pe.data.cpu().numpy(), rows)))
    dx0 = seen["dx0"].cpu().numpy()
    assert np.abs(dx0[:, rows]).sum() > 0
    np.testing.assert_array_equal(_bits(emb.grad), _bits(R.table_grad(dx0, tok, rows, N)))
    # d(pos_embedding) over the value rows: the batch sum of dx0 there. K.colsum sums B = 3 fp32
    # terms per element in an order of its own: at most 2 roundings of at most 2^-24 sum|terms|
    got = pe.grad.cpu().numpy()[rows]
    bound = 2.0 * 2.0 ** -24 * np.abs(dx0[:, rows]).sum(0) + 1e-30
    assert (np.abs(got - dx0[:, rows].astype(np.float64).sum(0)) <= bound).all()
    K.device_status()


def test_tables_next_to_tome(dev):
    """A Value set between Image and Readout under ToMe: its length is constant across the layers
    while the image set shrinks, and the readout rows follow."""
    m, _ = _model(dev, "tome")
    assert [m.layer_sets[i][0].lens for i in range(2)] == [[16, 5, 4], [14, 5, 4]]
    assert [m.layer_sets[i][0].starts for i in range(2)] == [[0, 16, 21], [0, 14, 19]]
    assert [m.layer_sets[i][0].vis for i in range(2)] == [[0b011, 0b011, 0b111]] * 2
    assert [m.layer_sets[i][2:4] for i in range(2)] == [(0, 2), (0, 2)]       # ToMe: set 0, r = 2
    assert m.L_final == 21 and m.readout_rows.tolist() == [17, 18, 19, 20]
    assert m.value_rows.tolist() == [16, 17, 18, 19, 20]
    two, _ = _model(dev, "two-steps")
    assert two.value_rows.tolist() == [16, 17, 18, 39, 40, 41] and two.n_value_sets == 2
    assert two.readout_rows.tolist() == [19, 20, 21, 22, 42, 43, 44, 45]


def test_values_keyword_of_the_losses(dev):
    m, O = _model(dev, "one")
    images, actions, values, _ = _batch(dev, m)
    _, _, other, _ = _batch(dev, m, seed=1)
    rng = _rng(dev)
    loss = lambda **kw: m.compute_diffusion_denoise_loss(None, images, actions, True, rng, **kw)[0]
    a, b, c = loss(values=values), loss(values=values.clone()), loss(values=other)
    flat = loss(values=values.reshape(B, -1))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, flat) and not torch.equal(a, c)
    bad = [None, values[:, :, :4], values[:2], values.double(), values.reshape(-1),
           values.reshape(B, -1, 1), values.cpu()]
    for v in bad:
        with pytest.raises(ValueError):
            loss(values=v)
    with pytest.raises(ValueError):
        m.predict_diffusion_action(None, images, rng)
    out = m.predict_diffusion_action(None, images, rng, values=values)
    assert tuple(out.shape) == (B, m.cfg.action_space_dim) and torch.isfinite(out).all()
    plain, _ = _model(dev, "one", input_sequence="[Image{16};Readout{4}]")
    with pytest.raises(ValueError, match="no Value set"):
        plain.compute_diffusion_denoise_loss(None, images, actions, True, rng, values=values)
    assert plain.value_tokenizer is None and plain.tail_region() is None


def test_other_heads_and_train_steps_take_values(dev):
    m, O = _model(dev, "one", action_heads=("diffusion", "continuous", "categorical"),
                  tokens_per_readout=8, input_sequence="[Image{16};Value{5};Readout{8}]")
    images, actions, values, _ = _batch(dev, m)
    snap = m.store.flat.clone()
    for step, act in ((O.continuous_train_step, actions),
                      (O.categorical_train_step, actions.clamp(-1, 1))):
        state = O.create_octo_train_state(m, seed=7)
        with pytest.raises(ValueError):
            step(m, state, None, images, act)
        state, grads = step(m, state, None, images, act, values=values)
        assert state.step == 1 and np.isfinite(float(state.last_loss))
        assert float(grads["ValueTokenizer_0/embedding"].abs().sum()) > 0
    assert not torch.equal(m.store.flat, snap)
    rng = _rng(dev)
    assert torch.isfinite(m.predict_continuous_action(None, images, rng, values=values)).all()
    assert torch.isfinite(m.predict_action_logits(None, images, rng, values=values)).all()


def test_frozen_backbone_skips_the_token_backward(dev, monkeypatch):
    m, O = _model(dev, "one")
    images, actions, values, _ = _batch(dev, m)
    calls = []
    bwd = m._backward_tokens
    monkeypatch.setattr(m, "_backward_tokens", lambda st, dx0: (calls.append(1), bwd(st, dx0))[1])
    try:
        O.create_octo_train_state(m, O.AdamW(frozen_keys="head_only"))
        assert m._cut == (m.cfg.num_blocks, True)
        m.store.zero_grad()
        _, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev),
                                                 values=values)
        m.backward(st)
        torch.cuda.synchronize()
        assert not calls and not m.value_tokenizer.embedding.grad.any()
        assert float(m.head.d2.w.grad.abs().sum()) > 0
        # the embedding alone trained: the whole backward runs again
        names = [p.name for p in m.store.params if p.name != "ValueTokenizer_0/embedding"]
        O.create_octo_train_state(m, O.AdamW(frozen_keys=names))
        assert m._cut == (0, False)
        m.store.zero_grad()
        _, st = m.compute_diffusion_denoise_loss(None, images, actions, True, _rng(dev),
                                                 values=values)
        m.backward(st)
        torch.cuda.synchronize()
        assert calls and float(m.value_tokenizer.embedding.grad.abs().sum()) > 0
    finally:
        O.create_octo_train_state(m, O.AdamW())


def test_ddp_step_captures_with_values(dev):
    """The one-graph training step with a static `values` buffer: captured and replayed once it
    repeats the eager step bitwise (deterministic mode), and it reads the buffer on every replay."""
    from multi_modal_transformers_tokenmerge_amd import _C
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    m, O = _model(dev, "tome")
    images, actions, values, _ = _batch(dev, m)
    _, _, other, _ = _batch(dev, m, seed=1)
    buf = values.clone()
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
        state, _ = O.diffusion_train_step(m, state, None, images, actions, values=values)
        torch.cuda.synchronize()
        eager_loss, eager_flat = state.last_loss.clone(), st.flat.clone()
        restore()
        with pytest.raises(ValueError):
            DDPStep(m, state, None, images, actions, None, use_graph=True)
        step = DDPStep(m, state, None, images, actions, None, use_graph=True, values=buf).build()
        assert len(step.graphs) == 1
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


def test_checkpoint_round_trip(dev):
    from multi_modal_transformers_tokenmerge_amd import checkpoint as C
    m, _ = _model(dev, "one")
    tree = C.to_flax_params(m)
    leaf = tree["ValueTokenizer_0"]["embedding"]
    emb = m.value_tokenizer.embedding
    assert leaf.shape == emb.shape and leaf.dtype == np.float32
    np.testing.assert_array_equal(_bits(leaf), _bits(emb.data))
    other, _ = _model(dev, "one", value_tokenizer=dict(num_bins=256))
    other.value_tokenizer.embedding.data.zero_()
    assert C.load_flax_params(other, tree) == []
    np.testing.assert_array_equal(_bits(other.value_tokenizer.embedding.data), _bits(emb.data))
    plain, _ = _model(dev, "one", input_sequence="[Image{16};Readout{4}]")
    assert "ValueTokenizer_0" not in C.to_flax_params(plain)


def test_standalone_module(dev):
    """The module form: tokens() and __call__ (the table rows alone, no position term)."""
    from multi_modal_transformers_tokenmerge_amd.tokenizers.numeric_values.value_tokenizer import \
        ValueTokenizer
    t = ValueTokenizer(num_bins=16, mu=100.0, embedding_dim=24)
    rng = np.random.default_rng(0)
    want = rng.integers(0, 16, (2, 3, 4))
    v = torch.from_numpy(R.bin_centre_values(want, 16, 100.0, "mu_law", rng)).to(dev)
    tok, out = t.tokens(v), t(v)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tok.cpu().numpy(), want)
    table = t.params["ValueTokenizer_0/embedding"]
    assert tuple(out.shape) == (2, 3, 4, 24) and torch.equal(out, table[tok.long()] + 0.0)
    with pytest.raises(ValueError):
        ValueTokenizer()(v)                                     # unbound without embedding_dim
