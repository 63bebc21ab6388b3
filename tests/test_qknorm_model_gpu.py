"""GPU: QK-norm through the model (OctoConfig.normalize_qk): octo-tiny (D 192, 3 heads, Dh 64),
three blocks, ToMe Image{2} per block (L 20 -> 14), B = 2.

* Deterministic mode: the graphed diffusion train step equals the eager step bit for bit.
* One finite step: every block's two scales get a non-zero gradient and move under AdamW; with
  weight_decay_mask="kernels" and a zeroed gradient they keep their bits (their names do not end in
  /kernel) while the kernels decay; frozen_keys "*/query_ln/*" pins query_ln while key_ln moves.
* Flag off: losses and parameters after one step are bit-equal to the model whose config never
  names the flag; the flag-on model has num_blocks * 2 * Dh more parameters.
* fp8 and pruning: one forward / backward each stays finite with a clean device status.
"""
import math

import pytest
import torch

from oracle.parity import _inputs

pytestmark = pytest.mark.gpu

B, NB = 2, 3
TOME = "[Image{2};Readout{0}]"


def _model(dev, **kw):
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    kw.setdefault("token_compression_sequence", TOME)
    model = O.Octo(get_config("octo-tiny", num_blocks=NB, **kw), dev, seed=0)
    images, _, actions = _inputs(model, B, seed=3)
    return O, model, torch.from_numpy(images).to(dev), torch.from_numpy(actions).to(dev)


def _scales(model):
    return [(b.q_ln, b.k_ln) for b in model.stack.blocks]


def test_graphed_step_equals_eager(dev):
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    O, model, img, act = _model(dev, normalize_qk=True)
    assert model.L0 == 20
    state = O.create_octo_train_state(model, seed=7)
    st = model.store
    kept = (st.flat, st.flat_bf16, st.m, st.v, state.rng)
    start = [t.clone() for t in kept]
    try:
        st.set_deterministic(True)
        state, _ = O.diffusion_train_step(model, state, None, img, act)
        torch.cuda.synchronize()
        eager_loss, eager_flat = state.last_loss.clone(), st.flat.clone()
        for d, v in zip(kept, start):
            d.copy_(v)
        st.refresh_transposed()
        st.refresh_fp8()
        step = DDPStep(model, state, None, img, act, None, use_graph=True).build()
        assert len(step.graphs) == 1
        step()
        torch.cuda.synchronize()
        assert torch.equal(step.loss_buf.view(-1), eager_loss.view(-1))
        assert torch.equal(st.flat, eager_flat)
        assert math.isfinite(float(eager_loss))
        for q, k in _scales(model):    # the captured step trained the scales
            assert not torch.equal(q.data, torch.ones_like(q.data))
            assert not torch.equal(k.data, torch.ones_like(k.data))
    finally:
        st.set_deterministic(False)


def test_one_step_trains_the_scales(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    O, model, img, act = _model(dev, normalize_qk=True)
    st = model.store
    start = [t.clone() for t in (st.flat, st.flat_bf16, st.m, st.v)]

    def restore():
        for d, s in zip((st.flat, st.flat_bf16, st.m, st.v), start):
            d.copy_(s)
        st.refresh_transposed()
        st.zero_grad()

    # ---- gradients and a plain AdamW step
    state = O.create_octo_train_state(model, O.AdamW(learning_rate=1e-3), seed=7)
    st.zero_grad()
    loss, sv = model.compute_diffusion_denoise_loss(None, img, act, True, state.rng, 0)
    model.backward(sv)
    torch.cuda.synchronize()
    K.device_status()
    assert math.isfinite(float(loss)) and torch.isfinite(st.flat_grad).all()
    for q, k in _scales(model):
        assert q.grad.abs().max() > 0 and k.grad.abs().max() > 0, q.name
    grad = st.flat_grad.clone()
    state.apply_gradients()
    torch.cuda.synchronize()
    assert torch.isfinite(st.flat).all()
    for q, k in _scales(model):
        assert not torch.equal(q.data, torch.ones_like(q.data)), q.name
        assert not torch.equal(k.data, torch.ones_like(k.data)), k.name

    # ---- weight_decay_mask="kernels", zero gradient: the scales keep their bits, kernels decay
    restore()
    state = O.create_octo_train_state(
        model, O.AdamW(learning_rate=1e-2, weight_decay=0.1, weight_decay_mask="kernels"), seed=7)
    groups = state.param_groups
    for q, k in _scales(model):
        assert groups[q.name] == {"decay": False, "frozen": False} == groups[k.name]
    st.flat_grad.zero_()
    state.apply_gradients()
    torch.cuda.synchronize()
    for q, k in _scales(model):
        assert torch.equal(q.data, torch.ones_like(q.data)), q.name
        assert torch.equal(k.data, torch.ones_like(k.data)), k.name
    w = model.stack.blocks[0].qkv.w
    assert not torch.equal(w.data, start[0][w.offset:w.offset + w.numel].view(w.shape))

    # ---- frozen_keys reach the scales like any other parameter
    restore()
    state = O.create_octo_train_state(
        model, O.AdamW(learning_rate=1e-3, frozen_keys=("*/query_ln/*",)), seed=7)
    assert model._cut == (0, False)
    st.flat_grad.copy_(grad)
    state.apply_gradients()
    torch.cuda.synchronize()
    for q, k in _scales(model):
        assert torch.equal(q.data, torch.ones_like(q.data)), q.name
        assert not torch.equal(k.data, torch.ones_like(k.data)), k.name
    model.set_param_groups(None, None)


def test_flag_off_is_the_model_that_never_names_it(dev):
    results = []
    for kw in ({}, {"normalize_qk": False}):
        O, model, img, act = _model(dev, **kw)
        st = model.store
        with st.deterministic():
            state = O.create_octo_train_state(model, seed=7)
            state, _ = O.diffusion_train_step(model, state, None, img, act)
            torch.cuda.synchronize()
        assert all(sv_name.find("_ln/") < 0 for sv_name in st.by_name)
        results.append((state.last_loss.clone(), st.flat.clone(), model.num_params()))
    (l0, f0, n0), (l1, f1, n1) = results
    assert torch.equal(l0, l1) and torch.equal(f0, f1) and n0 == n1
    _, on, _, _ = _model(dev, normalize_qk=True)
    Dh = on.D // on.cfg.num_heads
    assert on.num_params() - n0 == NB * 2 * Dh


@pytest.mark.parametrize("kw", [dict(fp8=True),
                                dict(compression="prune",
                                     token_compression_sequence="[Image{2};Readout{1}]")],
                         ids=["fp8", "prune"])
def test_fp8_and_pruning_stay_finite(dev, kw):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    O, model, img, act = _model(dev, normalize_qk=True, **kw)
    state = O.create_octo_train_state(model, seed=7)
    model.store.zero_grad()
    loss, sv = model.compute_diffusion_denoise_loss(None, img, act, True, state.rng, 0)
    model.backward(sv)
    torch.cuda.synchronize()
    K.device_status()
    assert math.isfinite(float(loss)) and torch.isfinite(model.store.flat_grad).all()
    assert all(s["qk_pre"] is not None for s in sv["stack_sv"])
    for q, k in _scales(model):
        assert q.grad.abs().max() > 0 and k.grad.abs().max() > 0, q.name
