"""The parameter EMA through the training step (AdamW.ema_decay, OCTOTrainState.ema_weights(),
DDPStep.build(), checkpoint) on octo-tiny, B = 4. Every run is inside store.deterministic(), so
two runs are comparable bit for bit:

1. the EMA does not perturb training, and follows the float64 recurrence over the recorded masters;
2. frozen parameters' EMA stays equal to them, the head's moves;
3. ema_weights() swaps the EMA in, with every shadow re-derived;
4. an action predicted inside the block equals a second model loaded with ema_params;
5. leaving the block restores every buffer (fp8 shadows too); no step, no nesting inside it;
6. DDPStep.build() leaves the EMA as it found it; graph replays equal eager steps of a twin;
7. save_train_state / load_train_state carry it.
"""
import numpy as np
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd.schedules import EmaDecay, WarmupCosine

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit round-off
B = 4


def _O():
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    return O


def _tiny(dev, seed=0, **kw):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from oracle.parity import _inputs
    model = _O().Octo(get_config("octo-tiny", num_blocks=2, **kw), dev, seed=seed)
    images, _, actions = _inputs(model, B)
    return model, torch.from_numpy(images).to(dev), torch.from_numpy(actions).to(dev)


def _same(a, b):
    """Bitwise equality."""
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    return torch.equal(a.view(view[a.element_size()]), b.view(view[b.element_size()]))


def _run(dev, tx, steps, seed=0):
    """`steps` eager diffusion_train_steps of a fresh model; the master after every step."""
    O = _O()
    model, img, act = _tiny(dev, seed)
    state = O.create_octo_train_state(model, tx, seed=7)
    masters = [model.store.flat.clone()]
    with model.store.deterministic():
        for _ in range(steps):
            state, _ = O.diffusion_train_step(model, state, None, img, act)
            masters.append(model.store.flat.clone())
        torch.cuda.synchronize()
    return model, state, img, act, masters


def test_training_is_not_perturbed(dev):
    O = _O()
    N, decay = 4, EmaDecay()
    model, state, _, _, masters = _run(dev, O.AdamW(ema_decay=decay), N)
    plain, pstate, _, _, _ = _run(dev, O.AdamW(), N)
    assert plain.store.ema is None and state.step == pstate.step == N
    for name in ("flat", "m", "v", "flat_bf16"):
        assert _same(getattr(model.store, name), getattr(plain.store, name)), name
    assert not _same(masters[0], masters[-1])
    # the float64 recurrence over the recorded masters, with the fp32 d and 1 - d of each step
    # (s = the count before the step); per step the kernel is within 2U (|d e| + |(1 - d) p|) <=
    # 2U max|.|, and the recurrence contracts (d <= 1), so the per-step bounds add
    e = masters[0].double()
    peak = masters[0].abs().double()
    for s in range(N):
        d = decay(s)
        d_f, omd_f = float(np.float32(d)), float(np.float32(1.0 - d))
        e = d_f * e + omd_f * masters[s + 1].double()
        peak = torch.maximum(peak, masters[s + 1].abs().double())
    err = (model.store.ema.double() - e).abs()
    bound = N * 2 * U * peak
    print(f"EMA vs float64 recurrence: worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert [decay(s) for s in range(N)][:2] == [0.0, 0.0] and decay(3) > decay(2) > 0
    assert not _same(model.store.ema, model.store.flat)  # steps 2 and 3 averaged
    assert state.last_ema_decay == decay(N - 1)
    views = state.ema_params
    for p in model.store.params:
        assert _same(views[p.name], model.store.ema[p.offset:p.offset + p.numel].view(p.shape))


def test_head_only_keeps_the_frozen_average(dev):
    O = _O()
    model, state, _, _, masters = _run(dev, O.AdamW(frozen_keys="head_only", ema_decay=0.9), 3)
    st = model.store
    assert st.chunk_flags is not None
    frozen = [p for p in st.params if p.frozen]
    head = [p for p in st.params if not p.frozen]
    assert frozen and head
    ema = state.ema_params
    for p in frozen:
        sl = slice(p.offset, p.offset + p.numel)
        assert _same(ema[p.name], p.data) and _same(st.flat[sl], masters[0][sl]), p.name
    moved = 0
    for p in head:
        sl = slice(p.offset, p.offset + p.numel)
        if not _same(st.flat[sl], masters[0][sl]):  # a parameter the step moved
            moved += 1
            assert not _same(ema[p.name], masters[0][sl].view(p.shape)), p.name
            assert not _same(ema[p.name], p.data), p.name
    assert moved >= len(head) // 2


def test_ema_weights_swaps_in(dev):
    O = _O()
    model, state, _, _, _ = _run(dev, O.AdamW(ema_decay=0.9), 3)
    st = model.store
    flat0, ema0 = st.flat.clone(), st.ema.clone()
    ptrs = [t.data_ptr() for t in (st.flat, st.ema, st.flat_bf16, st.flat_bf16_t)]
    with st.deterministic(), state.ema_weights() as inside:
        torch.cuda.synchronize()
        assert inside is state
        assert _same(st.flat, ema0) and _same(st.ema, flat0)
        assert _same(st.flat_bf16, st.flat.to(torch.bfloat16))
        transposed = [p for p in st.params if p.transposed]
        assert transposed
        for p in transposed:
            assert _same(p.bf16_t, p.bf16.t().contiguous()), p.name
        for p in st.params:  # the views every reader goes through
            assert _same(p.data, ema0[p.offset:p.offset + p.numel].view(p.shape))
        assert ptrs == [t.data_ptr() for t in (st.flat, st.ema, st.flat_bf16, st.flat_bf16_t)]
    torch.cuda.synchronize()
    assert _same(st.flat, flat0) and _same(st.ema, ema0)


def test_ema_weights_action_parity(dev):
    O = _O()
    model, state, img, _, _ = _run(dev, O.AdamW(ema_decay=0.9), 3)
    rng = torch.tensor([5, 11], dtype=torch.int32, device=dev)
    twin, _, _ = _tiny(dev, seed=1)
    twin.store.load_state_dict(state.ema_params)
    with model.store.deterministic():
        raw = model.predict_diffusion_action(None, img, rng, train=False).clone()
        with state.ema_weights():
            got = model.predict_diffusion_action(None, img, rng, train=False).clone()
        want = twin.predict_diffusion_action(None, img, rng, train=False).clone()
        again = model.predict_diffusion_action(None, img, rng, train=False).clone()
        torch.cuda.synchronize()
    assert got.shape == (B, model.cfg.action_space_dim) and bool(torch.isfinite(got).all())
    assert _same(got, want)
    assert _same(again, raw) and not _same(got, raw)  # the block did change what was evaluated


def _fp8_one_block(dev):
    """The fp8 preset, one encoder block and one T5 layer; its EMA moved off the master by hand
    (no step is needed to test the swap)."""
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.tokenizers.text.t5_base import T5Config
    O = _O()
    cfg = get_config("octo-base-hires-tome32", num_blocks=1, t5=T5Config(num_layers=1))
    assert cfg.fp8
    model = O.Octo(cfg, dev, seed=0)
    state = O.create_octo_train_state(model, O.AdamW(ema_decay=EmaDecay()), seed=7)
    gen = torch.Generator(device=dev).manual_seed(3)
    model.store.ema.mul_(1.0 + 0.05 * torch.randn(model.store.n, generator=gen, device=dev))
    return model, state


@pytest.mark.parametrize("which", ["tiny", "fp8"])
def test_ema_weights_restores_on_exit(dev, which):
    O = _O()
    if which == "tiny":
        model, state, _, _, _ = _run(dev, O.AdamW(ema_decay=0.9), 3)
    else:
        model, state = _fp8_one_block(dev)
    st = model.store
    assert (st.flat_fp8 is not None) == (which == "fp8") and st.flat_bf16_t is not None
    names = ["flat", "ema", "flat_bf16", "flat_bf16_t"] + (["flat_fp8", "fp8_scale"]
                                                          if which == "fp8" else [])
    torch.cuda.synchronize()
    before = {n: getattr(st, n).clone() for n in names}
    step0 = state.step
    with st.deterministic():
        with state.ema_weights():
            torch.cuda.synchronize()
            for n in names:  # every buffer did change
                assert not _same(getattr(st, n), before[n]), n
            assert _same(st.flat, before["ema"])
            with pytest.raises(RuntimeError, match="apply_gradients inside ema_weights"):
                state.apply_gradients()
            with pytest.raises(RuntimeError, match="already inside"):
                with state.ema_weights():
                    pass
        torch.cuda.synchronize()
        for n in names:
            assert _same(getattr(st, n), before[n]), n
        with pytest.raises(KeyError):  # an exception inside the block restores as well
            with state.ema_weights():
                raise KeyError("inside")
        torch.cuda.synchronize()
        for n in names:
            assert _same(getattr(st, n), before[n]), n
    assert state.step == step0
    with state.ema_weights():  # and the block can be entered again
        pass
    plain = O.create_octo_train_state(model, O.AdamW())
    with pytest.raises(AttributeError):
        plain.ema_weights()


def test_ddpstep_build_and_replays(dev):
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    O = _O()
    tx = O.AdamW(WarmupCosine(0.0, 1e-3, 2, 8), max_grad_norm=1.0, ema_decay=0.9)
    eager, estate, _, _, _ = _run(dev, tx, 5)

    model, state, img, act, _ = _run(dev, tx, 2)
    st = model.store
    kept = ("flat", "flat_bf16", "m", "v", "ema", "flat_bf16_t")
    before = {n: getattr(st, n).clone() for n in kept}
    assert not _same(st.ema, st.flat)
    with st.deterministic():
        step = DDPStep(model, state, None, img, act, None, use_graph=True).build()
        torch.cuda.synchronize()
        for n in kept:
            assert _same(getattr(st, n), before[n]), n
        assert len(step.graphs) == 1 and state.step == 2
        for _ in range(3):
            step()
        torch.cuda.synchronize()
    assert state.step == estate.step == 5
    for n in ("flat", "m", "v", "flat_bf16", "ema"):
        assert _same(getattr(st, n), getattr(eager.store, n)), n
    assert not _same(st.ema, before["ema"])


def test_checkpoint_round_trip(dev, tmp_path):
    from multi_modal_transformers_tokenmerge_amd import checkpoint as CK
    O = _O()
    model, state, _, _, _ = _run(dev, O.AdamW(ema_decay=0.9), 3)
    path = str(tmp_path / "ema.pt")
    CK.save_train_state(path, state)
    assert "ema" in torch.load(path, map_location="cpu", weights_only=True)

    other, _, _ = _tiny(dev, seed=1)
    fresh = O.create_octo_train_state(other, O.AdamW(ema_decay=0.9), seed=99)
    assert not _same(other.store.flat, model.store.flat)
    CK.load_train_state(path, fresh)
    assert _same(other.store.ema, model.store.ema) and _same(other.store.flat, model.store.flat)
    assert not _same(other.store.ema, other.store.flat) and fresh.step == 3

    # a file with an EMA, loaded into a state that keeps none: ignored
    bare = O.create_octo_train_state(other, O.AdamW(), seed=99)
    CK.load_train_state(path, bare)
    assert other.store.ema is None and _same(other.store.flat, model.store.flat)

    # a file without one, loaded into a state that keeps one: the average starts at the master
    plain_path = str(tmp_path / "plain.pt")
    CK.save_train_state(plain_path, bare)
    assert "ema" not in torch.load(plain_path, map_location="cpu", weights_only=True)
    third, _, _ = _tiny(dev, seed=2)
    tstate = O.create_octo_train_state(third, O.AdamW(ema_decay=EmaDecay()), seed=5)
    third.store.ema.fill_(7.0)
    CK.load_train_state(plain_path, tstate)
    assert _same(third.store.ema, third.store.flat) and _same(third.store.flat, model.store.flat)
    assert third.store.ema.data_ptr() != third.store.flat.data_ptr()
