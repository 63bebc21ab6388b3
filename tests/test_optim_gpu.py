"""Device-resident optimizer control on the GPU (include/mmt_api.h mmt_optim_prepare /
mmt_adamw_dev; schedules.py; OCTOTrainState.opt):

1. the global gradient norm vs float64 at sizes around the grid's partition, to the bound its
   documented chain of fp32 roundings gives, and bitwise reproducible;
2. optax.clip_by_global_norm's factor and the folded grad_scale;
3. the three schedules evaluated on the device vs the host closed forms;
4. mmt_adamw_dev bit-identical to mmt_adamw given the same fp32 scalars;
5. non-finite gradients: flagged, skipped on request, propagated otherwise;
6. one captured graph trains through a moving learning rate, bit-equal to the eager steps;
7. resume files carry the optimizer's device words.
"""
import ctypes

import numpy as np
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd.schedules import Constant, WarmupCosine, WarmupRsqrt

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit round-off


def _C():
    from multi_modal_transformers_tokenmerge_amd import _C as C
    return C


def _chain(n: int) -> int:
    """Longest chain of fp32 roundings on any path to sum g^2 (include/mmt_api.h): a lane's
    accumulator takes ceil(per / 1024) fused multiply-adds, per = the workgroup's 16-B vectors,
    + 1 (tail) + 4 (a lane's 16 accumulators) + 6 (wave tree) + 2 (4 waves)."""
    G = _C().GRAD_NORM_GRID
    per = -(-(n // 4) // G)
    return -(-per // 1024) + 13


def _bufs(dev):
    C = _C()
    opt = torch.zeros(C.OPT_WORDS, dtype=torch.float32, device=dev)
    ws = torch.full((C.workspace_size(C.WS_GRAD_NORM, 1) // 4,), float("nan"), device=dev)
    state = torch.tensor([1234, 0], dtype=torch.int32, device=dev)
    return opt, ws, state


def _prepare(g, opt, ws, state, grad_scale=1.0, max_norm=0.0, skip=0, sched=None):
    C = _C()
    sc = (sched or Constant(1e-3)).to_c()
    C.call("mmt_optim_prepare", C.ptr(g), g.numel(), grad_scale, max_norm, skip,
           ctypes.addressof(sc), C.ptr(state), C.ptr(opt), C.ptr(ws), ws.numel() * 4,
           C.stream_ptr())


def _ulps(a, b) -> int:
    """Distance in fp32 representable values (same-sign finite a, b)."""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def _sizes():
    G = _C().GRAD_NORM_GRID
    return [1, 3, 255, 1024, G * 1024 - 1, G * 1024, G * 1024 + 1, 1_000_003]


def test_grid_constant_matches_workspace():
    C = _C()
    assert C.workspace_size(C.WS_GRAD_NORM, 12345) == 4 * C.GRAD_NORM_GRID


def test_norm_matches_float64_and_is_reproducible(dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    for n in _sizes():
        g = torch.randn(n, generator=gen, device=dev)
        ref = float(g.double().norm())
        got = []
        for _ in range(2):
            opt, ws, state = _bufs(dev)  # workspace full of NaN: every partial must be written
            _prepare(g, opt, ws, state)
            got.append(opt.cpu())
        A = _chain(n)
        rel = abs(float(got[0][0]) - ref) / ref
        print(f"n={n}: A={A} norm={float(got[0][0])!r} float64={ref!r} rel={rel:.3e} "
              f"bound={(A + 1) * U:.3e}")
        assert A <= 150
        assert rel <= (A + 1) * U <= 1e-5, (n, rel)
        assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), n
        assert got[0][1:].tolist() == [1.0, 1.0, np.float32(1e-3), 0.0, 0.0, 0.0, 0.0], n


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clip_and_scale(dev, grad_scale):
    n, max_norm = 100_003, 1.0
    gen = torch.Generator(device=dev).manual_seed(6)
    g0 = torch.randn(n, generator=gen, device=dev)
    g0 /= g0.double().norm().float() * grad_scale  # averaged norm ~ 1
    opt, ws, state = _bufs(dev)

    g = g0 * 4.0
    norm64 = grad_scale * float(g.double().norm())
    _prepare(g, opt, ws, state, grad_scale, max_norm)
    o = opt.cpu().numpy()
    assert _ulps(o[1], np.float32(max_norm / norm64)) <= 2, (o[1], max_norm / norm64)
    assert _ulps(o[2], np.float32(grad_scale) * o[1]) <= 2
    assert abs(float(o[0]) - norm64) <= 1e-5 * norm64

    g = g0 * 0.9
    _prepare(g, opt, ws, state, grad_scale, max_norm)
    o = opt.cpu().numpy()
    assert o[1] == np.float32(1.0) and o[2] == np.float32(grad_scale)

    _prepare(g0 * 4.0, opt, ws, state, grad_scale, 0.0)  # clipping off
    o = opt.cpu().numpy()
    assert o[1] == np.float32(1.0) and o[2] == np.float32(grad_scale)


def test_schedules_on_device(dev):
    INIT, PEAK, END, W, T, TAU = 1e-5, 3e-4, 3e-5, 10, 110, 50.0
    steps = [0, 1, W - 1, W, W + 1, W + (T - W) // 2, T, T + 5]
    g = torch.ones(1024, device=dev)
    _, ws, state = _bufs(dev)
    cases = [(f, s) for f in (Constant(2.5e-4), WarmupCosine(INIT, PEAK, W, T, END),
                              WarmupRsqrt(INIT, PEAK, W, TAU)) for s in steps]
    opts = torch.zeros((len(cases), 8), device=dev)
    for i, (f, s) in enumerate(cases):
        state[1] = s
        _prepare(g, opts[i], ws, state, sched=f)
    got = opts.cpu().numpy()
    for i, (f, s) in enumerate(cases):
        assert _ulps(got[i, 3], np.float32(f(s))) <= 1, (f, s, got[i, 3], f(s))
        assert got[i, 0] == np.float32(32.0)  # sqrt(1024 * 1)


def _adamw_state(dev, n, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    p = torch.randn(n, generator=gen, device=dev)
    return [p, torch.zeros_like(p), torch.zeros_like(p),
            torch.zeros(n, dtype=torch.bfloat16, device=dev)], gen


HYPER = (0.9, 0.999, 1e-8, 1e-2)


def _adamw_dev(bufs, g, state, opt):
    C = _C()
    p, m, v, sh = bufs
    C.call("mmt_adamw_dev", C.ptr(p), C.ptr(g), C.ptr(m), C.ptr(v), C.ptr(sh), p.numel(),
           C.ptr(state), C.ptr(opt), *HYPER, C.stream_ptr())


def test_adamw_dev_bit_identical_to_adamw(dev):
    C = _C()
    n = 100_003
    a, gen = _adamw_state(dev, n, 7)
    b = [t.clone() for t in a]
    opt, ws, state = _bufs(dev)
    sched = WarmupCosine(1e-4, 3e-3, 2, 6, 1e-4)
    for it in range(3):
        g = torch.randn(n, generator=gen, device=dev) * (it + 1)
        _prepare(g, opt, ws, state, 0.5, 1.0, 0, sched)
        o = opt.cpu().numpy()
        assert o[1] < 1.0 and _ulps(o[3], np.float32(sched(it))) <= 1  # clipping active
        _adamw_dev(a, g, state, opt)
        C.call("mmt_adamw", C.ptr(b[0]), C.ptr(g), C.ptr(b[1]), C.ptr(b[2]), C.ptr(b[3]), n,
               C.ptr(state), float(o[3]), *HYPER, float(o[2]), C.stream_ptr())
        C.call("mmt_step_advance", C.ptr(state), C.stream_ptr())
        torch.cuda.synchronize()
        for x, y, name in zip(a, b, ("p", "m", "v", "shadow")):
            assert torch.equal(x, y), (it, name)
    assert float(a[1].abs().sum()) > 0 and int(state[1]) == 3


@pytest.mark.parametrize("where", ["inf_in_tail", "nan_first"])
def test_nonfinite_gradient(dev, where):
    n = 100_003  # n % 4 == 3: the last element lies in the scalar tail
    bufs, gen = _adamw_state(dev, n, 8)
    clean = torch.randn(n, generator=gen, device=dev)
    bad = clean.clone()
    if where == "inf_in_tail":
        bad[-1] = float("inf")
    else:
        bad[0] = float("nan")
    opt, ws, state = _bufs(dev)
    # a clean step first, so the moments and the shadow are not trivially zero
    _prepare(clean, opt, ws, state, skip=1)
    _adamw_dev(bufs, clean, state, opt)
    before = [t.clone() for t in bufs]
    assert opt.cpu().tolist()[4:7] == [0.0, 0.0, 0.0]

    _prepare(bad, opt, ws, state, skip=1)
    _adamw_dev(bufs, bad, state, opt)
    o = opt.cpu().tolist()
    assert (o[4], o[5], o[6]) == (1.0, 1.0, 1.0)
    for x, y in zip(bufs, before):
        assert torch.equal(x, y)

    _prepare(clean, opt, ws, state, skip=1)
    _adamw_dev(bufs, clean, state, opt)
    o = opt.cpu().tolist()
    assert (o[4], o[5], o[6]) == (0.0, 1.0, 0.0)  # the count of skipped steps stays
    assert not torch.equal(bufs[0], before[0]) and bool(torch.isfinite(bufs[0]).all())

    _prepare(bad, opt, ws, state, skip=0)
    _adamw_dev(bufs, bad, state, opt)
    o = opt.cpu().tolist()
    assert (o[4], o[5], o[6]) == (1.0, 1.0, 0.0)
    assert bool(torch.isnan(bufs[0]).any())  # the update proceeds: NaN propagates, as in optax


def _tiny(dev, seed=0, B=3):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    from oracle.parity import _inputs
    model = O.Octo(get_config("octo-tiny", num_blocks=2), dev, seed=seed)
    images, _, actions = _inputs(model, B)
    return O, model, torch.from_numpy(images).to(dev), torch.from_numpy(actions).to(dev)


def test_one_graph_moving_learning_rate(dev):
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    O, model, img, act = _tiny(dev)
    sched = WarmupCosine(0, 1e-3, 2, 6)
    state = O.create_octo_train_state(model, O.AdamW(sched, max_grad_norm=1e-3), seed=7)
    st = model.store
    assert state.opt is not None and state.skipped_steps == 0
    want = [np.float32(sched(s)) for s in range(5)]
    # 0, 5e-4, 1e-3, 8.54e-4, 5e-4: the rate moves at every step of the one graph (the cosine's
    # midpoint at step 4 passes through the warm-up's value of step 1)
    assert all(a != b for a, b in zip(want, want[1:])) and len(set(want)) == 4
    kept = (st.flat, st.flat_bf16, st.m, st.v, state.rng)
    start = [t.clone() for t in kept]
    try:
        st.set_deterministic(True)
        for s in range(5):
            state, _ = O.diffusion_train_step(model, state, None, img, act)
            assert _ulps(state.last_lr, want[s]) <= 1, (s, state.last_lr, want[s])
            assert state.last_clip < 1.0 and state.last_grad_norm > 1e-3
        eager = [t.clone() for t in (st.flat, st.m, st.v)]
        assert state.step == 5

        for d, v in zip(kept, start):  # back to the initial weights, moments and counter
            d.copy_(v)
        st.refresh_transposed()
        st.refresh_fp8()
        opt_before = state.opt.clone()  # the words the eager steps left
        step = DDPStep(model, state, None, img, act, None, use_graph=True).build()
        torch.cuda.synchronize()
        assert torch.equal(state.opt.view(torch.int32), opt_before.view(torch.int32))
        assert len(step.graphs) == 1 and state.step == 0
        for s in range(5):
            step()
            assert _ulps(state.last_lr, want[s]) <= 1, (s, state.last_lr, want[s])
            assert state.last_clip < 1.0
        assert state.step == 5
        for a, b, name in zip(eager, (st.flat, st.m, st.v), ("flat", "m", "v")):
            assert torch.equal(a, b), name
    finally:
        st.set_deterministic(False)


def test_plain_adamw_keeps_no_device_words(dev):
    O, model, img, act = _tiny(dev)
    state = O.create_octo_train_state(model, seed=7)
    assert state.opt is None and state.opt_workspace is None
    with pytest.raises(AttributeError):
        state.last_lr


def test_resume_carries_optimizer_words(dev, tmp_path):
    from multi_modal_transformers_tokenmerge_amd import checkpoint as CK
    sched = WarmupRsqrt(1e-5, 1e-3, 4, 10.0)
    O, model, img, act = _tiny(dev)
    state = O.create_octo_train_state(model, O.AdamW(sched, skip_nonfinite=True), seed=7)
    for _ in range(2):
        state, _ = O.diffusion_train_step(model, state, None, img, act)
    state.opt[5] = 3.0  # a run that skipped steps
    path = str(tmp_path / "resume.pt")
    CK.save_train_state(path, state)

    O, model2, _, _ = _tiny(dev, seed=1)
    fresh = O.create_octo_train_state(model2, O.AdamW(sched, skip_nonfinite=True), seed=99)
    CK.load_train_state(path, fresh)
    assert torch.equal(fresh.opt, state.opt) and fresh.skipped_steps == 3 and fresh.step == 2
    fresh, _ = O.diffusion_train_step(model2, fresh, None, img, act)
    assert _ulps(fresh.last_lr, np.float32(sched(2))) <= 1
    assert fresh.skipped_steps == 3 and fresh.step == 3

    d = torch.load(path, map_location="cpu", weights_only=True)
    del d["opt"]  # a file written before the optimizer kept device words
    old = str(tmp_path / "old.pt")
    torch.save(d, old)
    CK.load_train_state(old, fresh)
    assert torch.equal(fresh.opt, torch.zeros_like(fresh.opt)) and fresh.step == 2
