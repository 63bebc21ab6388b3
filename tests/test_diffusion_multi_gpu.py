"""The multi-draw diffusion loss on the device: mmt_diffusion_loss_multi and mmt_diffusion_loss_dq
through the C ABI against the float64 reference of tests/diffusion_multi_ref.py with the kernel
form that ran asserted, their draws, guards and reproducibility; then
DiffusionActionHead.loss_forward_multi / loss_backward against the reference built from the head's
own parameters, and the Octo model with n_diffusion_samples and action_pad_mask.

Tolerances. The kernel's rounding model is fp32 arithmetic on exactly widened bf16 weights
(include/mmt_api.h), the sampler kernel's: its bar KTOL = 1e-4 (atol = rtol,
tests/test_sampler_steps_gpu.py) holds for loss, t_out, eps_out and every fp32 quantity; the fp32
emulation differs from float64 by < 1e-6 on these inputs (tests/test_diffusion_multi_cpu.py). The
five bf16 outputs are one rounding of such a value (bf16 keeps 8 significant bits: half a unit in
the last place is at most 2^-8 |x|): |got - want| <= tol + 2^-8 (|want| + tol) with
tol = KTOL (1 + |want|). No pre-activation of the inputs lies within 1e-4 of zero (asserted on
the CPU), so no element is excluded. Head level: the loss within HTOL = 2e-3 (the sampler tests'
head-level bar), gradients by SURVEY §8c's bf16-operand bar (relative L2 <= 5e-2, cosine >=
0.999); model level: the same §8c bars against the single-draw path."""
import functools

import numpy as np
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from oracle import rng as R
from tests import diffusion_multi_ref as MR

pytestmark = pytest.mark.gpu

KTOL = 1e-4     # kernel level, fp32-operand form
HTOL = 2e-3     # head level loss
CASE_IDS = ["H%d-A%d-B%d-S%d-K%d" % c for c in MR.KERNEL_CASES]
BWD = ("noisy", "h", "dh", "dpred", "dP")


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _dev_inputs(dev, inp):
    d = {}
    for k, v in inp.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        d[k] = t.to(dev)
    d["w1"] = d["w1"].to(torch.bfloat16)
    d["w2"] = d["w2"].to(torch.bfloat16)
    return d


def _loss(dev, d, case, *, mask=None, rng=None, inject=True, grad_scale=1.0, sample_offset=0,
          backward=True, want_eps=True, B=None, A=None, K=None, H=None, steps=None, w1=None,
          ld_w1=None):
    """One mmt_diffusion_loss_multi call on the device arrays d -> dict of outputs."""
    cH, cA, cB, cS, cK = case
    H, A, B = cH if H is None else H, cA if A is None else A, cB if B is None else B
    steps, K = cS if steps is None else steps, cK if K is None else K
    w1 = d["w1"] if w1 is None else w1
    nan = float("nan")
    o = dict(loss=torch.full((1,), nan, dtype=torch.float32, device=dev),
             t=torch.full((max(K, 1), B), -7, dtype=torch.int32, device=dev),
             eps=torch.full((max(K, 1), B, max(A, 1)), nan, dtype=torch.float32, device=dev)
             if want_eps else None)
    shapes = dict(noisy=(K * B, A), h=(K * B, H), dh=(K * B, H), dpred=(K * B, A), dP=(B, H))
    for k in BWD:
        o[k] = (torch.full([max(s, 1) for s in shapes[k]], nan, dtype=torch.bfloat16, device=dev)
                if backward else None)
    scratch = torch.empty(B + 1, dtype=torch.float32, device=dev)
    _C.call("mmt_diffusion_loss_multi", _C.ptr(rng), B, A, K, steps, H, sample_offset,
            _C.ptr(d["actions"]), _C.ptr(mask), _C.ptr(d["alpha_hats"]), _C.ptr(d["P"]),
            d["P"].stride(0), _C.ptr(d["Q"]), d["Q"].stride(0), _C.ptr(w1),
            w1.stride(0) if ld_w1 is None else ld_w1, _C.ptr(d["w2"]), _C.ptr(d["b2"]),
            _C.ptr(d["t"]) if inject else None, _C.ptr(d["eps"]) if inject else None,
            float(grad_scale), _C.ptr(scratch), _C.ptr(o["loss"]), _C.ptr(o["t"]), _C.ptr(o["eps"]),
            *(_C.ptr(o[k]) for k in BWD), _C.stream_ptr())
    return o


@functools.lru_cache(maxsize=None)
def _want(case, mask_name, grad_scale):
    w = MR.want(case, mask_name, grad_scale)
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def _close(name, got, want, bf16_rounded=False):
    want = np.asarray(want, dtype=np.float64).reshape(got.shape)
    tol = KTOL * (1.0 + np.abs(want))
    bound = tol + 2.0 ** -8 * (np.abs(want) + tol) if bf16_rounded else tol
    err = np.abs(got - want)
    print(f"{name}: max |err| {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.isfinite(got).all(), name
    assert np.all(err <= bound), f"{name}: max err / bound {np.max(err / bound):.3f}"


# ------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("mask_name", ["none", "random", "zero-row", "all-zero"])
@pytest.mark.parametrize("case", MR.KERNEL_CASES, ids=CASE_IDS)
def test_kernel_matches_reference(dev, case, mask_name):
    H, A, B, steps, K = case
    inp = MR.kernel_inputs(*case)
    d = _dev_inputs(dev, inp)
    m = MR.masks(inp)[mask_name]
    m_d = None if m is None else torch.from_numpy(m).to(dev)
    gs = float(K * B)         # dpred of the size of d itself: the 1e-4 bar bites
    _C.call("mmt_device_status", _C.stream_ptr())
    o = _loss(dev, d, case, mask=m_d, grad_scale=gs)
    route = _C.diffusion_loss_last_route()
    assert route == _C.diffusion_loss_route(A, H)
    assert (route == _C.DIFFUSION_LOSS_ROUTE_STREAM) == (H == 1024)
    assert route in (_C.DIFFUSION_LOSS_ROUTE_LDS, _C.DIFFUSION_LOSS_ROUTE_STREAM)
    fwd = _loss(dev, d, case, mask=m_d, grad_scale=gs, backward=False, want_eps=False)
    again = _loss(dev, d, case, mask=m_d, grad_scale=gs)
    torch.cuda.synchronize()
    _C.call("mmt_device_status", _C.stream_ptr())
    w = _want(case, mask_name, gs)
    assert torch.equal(o["t"], d["t"]) and torch.equal(o["eps"], d["eps"])
    _close("loss", _np(o["loss"]), w["loss"])
    for k in BWD:
        _close(k, _np(o[k]), w[k], bf16_rounded=True)
    if mask_name == "all-zero":
        assert float(o["loss"]) == 0.0
        for k in ("dh", "dpred", "dP"):
            assert not _np(o[k]).any(), k
    if mask_name == "zero-row":
        assert not _np(o["dpred"]).reshape(K, B, A)[:, 1].any() and not _np(o["dP"])[1].any()
    # forward only: the same loss bits; a second call: the same bits everywhere
    assert torch.equal(fwd["loss"], o["loss"]) and torch.equal(fwd["t"], o["t"])
    for k in ("loss", "t", "eps") + BWD:
        assert torch.equal(again[k].view(torch.int16) if again[k].dtype == torch.bfloat16
                           else again[k], o[k].view(torch.int16)
                           if o[k].dtype == torch.bfloat16 else o[k]), k


def test_graph_capture_repeats_the_eager_call(dev):
    case = MR.KERNEL_CASES[1]
    inp = MR.kernel_inputs(*case)
    d = _dev_inputs(dev, inp)
    rng = torch.tensor([5, 1], dtype=torch.int32, device=dev)
    m_d = torch.from_numpy(inp["mask"]).to(dev)
    eager = _loss(dev, d, case, mask=m_d, rng=rng, inject=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = _loss(dev, d, case, mask=m_d, rng=rng, inject=False)
    cap["loss"].fill_(float("nan"))
    cap["dP"].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k in ("loss", "t", "eps") + BWD:
        assert torch.equal(cap[k].float(), eager[k].float()), k


# ------------------------------------------------------------------------------------ draws
def test_k1_draws_are_diffusion_preps(dev):
    """At K = 1 t_out and eps_out are mmt_diffusion_prep's, bit for bit, for the same rng and
    offset."""
    case = (192, 8, 5, 7, 3)
    H, A, B, steps, _ = case
    d = _dev_inputs(dev, MR.kernel_inputs(*case))
    rng = torch.tensor([4321, 9], dtype=torch.int32, device=dev)
    o = _loss(dev, d, case, rng=rng, inject=False, K=1, sample_offset=40)
    F = 4
    t_p = torch.empty(B, dtype=torch.int32, device=dev)
    eps_p = torch.empty((B, A), dtype=torch.float32, device=dev)
    cat = torch.empty((B, A), dtype=torch.bfloat16, device=dev)
    feats = torch.empty((B, 2 * F), dtype=torch.bfloat16, device=dev)
    fw = torch.ones(F, dtype=torch.float32, device=dev)
    _C.call("mmt_diffusion_prep", _C.ptr(rng), B, A, steps, 40, _C.ptr(d["actions"]),
            _C.ptr(d["alpha_hats"]), _C.ptr(fw), F, None, None, _C.ptr(t_p), _C.ptr(eps_p),
            _C.ptr(cat), cat.stride(0), _C.ptr(feats), _C.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(o["t"][0], t_p) and torch.equal(o["eps"][0], eps_p)
    # and the noisy operand is the prep kernel's noisy sample up to one bf16 step (the two
    # kernels may contract a1 a + a2 eps differently)
    np.testing.assert_allclose(_np(o["noisy"]), _np(cat), rtol=2.0 ** -7, atol=1e-6)


def test_draw_streams(dev):
    case = (200, 24, 33, 12, 2)
    H, A, B, steps, _ = case
    K, seed, step = 5, 77, 3
    d = _dev_inputs(dev, MR.kernel_inputs(*case))
    rng = torch.tensor([seed, step], dtype=torch.int32, device=dev)
    o = _loss(dev, d, case, rng=rng, inject=False, K=K)
    t_want, eps_want = MR.draws(seed, step, B, A, steps, K)
    torch.cuda.synchronize()
    assert np.array_equal(o["t"].cpu().numpy(), t_want)                # bit for bit, every k
    np.testing.assert_allclose(_np(o["eps"]), eps_want, atol=1e-5, rtol=1e-5)
    eps = _np(o["eps"])
    for a in range(K):                                                 # pairwise different
        for b in range(a + 1, K):
            assert (eps[a] == eps[b]).mean() < 0.01
            assert not np.array_equal(t_want[a], t_want[b])
    assert 0.8 < eps.std() < 1.2
    # keyed by the global sample index: rows 2.. of the batch at offset 0 are the batch at offset 2
    s = 2
    tail = dict(d, P=d["P"][s:].contiguous(), actions=d["actions"][s:].contiguous())
    o2 = _loss(dev, tail, case, rng=rng, inject=False, K=K, B=B - s, sample_offset=s)
    torch.cuda.synchronize()
    assert torch.equal(o2["t"], o["t"][:, s:]) and torch.equal(o2["eps"], o["eps"][:, s:])
    # what was drawn, injected: the same outputs
    inj = dict(d, t=o["t"].clone(), eps=o["eps"].clone())
    o3 = _loss(dev, inj, case, K=K)
    for k in ("loss",) + BWD:
        assert torch.equal(o3[k].float(), o[k].float()), k


# ------------------------------------------------------------------------------------ guards
BAD = [dict(A=12), dict(A=0), dict(A=72), dict(H=1032), dict(H=196), dict(H=0), dict(K=0),
       dict(K=65), dict(steps=0), dict(ld_w1=20), dict(inject=False), dict(B=0), dict(w1="odd")]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
def test_unsupported_calls_are_rejected_before_a_launch(dev, bad):
    case = (192, 8, 5, 7, 3)
    d = _dev_inputs(dev, MR.kernel_inputs(*case))
    ok = _loss(dev, d, case)
    assert _C.diffusion_loss_last_route() == _C.DIFFUSION_LOSS_ROUTE_LDS
    bad = dict(bad)
    if bad.get("w1") == "odd":       # a W1 base 2 bytes off a 16-B boundary
        bad["w1"] = d["w1"].reshape(-1)[1:1 + 16 * 100].view(100, 16)
        bad["ld_w1"] = 16
    with pytest.raises(_C.MMTError):
        _loss(dev, d, case, **bad)
    assert _C.diffusion_loss_last_route() == _C.DIFFUSION_LOSS_ROUTE_NONE
    torch.cuda.synchronize()
    assert torch.isfinite(ok["loss"]).all()


def test_half_given_backward_outputs_are_rejected(dev):
    case = (192, 8, 5, 7, 3)
    H, A, B, steps, K = case
    d = _dev_inputs(dev, MR.kernel_inputs(*case))
    buf = torch.empty(K * B * H, dtype=torch.bfloat16, device=dev)
    scratch = torch.empty(B + 1, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    t = torch.empty((K, B), dtype=torch.int32, device=dev)
    with pytest.raises(_C.MMTError):
        _C.call("mmt_diffusion_loss_multi", None, B, A, K, steps, H, 0, _C.ptr(d["actions"]), None,
                _C.ptr(d["alpha_hats"]), _C.ptr(d["P"]), H, _C.ptr(d["Q"]), H, _C.ptr(d["w1"]),
                d["w1"].stride(0), _C.ptr(d["w2"]), _C.ptr(d["b2"]), _C.ptr(d["t"]),
                _C.ptr(d["eps"]), 1.0, _C.ptr(scratch), _C.ptr(loss), _C.ptr(t), None,
                _C.ptr(buf), _C.ptr(buf), None, None, None, _C.stream_ptr())
    assert _C.diffusion_loss_last_route() == _C.DIFFUSION_LOSS_ROUTE_NONE


def test_out_of_range_t_is_reported_not_followed(dev):
    case = (192, 8, 5, 7, 3)
    H, A, B, steps, K = case
    inp = MR.kernel_inputs(*case)
    d = _dev_inputs(dev, inp)
    bad = inp["t"].copy()
    bad[0, 1], bad[2, 4] = steps, -1
    _C.call("mmt_device_status", _C.stream_ptr())
    got = _loss(dev, dict(d, t=torch.from_numpy(bad).to(dev)), case)
    with pytest.raises(_C.MMTError):
        _C.call("mmt_device_status", _C.stream_ptr())
    _C.call("mmt_device_status", _C.stream_ptr())     # the report cleared the word
    bad[0, 1] = bad[2, 4] = 0
    want = _loss(dev, dict(d, t=torch.from_numpy(bad).to(dev)), case)
    torch.cuda.synchronize()
    assert np.array_equal(got["t"].cpu().numpy(), bad)
    for k in ("loss",) + BWD:
        assert torch.isfinite(got[k].float()).all() and torch.equal(got[k].float(), want[k].float()), k


# ------------------------------------------------------------------------------------ dQ
@pytest.mark.parametrize("rows,steps,H,ld", [(15, 7, 192, 192), (66, 12, 200, 208), (72, 9, 72, 72),
                                             (2500, 5, 64, 64)])   # past two 1024-row tiles
def test_dq_segment_sum(dev, rows, steps, H, ld):
    g = np.random.default_rng(rows + H)
    dh = MR.bf16(g.standard_normal((rows, ld)))
    t = g.integers(0, steps - 1, size=rows).astype(np.int32)    # step steps - 1: no row
    dh_d = torch.from_numpy(dh.astype(np.float32)).to(dev).to(torch.bfloat16)
    t_d = torch.from_numpy(t).to(dev)
    outs = []
    for _ in range(2):
        dq = torch.full((steps, ld), float("nan"), dtype=torch.float32, device=dev)
        _C.call("mmt_diffusion_loss_dq", _C.ptr(t_d), _C.ptr(dh_d), ld, rows, steps, H, _C.ptr(dq),
                ld, _C.stream_ptr())
        outs.append(dq)
    torch.cuda.synchronize()
    got = _np(outs[0])[:, :H]
    want = MR.segment_sum(t, dh[:, :H], steps)
    counts = np.bincount(t, minlength=steps)[:, None]
    err = np.abs(got - want)
    print(f"max |err| {err.max():.3e}")
    assert np.all(err <= 1e-4 * np.maximum(counts, 1))
    assert not got[steps - 1].any() and counts[steps - 1, 0] == 0
    assert torch.equal(outs[0][:, :H], outs[1][:, :H])
    assert torch.isnan(outs[0][:, H:]).all()                    # nothing past the H columns
    with pytest.raises(_C.MMTError):
        _C.call("mmt_diffusion_loss_dq", _C.ptr(t_d), _C.ptr(dh_d), H - 8, rows, steps, H,
                _C.ptr(outs[0]), ld, _C.stream_ptr())


# ------------------------------------------------------------------------------------ head
HD, HA, HH, HS, HB, HK = 64, 16, 72, 6, 5, 3


def _head(dev, seed=3, **kw):
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    store = ParamStore()
    head = DiffusionActionHead.create(store, "diffusion_action_head", HD, HA, HS, hidden=HH, **kw)
    store.materialize(dev, seed=seed)
    return head, store


def _head_params(head):
    return dict(fourier=_np(head.fourier.data).reshape(-1), t1w=_np(head.t1.w.bf16),
                t1b=_np(head.t1.b.data), t2w=_np(head.t2.w.bf16), t2b=_np(head.t2.b.data),
                w1=_np(head.d1.w.bf16), b1=_np(head.d1.b.data), w2=_np(head.d2.w.bf16),
                b2=_np(head.d2.b.data))


def _head_grads(head):
    return dict(fourier=_np(head.fourier.grad).reshape(-1), t1w=_np(head.t1.w.grad),
                t1b=_np(head.t1.b.grad), t2w=_np(head.t2.w.grad), t2b=_np(head.t2.b.grad),
                w1=_np(head.d1.w.grad), b1=_np(head.d1.b.grad), w2=_np(head.d2.w.grad),
                b2=_np(head.d2.b.grad))


def _head_inputs(dev, seed=0):
    g = np.random.default_rng(seed)
    e = MR.bf16(0.5 * g.standard_normal((HB, HD)))
    actions = g.standard_normal((HB, HA)).astype(np.float32)
    t = g.integers(0, HS, size=(HK, HB)).astype(np.int32)
    eps = g.standard_normal((HK, HB, HA)).astype(np.float32)
    mask = g.random((HB, HA)) < 0.7
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(e=e, actions=actions, t=t, eps=eps, mask=mask), dict(
        e=to(e.astype(np.float32)).to(torch.bfloat16), actions=to(actions), t=to(t), eps=to(eps),
        mask=to(mask))


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_head_gradients_match_reference(dev, masked):
    """Every head parameter gradient and d(pooled readout) against the float64 reference built
    from the head's own parameters (the bf16 shadows its GEMMs read). The device rounds the time
    embedding and the GEMM operands dQ, dP to bf16; the L2 metrics are the bar for
    that. The smallest reference |pre| is printed."""
    head, store = _head(dev)
    n, d = _head_inputs(dev)
    store.zero_grad()
    loss, sv = head.loss_forward_multi(d["e"], d["actions"], None, 0, HK,
                                       d["mask"] if masked else None, d["t"], d["eps"])
    assert _C.diffusion_loss_last_route() == _C.DIFFUSION_LOSS_ROUTE_LDS
    de = head.loss_backward(sv)
    torch.cuda.synchronize()
    _C.call("mmt_device_status", _C.stream_ptr())
    w = MR.head_grads(_head_params(head), n["e"], n["actions"], n["mask"] if masked else None,
                      head.alpha_hats_np, n["t"], n["eps"], HA)
    print(f"loss {float(loss):.6f} vs {w['loss']:.6f}; min |pre| {np.abs(w['pre']).min():.3e}")
    np.testing.assert_allclose(float(loss), w["loss"], atol=HTOL, rtol=HTOL)
    got = dict(_head_grads(head), de=_np(de))
    assert de.shape == (HB, HD) and de.dtype == torch.bfloat16
    for k, g in got.items():
        ref = np.asarray(w[k]).reshape(g.shape)
        rel = np.linalg.norm(g - ref) / np.linalg.norm(ref)
        cos = float((g * ref).sum() / (np.linalg.norm(g) * np.linalg.norm(ref)))
        print(f"{k}: relative L2 {rel:.3e}, cosine {cos:.6f}")
        assert rel <= 5e-2 and cos >= 0.999, (k, rel, cos)


def test_head_k1_through_the_multi_path(dev):
    """K = 1 through loss_forward_multi: the draws are the single-draw path's (same rng and
    offset), and the loss agrees with it within the head-level bar (that path rounds cat and the
    hidden layer to bf16, this one does not: the looser 2e-2 relative §8c bar)."""
    head, _ = _head(dev)
    _, d = _head_inputs(dev)
    rng = torch.tensor([99, 3], dtype=torch.int32, device=dev)
    cat = head.new_cat(HB, dev)
    head.readout_slot(cat).copy_(d["e"])
    l_old, sv_old = head.loss_forward(cat, d["actions"], rng, 11)
    l_new, sv_new = head.loss_forward_multi(d["e"], d["actions"], rng, 11, 1)
    torch.cuda.synchronize()
    assert torch.equal(sv_new["t"][0], sv_old["t"]) and torch.equal(sv_new["eps"][0], sv_old["eps"])
    np.testing.assert_allclose(float(l_new), float(l_old), rtol=2e-2)


# float32 bits of denoise_loss on this test's inputs (head seed 3, D 64, A 16, hidden 72, 6 steps;
# readouts (5, 4, 64) and actions (5, 16) from torch.Generator seed 0; rng (7, 0), offset 0),
# recorded once on an MI355X from a checkout of the commit before the multi-draw loss: 21.204159
PARENT_LOSS_BITS = 0x41A9A21E


def test_head_option_guards_and_default_path(dev, monkeypatch):
    """num_blocks = 2 with either option is a ValueError; K = 1 without a mask through
    denoise_loss issues the single-draw launches and reproduces the loss bits that path gave
    before this entry existed (PARENT_LOSS_BITS); a mask or K > 1 takes the new entry."""
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    with pytest.raises(ValueError):      # num_blocks = 2 with K = 2
        DiffusionActionHead.create(ParamStore(), "h", HD, HA, HS, num_blocks=2,
                                   n_diffusion_samples=2)
    two, _ = _head(dev, num_blocks=2)
    g = torch.Generator().manual_seed(0)
    readouts = torch.randn((HB, 4, HD), generator=g).to(dev)
    actions = torch.randn((HB, HA), generator=g).to(dev)
    rng = torch.tensor([7, 0], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):      # a mask on a two-block denoiser
        two.denoise_loss(readouts, actions, rng=rng,
                         pad_mask=torch.ones((HB, HA), dtype=torch.bool, device=dev))
    # K = 1 without a mask through denoise_loss issues mmt_diffusion_prep and mmt_diffusion_loss
    # and never the new entry; with a mask or K > 1 it is the new entry
    head, _ = _head(dev)
    names = []
    real = _C.call
    monkeypatch.setattr(_C, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    l1 = head.denoise_loss(readouts, actions, rng=rng)
    assert "mmt_diffusion_prep" in names and "mmt_diffusion_loss" in names
    assert "mmt_diffusion_loss_multi" not in names
    assert l1.view(torch.int32).item() == PARENT_LOSS_BITS, hex(l1.view(torch.int32).item())
    names.clear()
    ones = torch.ones((HB, HA), dtype=torch.bool, device=dev)
    l2 = head.denoise_loss(readouts, actions, rng=rng, pad_mask=ones)
    assert "mmt_diffusion_loss_multi" in names and "mmt_diffusion_prep" in names   # the time table
    assert "mmt_diffusion_loss" not in names
    k4, _ = _head(dev, n_diffusion_samples=4)
    names.clear()
    l3 = k4.denoise_loss(readouts, actions, rng=rng)
    assert "mmt_diffusion_loss_multi" in names and "mmt_diffusion_loss" not in names
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(l2), float(l1), rtol=2e-2)    # all-ones mask, same draws
    assert np.isfinite(float(l3)) and float(l3) != float(l2)


# ------------------------------------------------------------------------------------ model
def _model(dev, **kw):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    cfg = get_config("octo-tiny", **kw)
    return O.Octo(cfg, dev, seed=0), cfg, O


def _batch(dev, model, cfg, B=4):
    g = torch.Generator().manual_seed(0)
    S = cfg.image_size[0]
    images = torch.randint(0, 256, (B, model.n_images, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    actions = torch.randn((B, cfg.action_horizon, cfg.action_space_dim), generator=g).to(dev)
    return images, actions


def test_model_repeated_draws_match_the_single_draw_step(dev):
    """K = 4 with the same injected (t, eps) in every draw against the existing single-draw step
    with that (t, eps): the §8c bf16 bars (the old path rounds cat and the hidden layer to bf16)."""
    B, K = 4, 4
    m1, cfg1, O = _model(dev, action_horizon=2)
    mK, cfgK, _ = _model(dev, action_horizon=2, n_diffusion_samples=K)
    assert mK.head.n_diffusion_samples == K and m1.head.n_diffusion_samples == 1
    assert torch.equal(m1.store.flat, mK.store.flat)          # the option moves no parameter
    images, actions = _batch(dev, m1, cfg1, B)
    A = m1.head.A
    g = torch.Generator().manual_seed(1)
    t = torch.randint(0, cfg1.diffusion_steps, (B,), generator=g, dtype=torch.int32).to(dev)
    eps = torch.randn((B, A), generator=g).to(dev)
    rng = torch.tensor([11, 0], dtype=torch.int32, device=dev)
    outs = []
    for m, inj in ((m1, dict(t=t, eps=eps)),
                   (mK, dict(t=t[None].repeat(K, 1).contiguous(),
                             eps=eps[None].repeat(K, 1, 1).contiguous()))):
        m.store.zero_grad()
        loss, st = m.compute_diffusion_denoise_loss(None, images, actions, True, rng, inject=inj)
        m.backward(st)
        torch.cuda.synchronize()
        outs.append((float(loss), _np(m.store.flat_grad)))
    (l1, g1), (lK, gK) = outs
    cos = float((g1 * gK).sum() / (np.linalg.norm(g1) * np.linalg.norm(gK)))
    print(f"loss {l1:.6f} vs {lK:.6f}, flat-gradient cosine {cos:.6f}")
    np.testing.assert_allclose(lK, l1, rtol=2e-2)
    assert cos >= 0.999, cos
    _C.call("mmt_device_status", _C.stream_ptr())


def test_model_pad_mask_and_train_step(dev):
    B = 4
    m, cfg, O = _model(dev, action_horizon=2, n_diffusion_samples=3)
    images, actions = _batch(dev, m, cfg, B)
    a = cfg.action_space_dim
    mask = torch.ones((B, 2, a), dtype=torch.bool, device=dev)
    mask[:, 1] = False                                        # the last chunk step is padding
    rng = torch.tensor([11, 0], dtype=torch.int32, device=dev)
    m.store.zero_grad()
    loss, st = m.compute_diffusion_denoise_loss(None, images, actions, True, rng,
                                                action_pad_mask=mask)
    m.backward(st)
    torch.cuda.synchronize()
    b2g = m.head.d2.b.grad
    assert torch.isfinite(loss).all() and float(b2g[:a].abs().sum()) > 0
    assert not b2g[a:].any()                                  # exactly zero
    assert not m.head.d2.w.grad[a:].any()
    flat = m.compute_diffusion_denoise_loss(None, images, actions, True, rng,
                                            action_pad_mask=mask.reshape(B, 2 * a))[0]
    assert torch.equal(flat, loss)
    for bad in (mask[:, :1], mask.float(), mask[:2]):
        with pytest.raises(ValueError):
            m.compute_diffusion_denoise_loss(None, images, actions, True, rng, action_pad_mask=bad)
    state = O.create_octo_train_state(m, seed=7)
    state, grads = O.diffusion_train_step(m, state, None, images, actions, action_pad_mask=mask)
    assert state.step == 1 and np.isfinite(float(state.last_loss))
    assert float(sum(g.abs().sum() for g in grads.values())) > 0
    _C.call("mmt_device_status", _C.stream_ptr())


def test_ddp_step_captures_with_the_option(dev):
    """The one-graph training step with K = 3: captured and replayed once, it repeats the eager
    step (deterministic mode: the multi-draw head itself has no atomics)."""
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    B = 4
    m, cfg, O = _model(dev, action_horizon=2, n_diffusion_samples=3)
    images, actions = _batch(dev, m, cfg, B)
    act = actions.reshape(B, -1).contiguous()
    state = O.create_octo_train_state(m, seed=7)
    st = m.store
    kept = (st.flat, st.flat_bf16, st.m, st.v, state.rng)
    start = [t.clone() for t in kept]
    try:
        st.set_deterministic(True)
        state, _ = O.diffusion_train_step(m, state, None, images, act)
        torch.cuda.synchronize()
        eager_loss, eager_flat = state.last_loss.clone(), st.flat.clone()
        for d, v in zip(kept, start):
            d.copy_(v)
        st.refresh_transposed()
        st.refresh_fp8()
        step = DDPStep(m, state, None, images, act, None, use_graph=True).build()
        assert len(step.graphs) == 1
        step()
        torch.cuda.synchronize()
        assert np.isfinite(float(eager_loss)) and float(eager_loss) > 0
        assert torch.equal(step.loss_buf.view(-1), eager_loss.view(-1))
        assert torch.equal(st.flat, eager_flat)
    finally:
        st.set_deterministic(False)
    _C.call("mmt_device_status", _C.stream_ptr())
