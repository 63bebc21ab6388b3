"""The step-table sampler (mmt_diffusion_sample_steps, csrc/sampler.hip) on the device: the kernel
through the C ABI against the float64 reference of tests/sampler_steps_ref.py with the kernel form
that ran asserted, its draws and reproducibility, then DiffusionActionHead's samplers (fresh-noise
DDPM, DDIM, frozen DDPM at widths other than 8) and the Octo model with an action horizon.

Tolerances. The kernel's rounding model is fp32 operands throughout (include/mmt_api.h), so the
kernel level uses atol = rtol = 1e-4 against the float64 reference (its fp32 emulation differs
from it by <= 2.2e-6 on these inputs, tests/test_sampler_steps_cpu.py; the margin covers the
reduction order) and the head level the project's fp32-form bar 2e-3 (tests/test_sampler_gpu.py:
there P and Q come from the bf16 GEMMs)."""
import functools

import numpy as np
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from oracle import rng as R
from tests import sampler_steps_ref as SR

pytestmark = pytest.mark.gpu

KTOL = 1e-4     # kernel level, fp32-operand form
HTOL = 2e-3     # head level, fp32-operand form


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _dev_inputs(dev, inp):
    d = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
         for k, v in inp.items()}
    d["w1"] = d["w1"].to(torch.bfloat16)
    d["w2"] = d["w2"].to(torch.bfloat16)
    return d


def _steps(dev, d, A, H, t, coef, clip, *, rng=None, z_in=None, noise_in=None, fresh=False,
           sample_offset=0, B=None, want_z=False, want_noise=False):
    """One mmt_diffusion_sample_steps call on the device arrays d -> (actions, z_out, noise_out)."""
    B = d["P"].shape[0] if B is None else B
    K = t.shape[0]
    actions = torch.full((B, A), float("nan"), dtype=torch.float32, device=dev)
    z_out = torch.empty((B, A), dtype=torch.float32, device=dev) if want_z else None
    n_out = torch.empty((K, B, A), dtype=torch.float32, device=dev) if want_noise else None
    _C.call("mmt_diffusion_sample_steps", _C.ptr(rng), B, A, K, sample_offset, _C.ptr(d["P"]),
            d["P"].stride(0), _C.ptr(d["Q"]), d["Q"].stride(0), d["Q"].shape[0], _C.ptr(d["w1"]),
            d["w1"].stride(0), _C.ptr(d["w2"]), _C.ptr(d["b2"]), _C.ptr(t), _C.ptr(coef),
            float(clip), _C.SAMPLE_FRESH_NOISE if fresh else 0, _C.ptr(z_in), _C.ptr(noise_in), H,
            _C.ptr(actions), _C.ptr(z_out), _C.ptr(n_out), _C.stream_ptr())
    return actions, z_out, n_out


@functools.lru_cache(maxsize=None)
def _kernel_want(case, fresh, clip, K):
    H, A, B, q_rows = case
    inp = SR.kernel_inputs(H, A, B, q_rows)
    t, coef = SR.kernel_table(q_rows, K)
    want = SR.run_steps(inp["P"], inp["Q"], inp["w1"][:, :A], inp["w2"], inp["b2"], t, coef, clip,
                        inp["z"], inp["noise"][:K] if fresh else None)
    want.setflags(write=False)
    return want


def _check(got, want, clip, tol, cap):
    sat = SR.saturated(want, clip)
    assert sat.mean() <= cap, f"{sat.mean():.3f} of the reference outputs sit at +-{clip}"
    assert np.isfinite(got).all() and np.all(np.abs(got) <= clip)
    assert np.array_equal(np.sign(got[sat]), np.sign(want[sat]))
    err = np.abs(got - want)
    print(f"max |err| {err.max():.3e}, saturated {sat.mean():.3f}")
    np.testing.assert_allclose(got, want, atol=tol, rtol=tol)


@pytest.mark.parametrize("clip", [5.0, 0.75])
@pytest.mark.parametrize("fresh", [False, True], ids=["frozen", "fresh"])
@pytest.mark.parametrize("case", SR.KERNEL_CASES, ids=lambda c: "H%d-A%d-B%d-q%d" % c)
def test_kernel_matches_reference(dev, case, fresh, clip):
    H, A, B, q_rows = case
    d = _dev_inputs(dev, SR.kernel_inputs(H, A, B, q_rows))
    for K in (SR.KERNEL_K, 1):
        t, coef = SR.kernel_table(q_rows, K)
        actions, _, _ = _steps(dev, d, A, H, torch.from_numpy(t).to(dev),
                               torch.from_numpy(coef).to(dev), clip, z_in=d["z"],
                               noise_in=d["noise"][:K].contiguous() if fresh else None, fresh=fresh)
        assert _C.sampler_last_route() == _C.sampler_steps_route(A, H)
        torch.cuda.synchronize()
        cap = SR.SATURATION_CAP[clip] if K == SR.KERNEL_K else 1.0
        _check(_np(actions), _kernel_want(case, fresh, clip, K), clip, KTOL, cap)
    # the table's forms: the last case streams its 256 KB of weights, the others keep them in LDS
    assert (_C.sampler_steps_route(A, H) == _C.SAMPLER_ROUTE_STEPS_STREAM) == (case[0] == 1024)
    _C.call("mmt_device_status", _C.stream_ptr())


# ------------------------------------------------------------------------------------ draws
def _draw_case(dev, A=8, H=192, B=21, q_rows=6):
    return _dev_inputs(dev, SR.kernel_inputs(H, A, B, q_rows)), A, H, B, q_rows


def test_z_draw_equals_legacy_kernel(dev):
    """At A = 8 the drawn z is mmt_diffusion_sample's, bit for bit."""
    d, A, H, B, q_rows = _draw_case(dev)
    t, coef = (torch.from_numpy(v).to(dev) for v in SR.kernel_table(q_rows, 3))
    rng = torch.tensor([4321, 9], dtype=torch.int32, device=dev)
    _, z_new, _ = _steps(dev, d, A, H, t, coef, 5.0, rng=rng, sample_offset=40, want_z=True)
    z_old = torch.empty((B, A), dtype=torch.float32, device=dev)
    scratch = torch.empty((B, A), dtype=torch.float32, device=dev)
    legacy_coef = torch.ones((1, 3), dtype=torch.float32, device=dev)
    _C.call("mmt_diffusion_sample", _C.ptr(rng), B, A, 1, 40, _C.ptr(d["P"]), d["P"].stride(0),
            _C.ptr(d["Q"]), d["Q"].stride(0), _C.ptr(d["w1"]), d["w1"].stride(0), _C.ptr(d["w2"]),
            _C.ptr(d["b2"]), _C.ptr(legacy_coef), None, H, _C.ptr(scratch), _C.ptr(z_old),
            _C.stream_ptr())
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_LEGACY_WAVE
    torch.cuda.synchronize()
    assert torch.equal(z_new, z_old)
    assert 0.5 < float(z_new.std()) < 1.5


@pytest.mark.parametrize("A,H", [(8, 192), (24, 200)])
def test_draws_feed_back_shift_and_repeat(dev, A, H):
    d, A, H, B, q_rows = _draw_case(dev, A, H)
    K = 5
    t, coef = (torch.from_numpy(v).to(dev) for v in SR.kernel_table(q_rows, K))
    rng = torch.tensor([77, 3], dtype=torch.int32, device=dev)
    kw = dict(rng=rng, fresh=True, want_z=True, want_noise=True)
    a1, z1, n1 = _steps(dev, d, A, H, t, coef, 5.0, **kw)
    a2, z2, n2 = _steps(dev, d, A, H, t, coef, 5.0, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and torch.equal(z1, z2) and torch.equal(n1, n2)
    assert torch.isfinite(n1).all() and torch.isfinite(z1).all() and torch.isfinite(a1).all()
    for k in range(1, K):      # a stream per step, and none of them z's
        assert not torch.equal(n1[k], n1[k - 1])
    assert not torch.equal(n1[0], z1)
    assert 0.7 < float(n1.std()) < 1.3
    # what was drawn, injected: the same run
    a3, _, _ = _steps(dev, d, A, H, t, coef, 5.0, z_in=z1.clone(), noise_in=n1.clone(), fresh=True)
    assert torch.equal(a3, a1)
    # streams are keyed by the global sample index: a shifted batch is the tail of the full one
    s = 6
    tail = dict(d, P=d["P"][s:].contiguous())
    a4, z4, n4 = _steps(dev, tail, A, H, t, coef, 5.0, sample_offset=s, **kw)
    assert torch.equal(z4, z1[s:]) and torch.equal(n4, n1[:, s:]) and torch.equal(a4, a1[s:])
    # frozen noise differs from fresh noise, and is reproducible too
    f1, _, _ = _steps(dev, d, A, H, t, coef, 5.0, rng=rng)
    f2, _, _ = _steps(dev, d, A, H, t, coef, 5.0, z_in=z1.clone())
    assert torch.equal(f1, f2) and not torch.equal(f1, a1)


def test_step_noise_streams_over_a_long_table(dev):
    """n_steps past 256 (the entry takes up to 1024): every step's drawn noise is a stream of its
    own. stream_key keeps 8 bits of its site, so a key made from 16 + k alone would repeat after
    256 steps and hand step 243 z's own stream. The rows are also pinned to the documented keys
    (float64 Box-Muller on the oracle's counter streams; the device's logf / cosf differ by ulps),
    and the draws-only launch returns the same bits as the sampling call."""
    d, A, H, B, q_rows = _draw_case(dev, B=3)
    K, off = 520, 11
    t = torch.from_numpy(np.arange(K, dtype=np.int32) % q_rows).to(dev)
    coef = torch.from_numpy(np.tile(np.float32([0.99, -0.01, 0.05]), (K, 1))).to(dev)
    rng = torch.tensor([77, 3], dtype=torch.int32, device=dev)
    a, z, n = _steps(dev, d, A, H, t, coef, 5.0, rng=rng, fresh=True, sample_offset=off,
                     want_z=True, want_noise=True)
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_STEPS_LDS
    z_d = torch.empty_like(z)
    n_d = torch.empty_like(n)
    _C.call("mmt_diffusion_sample_steps", _C.ptr(rng), B, A, K, off, None, 0, None, 0, 0, None, 0,
            None, None, None, None, 0.0, _C.SAMPLE_FRESH_NOISE | _C.SAMPLE_DRAWS_ONLY, None, None,
            0, None, _C.ptr(z_d), _C.ptr(n_d), _C.stream_ptr())
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_STEPS_DRAWS
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(z_d, z) and torch.equal(n_d, n)
    rows = np.concatenate([_np(z)[None], _np(n)]).reshape(K + 1, -1)
    assert len({r.tobytes() for r in rows}) == K + 1          # z and the K steps: all different
    assert not np.array_equal(rows[1 + 243], rows[0]) and not np.array_equal(rows[1], rows[1 + 256])
    # no two rows share even one (sample, component) draw beyond chance: 24-bit uniforms
    assert (rows[1:257] == rows[257:513]).mean() < 0.01
    np.testing.assert_allclose(_np(z), SR.normal_draws(R.stream_key(77, 3, 0xFFFE, 3), B, A, off),
                               atol=1e-5, rtol=1e-5)
    for k in (0, 239, 240, 243, 256, 479, 480, 519):
        np.testing.assert_allclose(_np(n[k]), SR.normal_draws(SR.step_noise_key(77, 3, k), B, A, off),
                                   atol=1e-5, rtol=1e-5, err_msg=f"step {k}")


def test_call_is_graph_capturable(dev):
    """Captured into a graph and replayed, the call repeats the eager run bit for bit (it
    allocates nothing and synchronises nothing)."""
    d, A, H, B, q_rows = _draw_case(dev, 24, 200)
    t, coef = (torch.from_numpy(v).to(dev) for v in SR.kernel_table(q_rows, 5))
    rng = torch.tensor([5, 1], dtype=torch.int32, device=dev)
    kw = dict(rng=rng, fresh=True, want_z=True, want_noise=True)
    eager = _steps(dev, d, A, H, t, coef, 5.0, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _steps(dev, d, A, H, t, coef, 5.0, **kw)
    for _ in range(2):
        for out in captured:
            out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))


def test_out_of_range_step_is_reported_not_followed(dev):
    d, A, H, B, q_rows = _draw_case(dev)
    t_np, coef_np = SR.kernel_table(q_rows, 4)
    bad = t_np.copy()
    bad[1], bad[3] = q_rows, -1
    coef = torch.from_numpy(coef_np).to(dev)
    _C.call("mmt_device_status", _C.stream_ptr())
    got, _, _ = _steps(dev, d, A, H, torch.from_numpy(bad).to(dev), coef, 5.0, z_in=d["z"])
    with pytest.raises(_C.MMTError):
        _C.call("mmt_device_status", _C.stream_ptr())
    _C.call("mmt_device_status", _C.stream_ptr())     # the report cleared the word
    # the bad rows were replaced by row 0
    bad[1] = bad[3] = 0
    want, _, _ = _steps(dev, d, A, H, torch.from_numpy(bad).to(dev), coef, 5.0, z_in=d["z"])
    assert torch.isfinite(got).all() and torch.equal(got, want)


# ------------------------------------------------------------------------------------ head
def _head(dev, D, A, seed, **kw):
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    store = ParamStore()
    head = DiffusionActionHead.create(store, "diffusion_action_head", D, A, 32, **kw)
    store.materialize(dev, seed=seed)
    return head


def _readout(dev, B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, D), generator=g) * 0.5).to(torch.bfloat16).to(dev)


def _spec_and_table(head, mode):
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import SamplerSpec
    if mode == "fresh":
        return SamplerSpec(noise="fresh"), SR.ddpm_table(head.betas_np, head.alpha_hats_np, False)
    if mode == "ddim8":
        return SamplerSpec("ddim", 8), SR.ddim_table(head.alpha_hats_np, 8)
    return SamplerSpec(), SR.ddpm_table(head.betas_np, head.alpha_hats_np, True)


def _head_want(head, readout, temb, z, noise, table, A, **kw):
    P, Q, w1x = SR.split_first_dense(_np(readout), _np(temb), _np(head.d1.w.bf16),
                                     _np(head.d1.b.data), A)
    return SR.run_steps(P, Q, w1x, _np(head.d2.w.bf16), _np(head.d2.b.data), table[0], table[1],
                        5.0, _np(z), None if noise is None else _np(noise), **kw)


# (D, A, B, mode, head seed): the seeds were picked on the CPU (the oracle's time embedding and
# a restatement of the draws) for the share of reference outputs inside the clip
HEAD_CASES = [(384, 32, 6, "fresh", 23), (384, 16, 33, "fresh", 5), (192, 32, 33, "fresh", 1),
              (384, 32, 33, "ddim8", 3), (192, 16, 33, "ddim8", 6), (384, 16, 33, "frozen", 5)]


@pytest.mark.parametrize("D,A,B,mode,seed", HEAD_CASES,
                         ids=["D%d-A%d-B%d-%s" % c[:4] for c in HEAD_CASES])
def test_head_matches_reference(dev, D, A, B, mode, seed):
    """predict_action_mean with a sampler spec against the float64 reference of the table update,
    given the device's time embedding, z and step noise. The fused kernel is the fp32-operand
    form: the project's 2e-3 bar (tests/test_sampler_gpu.py), every element."""
    head = _head(dev, D, A, seed)
    readout = _readout(dev, B, D, D + B + A)
    rng = torch.tensor([1234, 7], dtype=torch.int32, device=dev)
    spec, table = _spec_and_table(head, mode)
    out = head.predict_action_mean(readout, rng, sample_offset=100, return_noise=True, sampler=spec)
    assert _C.sampler_last_route() == _C.sampler_steps_route(A, D)
    temb = head.time_embeddings(dev)
    torch.cuda.synchronize()
    assert len(out) == (3 if mode == "fresh" else 2)
    actions, z = out[0], out[1]
    noise = out[2] if mode == "fresh" else None
    assert actions.shape == (B, A) and z.shape == (B, A)
    K = len(table[0])
    assert noise is None or noise.shape == (K, B, A)
    t_head, coef_head = head.sampler_table(spec)
    assert np.array_equal(t_head, table[0]) and np.array_equal(coef_head, table[1])
    want = _head_want(head, readout, temb, z, noise, table, A)
    sat = SR.saturated(want, 5.0)
    print(f"inside the clip {(~sat).sum()} of {sat.size}, saturated {sat.mean():.2f}")
    assert (~sat).sum() >= 100 and sat.mean() <= 0.80
    got = _np(actions)
    assert np.all(np.abs(got) <= 5.0)
    print(f"max |err| {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, atol=HTOL, rtol=HTOL)
    # the same draws injected: the same actions
    again = head.predict_action_mean(readout, None, z=z.clone(), sampler=spec,
                                     noise=None if noise is None else noise.clone())
    assert torch.equal(again, actions)


def test_default_call_at_width_8_is_the_legacy_kernel(dev):
    head = _head(dev, 384, 8, 3)
    B = 17
    readout = _readout(dev, B, 384, 11)
    rng = torch.tensor([99, 3], dtype=torch.int32, device=dev)
    a1, z1 = head.predict_action_mean(readout, rng, sample_offset=5, return_noise=True)
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_LEGACY_WAVE
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import SamplerSpec
    a2 = head.predict_action_mean(readout, rng, sample_offset=5, sampler=SamplerSpec(steps=32))
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_LEGACY_WAVE
    P, Q = head._split_first_dense(readout)
    w1 = head.d1.w.bf16
    a3 = torch.empty((B, 8), dtype=torch.float32, device=dev)
    z3 = torch.empty((B, 8), dtype=torch.float32, device=dev)
    _C.call("mmt_diffusion_sample", _C.ptr(rng), B, 8, 32, 5, _C.ptr(P), P.stride(0), _C.ptr(Q),
            Q.stride(0), _C.ptr(w1), w1.stride(0), _C.ptr(head.d2.w.bf16), _C.ptr(head.d2.b.data),
            _C.ptr(head.sampler_coef(dev)), None, head.hidden, _C.ptr(a3), _C.ptr(z3),
            _C.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(a1, a3) and torch.equal(z1, z3) and torch.equal(a2, a3)
    # anything but the reference's sampler leaves the legacy kernel, at width 8 too
    b1 = head.predict_action_mean(readout, rng, sample_offset=5, sampler={"noise": "fresh"})
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_STEPS_LDS
    assert not torch.equal(b1, a1)
    # and the step-table kernel on the reference's table agrees with the legacy kernel's
    # c1 (x - c2 eps) + c3 z up to the recombined coefficients' rounding
    frozen, _, _ = head._sample_steps(readout, None, 5, z1, None, SamplerSpec())
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_STEPS_LDS
    np.testing.assert_allclose(_np(frozen), _np(a1), atol=HTOL, rtol=HTOL)


def test_head_rejects_bad_sampler_calls(dev):
    head = _head(dev, 192, 16, 1)
    readout = _readout(dev, 4, 192, 0)
    rng = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    z = torch.zeros((4, 16), device=dev)
    for kw in (dict(sampler={"kind": "ddim", "steps": 33}), dict(sampler={"steps": 8}),
               dict(sampler={"kind": "euler"}),
               dict(noise=torch.zeros((31, 4, 16), device=dev)),           # K = 32
               dict(noise=torch.zeros((32, 4, 8), device=dev)),
               dict(noise=torch.zeros((32, 4, 16), dtype=torch.float64, device=dev)),
               dict(noise=torch.zeros((8, 4, 16), device=dev), sampler={"kind": "ddim", "steps": 8})):
        with pytest.raises(ValueError):
            head.predict_action_mean(readout, rng, z=z, **kw)
    with pytest.raises(ValueError):      # fresh noise needs rng or the noise
        head.predict_action_mean(readout, None, z=z, sampler={"noise": "fresh"})
    # num_blocks > 1 takes the loop form, whose draws need the same widths: a ValueError too
    wide = _head(dev, 192, 72, 1, num_blocks=2)
    with pytest.raises(ValueError):
        wide.predict_action_mean(readout, rng)
    ok = head.predict_action_mean(readout, None, z=z, noise=torch.zeros((32, 4, 16), device=dev))
    assert ok.shape == (4, 16) and torch.isfinite(ok).all()


@pytest.mark.parametrize("mode", ["fresh", "ddim8"])
def test_loop_form_walks_the_same_table(dev, mode):
    """The per-step launch form (OctoDenoise num_blocks > 1 takes it) forced at num_blocks = 1 on
    the same spec: it consumes the fused entry's draws, matches the reference with x and the
    hidden layer rounded to bf16 where it stores them (the loop form's 5e-3 bar), and the fused
    form within the bf16 storage difference (the existing 2e-2 relative bar). Head seed picked on
    the CPU: DDPM from a random head is chaotic where a clip or a relu flips."""
    D, A, B = 384, 16, 9
    head = _head(dev, D, A, 18)
    readout = _readout(dev, B, D, 5)
    rng = torch.tensor([77, 2], dtype=torch.int32, device=dev)
    spec, table = _spec_and_table(head, mode)
    out = head.predict_action_mean(readout, rng, sample_offset=3, return_noise=True, sampler=spec)
    fused, z = out[0], out[1]
    noise = out[2] if mode == "fresh" else None
    lout = head._predict_action_loop(readout, rng, 3, None, True, spec=spec)
    z_only, n_only = head._sample_draws(B, dev, rng, 3, len(table[0]), mode == "fresh", True)
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_STEPS_DRAWS
    temb = head.time_embeddings(dev)
    torch.cuda.synchronize()
    assert torch.equal(lout[1], z) and torch.equal(z_only, z)
    assert n_only is None if noise is None else torch.equal(n_only, noise)
    assert noise is None or torch.equal(lout[2], noise)
    want = _head_want(head, readout, temb, z, noise, table, A, stored_bf16=True)
    got = _np(lout[0])
    assert np.all(np.abs(got) <= 5.0)
    print(f"loop vs stored-bf16 reference: max |err| {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, atol=5e-3, rtol=5e-3)
    f = _np(fused)
    rel = np.linalg.norm(got - f) / np.linalg.norm(f)
    print(f"loop vs fused: relative {rel:.3e}")
    assert rel <= 2e-2, rel


# ------------------------------------------------------------------------------------ model
def test_octo_action_chunks(dev):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    cfg = get_config("octo-tiny", num_blocks=2, action_horizon=2, sampler={"kind": "ddim", "steps": 4})
    model = O.Octo(cfg, dev, seed=0)
    assert model.head.A == 16
    B = 3
    H = cfg.image_size[0]
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (B, model.n_images, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    actions = torch.randn((B, 2, 8), generator=g).to(dev)
    rng = torch.tensor([11, 0], dtype=torch.int32, device=dev)
    loss3, _ = model.compute_diffusion_denoise_loss(None, images, actions, True, rng)
    loss2, _ = model.compute_diffusion_denoise_loss(None, images, actions.reshape(B, 16), True, rng)
    assert torch.isfinite(loss3).all() and torch.equal(loss3, loss2)
    with pytest.raises(ValueError):
        model.compute_diffusion_denoise_loss(None, images, actions[:, :1], True, rng)
    state = O.create_octo_train_state(model, seed=7)
    state, grads = O.diffusion_train_step(model, state, None, images, actions)
    assert state.step == 1 and np.isfinite(float(state.last_loss))
    assert float(sum(g.abs().sum() for g in grads.values())) > 0
    a = model.predict_diffusion_action(None, images, rng)              # the config's DDIM K = 4
    assert _C.sampler_last_route() == _C.SAMPLER_ROUTE_STEPS_LDS
    b = model.predict_diffusion_action(None, images, rng, sampler={"kind": "ddim", "steps": 4})
    c, z = model.predict_diffusion_action(None, images, rng, sampler={"noise": "fresh"},
                                          return_noise=True)[:2]
    torch.cuda.synchronize()
    for out in (a, b, c):
        assert out.shape == (B, 2, 8) and torch.isfinite(out).all() and out.abs().max() <= 5.0
    assert torch.equal(a, b) and not torch.equal(a, c) and z.shape == (B, 16)
