"""CPU: the step-table sampler's host side. The DDPM / DDIM tables of
DiffusionActionHead.sampler_table against the independent restatement and known answers, the
float64 reference of tests/sampler_steps_ref.py against the project's DDPM oracle, the argument
checks of mmt_diffusion_sample_steps (rejected before any HIP call, so no GPU is needed: the
pointers are never dereferenced), the spec / config plumbing, and the inputs of the kernel-level
GPU test: their saturation and the fp32 emulation's distance from the float64 reference."""
import numpy as np
import pytest

from multi_modal_transformers_tokenmerge_amd import _C
from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import (DiffusionActionHead,
                                                                            SamplerSpec)
from multi_modal_transformers_tokenmerge_amd.params import ParamStore
from oracle import sampler_ref as ref
from tests import sampler_steps_ref as SR

S = 32


@pytest.fixture(scope="module")
def head():
    return DiffusionActionHead.create(ParamStore(), "diffusion_action_head", 192, 16, S)


# ------------------------------------------------------------------------------- tables
def test_ddpm_rows_are_the_oracle_coefficients(head):
    c = ref.sampler_coefficients(head.betas_np, head.alpha_hats_np)      # rows t = 0 .. S-1
    for spec, final in ((SamplerSpec(), True), (SamplerSpec(noise="fresh"), False),
                        (SamplerSpec(noise="fresh", final_noise=True), True),
                        (SamplerSpec(final_noise=False), False)):
        t, coef = head.sampler_table(spec)
        assert t.dtype == np.int32 and coef.dtype == np.float32 and coef.shape == (S, 3)
        assert np.array_equal(t, np.arange(S - 1, -1, -1))
        # x <- c1 (x - c2 eps) + c3 n  ==  a x + b eps + c n
        want = np.stack([c[t, 0], -c[t, 0] * c[t, 1], c[t, 2]], axis=1)
        if not final:
            want[-1, 2] = 0.0
        np.testing.assert_allclose(coef, want, rtol=2e-7, atol=0)
        t2, coef2 = SR.ddpm_table(head.betas_np, head.alpha_hats_np, final)
        assert np.array_equal(t, t2) and np.array_equal(coef, coef2)
    assert np.array_equal(head.sampler_table(SamplerSpec(steps=S))[1], head.sampler_table()[1])


@pytest.mark.parametrize("K", [1, 4, 8, S])
def test_ddim_rows(head, K):
    t, coef = head.sampler_table(SamplerSpec(kind="ddim", steps=K))
    t2, coef2 = SR.ddim_table(head.alpha_hats_np, K)
    assert np.array_equal(t, t2) and np.array_equal(coef, coef2)
    assert t.shape == (K,) and t[0] == S - 1 and np.all(np.diff(t) < 0)
    if K == 1:
        assert t.tolist() == [S - 1]
    else:
        assert t[-1] == 0
    if K == S:
        assert t.tolist() == list(range(S - 1, -1, -1))
    assert {4: [31, 21, 10, 0], 8: [31, 27, 22, 18, 13, 9, 4, 0]}.get(K, t.tolist()) == t.tolist()
    abar = head.alpha_hats_np.astype(np.float64)
    prev = SR.ddim_abar_prev(abar, t)
    assert prev[-1] == 1.0 and np.array_equal(prev[:-1], abar[t[1:]])
    assert np.all(coef[:, 2] == 0)
    # the last row lands on x0_hat = (x - sqrt(1 - abar_t) eps) / sqrt(abar_t)
    at = abar[t[-1]]
    np.testing.assert_allclose(coef[-1, :2], [1 / np.sqrt(at), -np.sqrt(1 - at) / np.sqrt(at)],
                               rtol=2e-7)
    # a perfect eps prediction is carried along the forward marginals x_t = sqrt(abar) x0 +
    # sqrt(1 - abar) eps
    x0, eps = 0.3, -1.1
    x = np.sqrt(abar[t[0]]) * x0 + np.sqrt(1 - abar[t[0]]) * eps
    err = 0.0     # the fp32 rounding of a and b (half an ulp, 2^-24 relative), carried along
    for k in range(K):
        a, b = float(coef[k, 0]), float(coef[k, 1])
        err = abs(a) * err + 2.0 ** -24 * (abs(a * x) + abs(b * eps))
        x = a * x + b * eps
        np.testing.assert_allclose(x, np.sqrt(prev[k]) * x0 + np.sqrt(1 - prev[k]) * eps,
                                   atol=err + 1e-12, rtol=0)


def test_bad_specs_raise(head):
    for kw in (dict(kind="heun"), dict(noise="pink"), dict(steps=0), dict(steps=2.5),
               dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")),
               dict(kind="ddim", noise="fresh"), dict(kind="ddim", final_noise=True)):
        with pytest.raises(ValueError):
            SamplerSpec(**kw)
    with pytest.raises(ValueError):
        SamplerSpec.of({"kind": "ddpm", "eta": 0.5})
    with pytest.raises(ValueError):
        head.sampler_table(SamplerSpec(steps=8))                    # DDPM walks all S steps
    with pytest.raises(ValueError):
        head.sampler_table(SamplerSpec(kind="ddim", steps=S + 1))
    with pytest.raises(ValueError):
        DiffusionActionHead.create(ParamStore(), "h", 192, 16, S, sampler={"kind": "euler"})
    assert SamplerSpec.of({"kind": "ddim", "steps": 8}) == SamplerSpec("ddim", 8)
    assert SamplerSpec().is_reference(S) and SamplerSpec(steps=S, final_noise=True).is_reference(S)
    for spec in (SamplerSpec(noise="fresh"), SamplerSpec(clip=1.0), SamplerSpec(final_noise=False),
                 SamplerSpec("ddim", S)):
        assert not spec.is_reference(S)
    h2 = DiffusionActionHead.create(ParamStore(), "h", 192, 16, S, sampler={"kind": "ddim", "steps": 4})
    assert h2.sampler == SamplerSpec("ddim", 4) and len(h2.sampler_table()[0]) == 4


# ------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("A", [8, 24])
def test_reference_with_frozen_ddpm_table_is_the_ddpm_oracle(head, A):
    g = np.random.default_rng(A)
    B, D, T, H = 5, 48, 16, 64
    readout, z = g.standard_normal((B, D)), g.standard_normal((B, A))
    temb = ref.bf16(g.standard_normal((S, T)))
    w1 = g.standard_normal((H, A + T + D)) / np.sqrt(A + T + D)
    b1, b2 = 0.1 * g.standard_normal(H), 0.1 * g.standard_normal(A)
    w2 = g.standard_normal((A, H)) / np.sqrt(H)
    t, coef = SR.ddpm_table(head.betas_np, head.alpha_hats_np, True)
    P, Q, w1x = SR.split_first_dense(readout, temb, w1, b1, A)
    c_ref = ref.sampler_coefficients(head.betas_np, head.alpha_hats_np)
    for stored in (False, True):
        want = ref.predict_action(readout, z, temb, w1, b1, w2, b2, c_ref, stored_bf16=stored)
        got = SR.run_steps(P, Q, w1x, w2, b2, t, coef, 5.0, z, stored_bf16=stored)
        assert np.any(np.abs(want) < 5.0)
        # the table is fp32 and recombined (a x + b eps against c1 (x - c2 eps)); with bf16
        # storage a value on a rounding boundary may flip (one bf16 ulp of x, 2^-8 relative)
        np.testing.assert_allclose(got, want, atol=2e-2 if stored else 1e-5, rtol=0)
        assert np.abs(got - want).mean() < (1e-3 if stored else 1e-6)


# ------------------------------------------------------------------------------- C ABI
PTR = 1 << 20          # non-null, 16-B aligned


def _call(lib, rng=PTR, B=4, A=16, n_steps=8, H=192, q_rows=32, w1=PTR, ld_w1=400, w2=PTR,
          clip=5.0, flags=0, z_in=None, noise_in=None, noise_out=None, z_out=None):
    return lib.mmt_diffusion_sample_steps(rng, B, A, n_steps, 0, PTR, H, PTR, H, q_rows, w1, ld_w1,
                                          w2, PTR, PTR, PTR, clip, flags, z_in, noise_in, H, PTR,
                                          z_out, noise_out, None)


@pytest.mark.parametrize("kw", [
    dict(A=12), dict(A=72), dict(A=0), dict(H=196), dict(H=1032), dict(H=0), dict(n_steps=0),
    dict(n_steps=1025), dict(q_rows=0), dict(clip=0.0), dict(clip=-5.0), dict(clip=float("nan")),
    dict(w1=PTR + 2), dict(w1=PTR + 8), dict(ld_w1=396), dict(ld_w1=8), dict(w2=PTR + 8),
    dict(rng=None), dict(rng=None, z_in=PTR, flags=_C.SAMPLE_FRESH_NOISE), dict(flags=4),
    dict(noise_in=PTR), dict(noise_out=PTR), dict(B=0),
    # MMT_SAMPLE_DRAWS_ONLY: an output is needed, and the width, step and rng rules still hold
    dict(flags=_C.SAMPLE_DRAWS_ONLY), dict(flags=_C.SAMPLE_DRAWS_ONLY, z_out=PTR, A=12),
    dict(flags=_C.SAMPLE_DRAWS_ONLY, z_out=PTR, n_steps=1025),
    dict(flags=_C.SAMPLE_DRAWS_ONLY, z_out=PTR, rng=None),
    dict(flags=_C.SAMPLE_DRAWS_ONLY, noise_out=PTR),
    dict(flags=_C.SAMPLE_DRAWS_ONLY | _C.SAMPLE_FRESH_NOISE, noise_out=PTR, rng=None, z_in=PTR),
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_c_abi_rejects_before_launch(kw):
    lib = _C.lib()
    assert _call(lib, **kw) == -1                       # MMT_ERR_INVALID
    assert b"mmt_diffusion_sample_steps" in lib.mmt_last_error()
    assert lib.mmt_sampler_last_route() == _C.SAMPLER_ROUTE_NONE


def test_step_noise_streams_do_not_repeat():
    """stream_key keeps 8 bits of its site, so the step index is split over the site (16 + k % 240)
    and the layer word (0xFFFE - k // 240): over the 1024 steps the entry accepts, every step has
    a key of its own, none is z's (site 3) or a training stream (sites 1, 2), and the first 240
    are site 16 + k of layer 0xFFFE."""
    from oracle import rng as R
    keys = [SR.step_noise_key(77, 3, k) for k in range(1024)]
    assert len(set(keys)) == 1024
    assert not set(keys) & {R.stream_key(77, 3, 0xFFFE, s) for s in range(16)}
    assert keys[:240] == [R.stream_key(77, 3, 0xFFFE, 16 + k) for k in range(240)]
    # what a key built from 16 + k alone would do: step 243 lands on z's stream
    assert R.stream_key(77, 3, 0xFFFE, 16 + 243) == R.stream_key(77, 3, 0xFFFE, 3)
    assert keys[243] != R.stream_key(77, 3, 0xFFFE, 3) and keys[256] != keys[0]


def test_route_rule():
    """LDS-resident while the padded bf16 W1x and W2 rows and the P + Q rows fit in 160 KB."""
    R = _C.sampler_steps_route
    assert [R(A, H) for H, A, _, _ in SR.KERNEL_CASES] == [_C.SAMPLER_ROUTE_STEPS_LDS] * 3 + \
        [_C.SAMPLER_ROUTE_STEPS_STREAM]
    assert R(32, 384) == R(64, 384) == R(64, 512) == _C.SAMPLER_ROUTE_STEPS_LDS
    assert R(64, 576) == _C.SAMPLER_ROUTE_STEPS_STREAM    # 4 576 72 + 18 KB > 160 KB


# ------------------------------------------------------------------------------- config
def test_chunk_config_loads():
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import OctoConfig, get_config
    cfg = get_config("octo_small_tome16_chunk4")
    assert cfg.action_horizon == 4 and cfg.action_space_dim * cfg.action_horizon == 32
    assert SamplerSpec.of(cfg.sampler) == SamplerSpec("ddim", 8)
    base = get_config("octo_small_tome16")
    assert base.action_horizon == 1 and base.sampler is None
    for kw in (dict(action_horizon=0), dict(action_horizon=2, action_heads=("diffusion", "continuous")),
               dict(action_horizon=2, action_heads=("diffusion", "categorical")),
               dict(sampler={"kind": "ddim", "noise": "fresh"})):
        with pytest.raises(ValueError):
            OctoConfig(**kw)


# ------------------------------------------------------------------------------- GPU test inputs
@pytest.mark.parametrize("case", SR.KERNEL_CASES, ids=lambda c: "H%d-A%d-B%d-q%d" % c)
def test_kernel_test_inputs(case):
    """On the arrays the kernel-level GPU test uses: the share of reference outputs at +-clip is
    under that test's caps, and the fp32 emulation of the update stays within its tolerance of
    the float64 reference (far within: the margin is the kernel's reduction order)."""
    H, A, B, q_rows = case
    inp = SR.kernel_inputs(H, A, B, q_rows)
    t, coef = SR.kernel_table(q_rows)
    assert np.array_equal(t, [(5 * k + 3) % q_rows for k in range(SR.KERNEL_K)])
    if q_rows % 5:       # Q is indexed non-monotonically (q_rows = 5 stays on row 3)
        assert len(set(np.diff(t.astype(int)) > 0)) == 2
    for fresh in (False, True):
        for clip, cap in SR.SATURATION_CAP.items():
            args = (inp["P"], inp["Q"], inp["w1"][:, :A], inp["w2"], inp["b2"], t, coef, clip,
                    inp["z"], inp["noise"] if fresh else None)
            want = SR.run_steps(*args)
            assert SR.saturated(want, clip).mean() <= cap
            f32 = SR.run_steps(*args, dtype=np.float32)
            assert f32.dtype == np.float32
            np.testing.assert_allclose(f32, want, atol=1e-5, rtol=1e-5)
            stored = SR.run_steps(*args, stored_bf16=True)
            np.testing.assert_allclose(stored, want, atol=5e-3, rtol=5e-3)
