"""The multi-draw diffusion loss without a GPU: the reference of tests/diffusion_multi_ref.py
against the reference head's loss, its invariance under repeated draws, the condition on the
kernel-level test inputs (no pre-activation within rounding of zero), the fp32 emulation's
distance from float64 (the floor under the GPU tolerance), the draws' keys, and the config key."""
import numpy as np
import pytest

from oracle import rng as R
from tests import diffusion_multi_ref as MR

CASE_IDS = ["H%d-A%d-B%d-S%d-K%d" % c for c in MR.KERNEL_CASES]


# ------------------------------------------------------------------------------- test inputs
@pytest.mark.parametrize("case", MR.KERNEL_CASES, ids=CASE_IDS)
def test_no_pre_activation_near_zero(case):
    """The ReLU gate flips for a pre-activation within rounding of zero: the inputs of every
    kernel-level case keep all float64 pre-activations PRE_MARGIN = 1e-4 (about 100 x the fp32
    form's error, printed below) away from it, so no GPU comparison needs an exclusion. The
    recorded seed is the first that does."""
    H, A, B, steps, K = case
    inp = MR.kernel_inputs(*case)
    lo = MR.min_abs_pre(inp, A)
    print(f"min |pre| {lo:.3e}")
    assert lo >= MR.PRE_MARGIN
    assert MR.find_seed(case) == MR.KERNEL_SEEDS[case]
    assert inp["t"].shape == (K, B) and inp["t"].min() >= 0 and inp["t"].max() < steps
    share = inp["mask"].mean()
    assert 0.5 < share < 0.9, share


@pytest.mark.parametrize("mask", ["none", "random", "zero-row", "all-zero"])
@pytest.mark.parametrize("case", MR.KERNEL_CASES, ids=CASE_IDS)
def test_fp32_emulation_floor(case, mask):
    """Every operand, product and sum in fp32 (numpy's summation order) against float64: the
    floor the GPU tests' 1e-4 bar is compared against."""
    w64 = MR.want(case, mask, grad_scale=case[2] * case[4])
    w32 = MR.want(case, mask, grad_scale=case[2] * case[4], dtype=np.float32)
    worst = 0.0
    for k in ("loss", "noisy", "pre", "h", "dpred", "dh", "dP", "dQ"):
        a, b = np.asarray(w64[k], np.float64), np.asarray(w32[k], np.float64)
        err = float(np.max(np.abs(a - b) / (1.0 + np.abs(a))))
        worst = max(worst, err)
        print(f"{k}: fp32 vs float64 max err / (1 + |ref|) = {err:.3e}")
    assert np.array_equal(w64["pre"] > 0, w32["pre"] > 0)     # what PRE_MARGIN buys
    assert worst <= 1e-5, worst                                # 10 x under the GPU bar


# ------------------------------------------------------------------------------- the maths
def _reference_head_loss(inp, A):
    """diffusion.py:128-142 for one draw: mean_b sum_j 0.5 (pred - eps)^2, written out plainly."""
    abar = inp["alpha_hats"].astype(np.float64)
    t, eps = inp["t"][0], inp["eps"][0].astype(np.float64)
    total = 0.0
    for b in range(inp["actions"].shape[0]):
        noisy = np.sqrt(abar[t[b]]) * inp["actions"][b] + np.sqrt(1 - abar[t[b]]) * eps[b]
        pre = inp["w1"][:, :A].astype(np.float64) @ noisy + inp["Q"][t[b]] + inp["P"][b]
        pred = inp["w2"].astype(np.float64) @ np.maximum(pre, 0) + inp["b2"]
        total += 0.5 * np.sum((pred - eps[b]) ** 2)
    return total / inp["actions"].shape[0]


def test_all_ones_k1_is_the_reference_loss():
    case = MR.KERNEL_CASES[-1]
    assert case[4] == 1
    inp = MR.kernel_inputs(*case)
    got = MR.want(case, "none")
    np.testing.assert_allclose(got["loss"], _reference_head_loss(inp, case[1]), rtol=1e-12)
    ones = MR.loss_multi(inp["actions"], np.ones_like(inp["mask"]), inp["alpha_hats"], inp["P"],
                         inp["Q"], inp["w1"][:, :case[1]], inp["w2"], inp["b2"], inp["t"], inp["eps"])
    for k in ("loss", "dpred", "dh", "dP", "dQ"):
        np.testing.assert_allclose(ones[k], got[k], rtol=1e-12, atol=0)


@pytest.mark.parametrize("mask", ["none", "random"])
def test_repeated_draws_give_the_single_draw_result(mask):
    """The same (t, eps) in each of K draws: the K = 1 loss and gradients (the 1 / K in the
    normaliser against the K equal terms)."""
    case = MR.KERNEL_CASES[-1]
    H, A, B, steps, _ = case
    inp = MR.kernel_inputs(*case)
    m = MR.masks(inp)[mask]
    args = (inp["actions"], m, inp["alpha_hats"], inp["P"], inp["Q"], inp["w1"][:, :A], inp["w2"],
            inp["b2"])
    one = MR.loss_multi(*args, inp["t"], inp["eps"])
    K = 3
    rep = MR.loss_multi(*args, np.repeat(inp["t"], K, 0), np.repeat(inp["eps"], K, 0))
    np.testing.assert_allclose(rep["loss"], one["loss"], rtol=1e-12)
    np.testing.assert_allclose(rep["dP"], one["dP"], rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(rep["dQ"], one["dQ"], rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(rep["dpred"].sum(0), one["dpred"][0], rtol=1e-10, atol=1e-15)


def test_mask_edge_cases():
    case = MR.KERNEL_CASES[0]
    zero = MR.want(case, "all-zero")
    assert zero["loss"] == 0 and not zero["dpred"].any() and not zero["dP"].any()
    row = MR.want(case, "zero-row")
    assert not row["dpred"][:, 1].any() and not row["dP"][1].any() and row["dP"][0].any()


def test_dpred_is_the_gradient_of_the_loss():
    """Central differences of the loss in pred's bias against sum(dpred): ties the backward's
    scale A / (K sum m) to the forward's."""
    case = MR.KERNEL_CASES[0]
    H, A, B, steps, K = case
    inp = MR.kernel_inputs(*case)
    m = MR.masks(inp)["random"]

    def loss(b2):
        return MR.loss_multi(inp["actions"], m, inp["alpha_hats"], inp["P"], inp["Q"],
                             inp["w1"][:, :A], inp["w2"], b2, inp["t"], inp["eps"])
    base = loss(inp["b2"])
    for j in (0, A - 1):
        hstep = np.zeros(A)
        hstep[j] = 1e-6
        num = (loss(inp["b2"] + hstep)["loss"] - loss(inp["b2"] - hstep)["loss"]) / 2e-6
        np.testing.assert_allclose(base["dpred"][:, :, j].sum(), num, rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------- draws
def test_draw_keys():
    """Draw 0 is mmt_diffusion_prep's stream; draws 1.. use layer 0xFFF9, a stream each."""
    B, A, steps, K = 9, 16, 32, 5
    t, eps = MR.draws(4321, 7, B, A, steps, K, sample_offset=3)
    t0, eps0 = R.diffusion_t_eps(4321, 7, B, A, steps, 3)
    assert np.array_equal(t[0], t0)
    np.testing.assert_allclose(eps[0], eps0, atol=1e-5, rtol=1e-5)
    keys = [MR.t_key(4321, 7, k) for k in range(64)] + [MR.eps_key(4321, 7, k) for k in range(64)]
    assert len(set(keys)) == 128
    assert t.min() >= 0 and t.max() < steps
    assert len({e.tobytes() for e in eps}) == K
    tail_t, tail_eps = MR.draws(4321, 7, B - 2, A, steps, K, sample_offset=5)
    assert np.array_equal(tail_t, t[:, 2:]) and np.array_equal(tail_eps, eps[:, 2:])


# ------------------------------------------------------------------------------- config
def test_nd8_config_loads():
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import OctoConfig, get_config
    cfg = get_config("octo_small_tome16_chunk4_nd8")
    assert cfg.n_diffusion_samples == 8 and cfg.action_horizon == 4
    assert get_config("octo_small_tome16_chunk4").n_diffusion_samples == 1
    assert get_config("octo_small_tome16").n_diffusion_samples == 1
    assert OctoConfig(n_diffusion_samples=64).n_diffusion_samples == 64
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            OctoConfig(n_diffusion_samples=bad)


def test_head_rejects_the_option_beyond_the_fused_kernel():
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    for kw in (dict(action_dim=16, num_blocks=2), dict(action_dim=12), dict(action_dim=72),
               dict(action_dim=16, hidden=1032)):
        with pytest.raises(ValueError):
            DiffusionActionHead.create(ParamStore(), "h", 64, n_diffusion_samples=2, **kw)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            DiffusionActionHead.create(ParamStore(), "h", 64, 16, n_diffusion_samples=bad)
    head = DiffusionActionHead.create(ParamStore(), "h", 64, 16, n_diffusion_samples=4)
    assert head.n_diffusion_samples == 4
    assert DiffusionActionHead.create(ParamStore(), "h", 64, 16, num_blocks=2).n_diffusion_samples == 1
