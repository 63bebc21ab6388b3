"""CPU: the configuration rules of the chunked continuous / categorical heads (pred_horizon,
continuous_loss), the float64 reference of tests/heads_chunk_ref.py against oracle/heads_ref.py
at h = 1, bin_values as the inverse of assign_bins, and the reference's mask normalisation."""
import numpy as np
import pytest

from multi_modal_transformers_tokenmerge_amd.action_heads.categorical import assign_bins, bin_values
from multi_modal_transformers_tokenmerge_amd.models.octo.config import OctoConfig, get_config
from oracle import heads_ref as HR
from tests import heads_chunk_ref as CR


# ------------------------------------------------------------------------------- configuration
@pytest.mark.parametrize("kind", ["continuous", "categorical"])
def test_pred_horizon_constructs(kind):
    cfg = OctoConfig(pred_horizon=2, action_heads=("diffusion", kind))
    assert cfg.pred_horizon == 2 and cfg.action_horizon == 1
    # the two horizons agree beside a non-diffusion head
    cfg = OctoConfig(action_horizon=2, pred_horizon=2, action_heads=("diffusion", kind))
    assert cfg.pred_horizon == cfg.action_horizon == 2
    assert OctoConfig().pred_horizon == 1 and OctoConfig().continuous_loss == "mse"
    assert OctoConfig(continuous_loss="l1").continuous_loss == "l1"


@pytest.mark.parametrize("ph", [1, 3])
def test_horizons_must_agree(ph):
    with pytest.raises(ValueError, match="pred_horizon"):
        OctoConfig(action_horizon=2, pred_horizon=ph, action_heads=("diffusion", "continuous"))
    # without such a head the diffusion head's chunk stands alone
    assert OctoConfig(action_horizon=2, pred_horizon=ph).action_horizon == 2


@pytest.mark.parametrize("kw", [dict(pred_horizon=0), dict(pred_horizon=-1), dict(pred_horizon=1.5),
                                dict(continuous_loss="huber"), dict(continuous_loss="L1")])
def test_bad_values_raise(kw):
    with pytest.raises(ValueError):
        OctoConfig(**kw)


def test_yaml_fields():
    cfg = get_config("octo_small_tome16_cont_chunk4")
    assert cfg.pred_horizon == 4 and cfg.continuous_loss == "l1"
    assert cfg.action_heads == ("diffusion", "continuous")
    assert cfg.action_horizon == 1 and cfg.action_space_dim == 8
    assert cfg.token_compression_sequence and cfg.token_embedding_dim == 384
    base = get_config("octo_small_tome16")
    assert base.pred_horizon == 1 and base.continuous_loss == "mse"
    assert base.action_heads == ("diffusion",)


# ------------------------------------------------------------------------------- reference
def test_reference_is_the_oracle_at_h1():
    g = np.random.default_rng(0)
    B, A, N, m = 9, 8, 32, 5.0
    z = g.standard_normal((B, A)) * 6
    y = g.standard_normal((B, A)) * 2
    p, l, dz = CR.continuous(z, y, None, 1, A, "mse", m)
    p0, l0, dz0 = HR.continuous(z, y, m)
    assert p.shape == (B, 1, A)
    np.testing.assert_allclose(p, p0, rtol=1e-12, atol=1e-12)
    assert l == pytest.approx(l0, rel=1e-12)
    np.testing.assert_allclose(dz, dz0, rtol=1e-12, atol=1e-12)
    zl = g.standard_normal((B, A, N)) * 3
    ya = (g.random((B, A)) * 12 - 6).astype(np.float32)
    ya[0, :3] = [-5.0, 5.0, 4.99]
    l, dz, cls = CR.categorical(zl, ya, None, 1, A, m)
    l0, dz0 = HR.categorical(zl, ya, m, N)
    assert l == pytest.approx(l0, rel=1e-12)
    np.testing.assert_allclose(dz, dz0, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(cls, zl.argmax(-1))


def test_chunk_is_steps_as_samples():
    """Without a mask a chunk of h steps is h times as many one-step samples."""
    g = np.random.default_rng(1)
    B, h, A, N = 4, 3, 5, 16
    z, y = g.standard_normal((B, h * A)) * 4, g.standard_normal((B, h * A)) * 2
    _, l, dz = CR.continuous(z, y, None, h, A)
    _, l1, dz1 = CR.continuous(z.reshape(B * h, A), y.reshape(B * h, A), None, 1, A)
    assert l == pytest.approx(l1, rel=1e-12)
    np.testing.assert_allclose(dz, dz1.reshape(B, h * A), rtol=1e-12)
    zl, ya = g.standard_normal((B, h * A, N)), (g.random((B, h * A)) * 10 - 5).astype(np.float32)
    l, dz, _ = CR.categorical(zl, ya, None, h, A)
    l1, dz1, _ = CR.categorical(zl.reshape(B * h, A, N), ya.reshape(B * h, A), None, 1, A)
    assert l == pytest.approx(l1, rel=1e-12)
    np.testing.assert_allclose(dz, dz1.reshape(dz.shape), rtol=1e-12)


@pytest.mark.parametrize("loss", ["mse", "l1"])
def test_mask_normalisation(loss):
    inp = CR.cont_inputs(5, 3, 8)
    ones = np.ones_like(inp["mask"])
    _, l_none, dz_none = CR.continuous(inp["z"], inp["y"], None, 3, 8, loss)
    _, l_ones, dz_ones = CR.continuous(inp["z"], inp["y"], ones, 3, 8, loss)
    assert l_ones == l_none and np.array_equal(dz_ones, dz_none)
    _, l_zero, dz_zero = CR.continuous(inp["z"], inp["y"], 0 * ones, 3, 8, loss)
    assert l_zero == 0.0 and not dz_zero.any() and np.isfinite(dz_zero).all()
    # a masked component carries no gradient; the rest is rescaled by count / sum m
    _, l_m, dz_m = CR.continuous(inp["z"], inp["y"], inp["mask"], 3, 8, loss)
    keep = inp["mask"] != 0
    assert not dz_m[~keep].any()
    np.testing.assert_allclose(dz_m[keep], dz_none[keep] * keep.size / keep.sum(), rtol=1e-12)


def test_mask_normalisation_categorical():
    inp = CR.cat_inputs(3, 2, 3, 32)
    ones = np.ones_like(inp["mask"])
    l_none, dz_none, _ = CR.categorical(inp["z"], inp["y"], None, 2, 3)
    l_ones, dz_ones, _ = CR.categorical(inp["z"], inp["y"], ones, 2, 3)
    assert l_ones == l_none and np.array_equal(dz_ones, dz_none)
    l_zero, dz_zero, _ = CR.categorical(inp["z"], inp["y"], 0 * ones, 2, 3)
    assert l_zero == 0.0 and not dz_zero.any()


def test_l1_inputs_keep_their_margin():
    for case in CR.CONT_CASES:
        inp = CR.cont_inputs(*case)
        p, _, _ = CR.continuous(inp["z"], inp["y"], None, case[1], case[2], "l1")
        assert np.abs(p.reshape(inp["y"].shape) - inp["y"]).min() >= CR.L1_MARGIN
        if inp["y"].shape[1] >= 3:
            np.testing.assert_array_equal(inp["y"][0, :3], np.float32([-5.0, 5.0, 4.99]))


# ------------------------------------------------------------------------------- decode table
@pytest.mark.parametrize("N,m", [(32, 5.0), (256, 5.0), (100, 2.5)])
def test_bin_values_invert_assign_bins(N, m):
    """Every target that has a class decodes to within half a bin (m / N) of itself; targets
    below the range decode to -m. Targets: 1e5 uniform draws over [-1.2 m, 1.2 m), every edge and
    the float just below it."""
    v = bin_values((-m, m), N)
    assert v.shape == (N,) and v.dtype == np.float32 and v[0] == np.float32(-m)
    edges = np.linspace(-m, m, N + 1, dtype=np.float32)
    g = np.random.default_rng(N)
    y = np.concatenate([(g.random(100000) * 2.4 * m - 1.2 * m).astype(np.float32), edges,
                        np.nextafter(edges, np.float32(-np.inf))])
    bins = assign_bins(y, (-m, m), N)
    has = bins < N
    assert has.sum() > 80000   # all but the top interval and what lies above the range
    dec = v[bins[has]].astype(np.float64)
    err = np.abs(dec - y[has].astype(np.float64))
    inside = bins[has] >= 1
    print(f"N {N} m {m}: max |decode - y| / (m / N) = {err[inside].max() / (m / N):.8f}")
    assert err[inside].max() <= (m / N) * (1 + 1e-5)
    below = bins == 0
    assert below.any() and np.all(y[below] < np.float32(-m)) and np.all(v[bins[below]] == np.float32(-m))
    # the classes are increasing, so argmax over neighbouring logits moves the action one way
    assert np.all(np.diff(v.astype(np.float64)) > 0)
    # the reference decode through the table: the float64 restatement of the kernel's rule
    z = np.full((2, N), -1.0)
    z[0, 5] = z[0, 7] = 3.0
    z[1, N - 1] = 3.0
    cls, act = CR.decode(z, v)
    assert cls.tolist() == [5, N - 1] and act.tolist() == [v[5], v[N - 1]]


def test_decode_reference_rule():
    """Smallest c with CDF(c) > u, clamped; u = ((draw >> 8) + 0.5) / 2^24 in fp32 lies in (0, 1]
    and is the same for the same key and counter."""
    z = np.log(np.array([[0.25, 0.25, 0.5]]))
    for u, want in ((0.0, 0), (0.2499, 0), (0.25, 1), (0.4999, 1), (0.5, 2), (1.0, 2)):
        assert CR.decode(z, np.arange(3.0), np.array([u]))[0][0] == want, u
    u = CR.decode_u(7, 3, 4096, 8)
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    np.testing.assert_array_equal(u[8:16], CR.decode_u(7, 3, 8, 8, sample_offset=1))
    assert not np.array_equal(u[:64], CR.decode_u(7, 4, 64, 8))
    assert abs(float(u.mean()) - 0.5) < 0.02
