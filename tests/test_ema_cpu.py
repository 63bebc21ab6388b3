"""The parameter EMA without a GPU: schedules.EmaDecay (the diffusers / Diffusion-Policy EMAModel
warm-up restated in float64, its C struct, its validation), AdamW.ema_decay, the EMA buffer of a
host-built model's store, and the optimizer YAML."""
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import config_loader as CL
from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
from multi_modal_transformers_tokenmerge_amd.schedules import (EMA_CONSTANT, EMA_WARMUP,
                                                               ConstantEmaDecay, EmaDecay,
                                                               WarmupCosine)


def test_schedule_defaults():
    e = EmaDecay()
    assert e(0) == 0.0 and e(1) == 0.0
    assert e(2) == 1.0 - 2.0 ** -0.75
    assert e(3) == 1.0 - 3.0 ** -0.75
    assert e(50) == 1.0 - 50.0 ** -0.75
    assert all(e(s) < e(s + 1) for s in range(1, 200))


def test_schedule_clamp_floor_and_shift():
    e = EmaDecay(max_value=0.9)
    # the defaults give 1 - s^-0.75, which first exceeds 0.9 at s = 22 (21^-0.75 = 0.1019,
    # 22^-0.75 = 0.0984)
    assert e(21) == 1.0 - 21.0 ** -0.75 < 0.9
    assert e(22) == 0.9 and e(10 ** 6) == 0.9
    assert EmaDecay()(10 ** 9) == 0.9999
    f = EmaDecay(min_value=0.5)
    assert f(1) == 0.0                      # k == 0 is 0 whatever the floor (EMAModel: step <= 0)
    assert f(2) == 0.5 > 1.0 - 2.0 ** -0.75  # the floor
    assert f(3) == 1.0 - 3.0 ** -0.75 > 0.5
    s = EmaDecay(update_after_step=10)
    assert [s(i) for i in range(12)] == [0.0] * 12
    assert s(12) == EmaDecay()(2) and s(13) == EmaDecay()(3)
    g = EmaDecay(inv_gamma=4.0, power=2.0 / 3.0)
    assert g(9) == 1.0 - (1.0 + 8 / 4.0) ** -(2.0 / 3.0)


def test_to_c_fields():
    c = EmaDecay(0.999, 0.25, 2.0, 0.5, 7).to_c()
    assert (c.kind, c.value, c.max_value, c.min_value, c.inv_gamma, c.power,
            c.update_after_step) == (EMA_WARMUP, 0.0, 0.999, 0.25, 2.0, 0.5, 7)
    k = ConstantEmaDecay(0.99).to_c()
    assert (k.kind, k.value) == (EMA_CONSTANT, 0.99)
    assert ConstantEmaDecay(0.99)(0) == ConstantEmaDecay(0.99)(10 ** 6) == 0.99


@pytest.mark.parametrize("kw", [dict(max_value=1.5), dict(max_value=-0.1), dict(min_value=-0.1),
                                dict(min_value=1.1), dict(max_value=0.5, min_value=0.6),
                                dict(inv_gamma=0.0), dict(inv_gamma=-1.0), dict(power=-0.5),
                                dict(update_after_step=-1), dict(max_value=float("nan"))])
def test_ema_decay_rejects(kw):
    with pytest.raises(ValueError):
        EmaDecay(**kw)


def test_adamw_ema_decay_field():
    assert O.AdamW().ema_decay is None and O.AdamW().ema_schedule is None
    assert O.AdamW(ema_decay=0.99).ema_schedule == ConstantEmaDecay(0.99)
    assert O.AdamW(ema_decay=0).ema_schedule == ConstantEmaDecay(0.0)
    e = EmaDecay(update_after_step=3)
    assert O.AdamW(ema_decay=e).ema_schedule is e
    # the EMA does not by itself ask for the device-side optimizer words
    assert not O.AdamW(ema_decay=e).device_control
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            O.AdamW(ema_decay=bad)
    for bad in ("0.99", True, [0.99], WarmupCosine(0.0, 1e-3, 2, 6), ConstantEmaDecay(0.5)):
        with pytest.raises((TypeError, ValueError)):
            O.AdamW(ema_decay=bad)


def test_store_ema_follows_the_latest_state():
    m = O.Octo(get_config("octo-tiny"), torch.device("cpu"), seed=0)
    assert m.store.ema is None
    st = O.create_octo_train_state(m, O.AdamW(ema_decay=EmaDecay()))
    assert m.store.ema is not m.store.flat and torch.equal(m.store.ema, m.store.flat)
    assert m.store.ema.dtype == torch.float32 and m.store.ema.numel() == m.store.n
    views = st.ema_params
    assert list(views) == [p.name for p in m.store.params]
    for p in m.store.params:
        assert views[p.name].shape == p.data.shape
        assert views[p.name].data_ptr() == m.store.ema.data_ptr() + 4 * p.offset
    assert st.last_ema_decay == 0.0
    plain = O.create_octo_train_state(m, O.AdamW())
    assert m.store.ema is None
    for s in (plain, st):  # the later state dropped it
        with pytest.raises(AttributeError):
            s.ema_params
        with pytest.raises(AttributeError):
            s.ema_weights()
        with pytest.raises(AttributeError):
            s.last_ema_decay


def test_yaml_instantiates():
    tx = CL.instantiate(CL.compose("optimizers/adamw_diffusion_ema")["optimizer"])
    assert isinstance(tx, O.AdamW) and isinstance(tx.ema_decay, EmaDecay)
    assert tx.ema_decay == EmaDecay(0.9999, 0.0, 1.0, 0.75, 0)
    assert isinstance(tx.learning_rate, WarmupCosine) and tx.max_grad_norm == 1.0
    assert tx.skip_nonfinite and tx.device_control and not tx.grouped
