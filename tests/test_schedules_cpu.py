"""CPU: the learning-rate schedules' host closed forms (schedules.py, the reference the GPU tests
compare the device values with), the optimizer YAML, AdamW's defaults, and the argument checks of
the device-side optimizer entry points (include/mmt_api.h mmt_optim_prepare / mmt_adamw_dev /
mmt_workspace_size(MMT_WS_GRAD_NORM)), which return before any HIP call."""
import ctypes
import math

import pytest

from multi_modal_transformers_tokenmerge_amd import Constant, WarmupCosine, WarmupRsqrt
from multi_modal_transformers_tokenmerge_amd import schedules as S

INIT, PEAK, END, W, T, TAU = 1e-5, 3e-4, 3e-5, 10, 110, 50.0
STEPS = [0, 1, W - 1, W, W + 1, W + (T - W) // 2, T, T + 5]
# float64 closed forms of a handful of operations: far inside 1e-12 relative
REL = 1e-12


def _warm(s):
    return INIT + (PEAK - INIT) * s / W


def test_constant():
    c = Constant(2.5e-4)
    assert [c(s) for s in STEPS] == [2.5e-4] * len(STEPS)
    cs = c.to_c()
    assert cs.kind == S.SCHED_CONSTANT and cs.peak_value == 2.5e-4


def test_warmup_cosine_closed_form():
    f = WarmupCosine(INIT, PEAK, W, T, END)
    assert f(0) == INIT
    assert f(1) == pytest.approx(_warm(1), rel=REL)
    assert f(W - 1) == pytest.approx(_warm(W - 1), rel=REL)
    assert f(W) == pytest.approx(PEAK, rel=REL)
    c1 = 0.5 * (1 + math.cos(math.pi / (T - W)))
    assert f(W + 1) == pytest.approx(END + (PEAK - END) * c1, rel=REL)
    assert f(W + (T - W) // 2) == pytest.approx((PEAK + END) / 2, rel=REL)
    assert f(T) == pytest.approx(END, rel=REL)
    assert f(T + 5) == pytest.approx(END, rel=REL)
    assert f(T + 5) == f(T)
    vals = [f(s) for s in range(W, T + 1)]
    assert all(a > b for a, b in zip(vals, vals[1:]))  # strictly decaying after the warm-up
    z = WarmupCosine(0.0, 1e-3, 2, 6)  # end_value 0: exactly 0 from T on
    assert z(0) == 0.0 and z(6) == 0.0 and z(11) == 0.0 and z(2) == pytest.approx(1e-3, rel=REL)


def test_warmup_rsqrt_closed_form():
    f = WarmupRsqrt(INIT, PEAK, W, TAU)
    assert f(0) == INIT
    assert f(1) == pytest.approx(_warm(1), rel=REL)
    assert f(W - 1) == pytest.approx(_warm(W - 1), rel=REL)
    assert f(W) == PEAK
    assert f(W + 1) == pytest.approx(PEAK * math.sqrt(TAU / (1 + TAU)), rel=REL)
    assert f(W + int(TAU)) == pytest.approx(PEAK / math.sqrt(2), rel=REL)
    for s in (W + (T - W) // 2, T, T + 5):
        assert f(s) == pytest.approx(PEAK * math.sqrt(TAU / (s - W + TAU)), rel=REL)


def test_schedule_validation():
    for bad in (lambda: WarmupCosine(0, 1e-3, 0, 10), lambda: WarmupCosine(0, 0.0, 2, 10),
                lambda: WarmupCosine(0, 1e-3, 5, 5), lambda: WarmupCosine(0, 1e-3, 5, 4),
                lambda: WarmupRsqrt(0, 1e-3, 0, 10.0), lambda: WarmupRsqrt(0, 0.0, 2, 10.0),
                lambda: WarmupRsqrt(0, 1e-3, 2, 0.0), lambda: WarmupRsqrt(0, 1e-3, 2, -1.0)):
        with pytest.raises(ValueError):
            bad()


def test_c_struct_layout_and_fields():
    # int + pad, 3 doubles, 2 int64, 1 double (include/mmt_api.h mmt_lr_schedule_t)
    assert ctypes.sizeof(S.LrSchedule) == 56
    c = WarmupCosine(INIT, PEAK, W, T, END).to_c()
    assert (c.kind, c.init_value, c.peak_value, c.end_value, c.warmup_steps, c.decay_steps) == \
        (S.SCHED_WARMUP_COSINE, INIT, PEAK, END, W, T)
    r = WarmupRsqrt(INIT, PEAK, W, TAU).to_c()
    assert (r.kind, r.init_value, r.peak_value, r.warmup_steps, r.timescale) == \
        (S.SCHED_WARMUP_RSQRT, INIT, PEAK, W, TAU)


def test_yaml_instantiates_optimizer():
    from multi_modal_transformers_tokenmerge_amd import config_loader as CL
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import AdamW
    cfg = CL.compose("optimizers/adamw_warmup_cosine_clip")
    tx = CL.instantiate(cfg["optimizer"])
    assert isinstance(tx, AdamW) and isinstance(tx.learning_rate, WarmupCosine)
    assert tx.learning_rate == WarmupCosine(0.0, 3e-4, 2000, 300000, 3e-5)
    assert tx.max_grad_norm == 1.0 and tx.skip_nonfinite is True and tx.device_control
    assert (tx.b1, tx.b2, tx.eps, tx.weight_decay) == (0.9, 0.999, 1e-8, 1e-4)


def test_adamw_defaults_unchanged():
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import AdamW
    tx = AdamW()
    assert (tx.learning_rate, tx.b1, tx.b2, tx.eps, tx.weight_decay) == (3e-4, 0.9, 0.999, 1e-8, 1e-4)
    assert tx.max_grad_norm is None and tx.skip_nonfinite is False
    assert not tx.device_control  # the plain mmt_adamw launch, no device-side words
    assert AdamW(learning_rate=1e-3, max_grad_norm=1.0).device_control
    assert AdamW(skip_nonfinite=True).device_control
    assert AdamW(learning_rate=Constant(1e-3)).device_control
    assert AdamW(learning_rate=1e-3, max_grad_norm=1.0).schedule == Constant(1e-3)
    with pytest.raises(ValueError):
        AdamW(max_grad_norm=0.0)
    with pytest.raises(TypeError):
        AdamW(learning_rate="3e-4")


def test_workspace_size_grad_norm_without_gpu():
    from multi_modal_transformers_tokenmerge_amd import _C
    for n in (1, 1000, 90_000_000):
        assert _C.workspace_size(_C.WS_GRAD_NORM, n) == 4 * _C.GRAD_NORM_GRID > 0
    with pytest.raises(_C.MMTError):
        _C.workspace_size(_C.WS_GRAD_NORM, 16, 2)
    with pytest.raises(_C.MMTError):
        _C.workspace_size(_C.WS_GRAD_NORM)
    with pytest.raises(_C.MMTError):
        _C.workspace_size(_C.WS_GRAD_NORM, 0)


def test_optim_entry_points_reject_bad_arguments_without_gpu():
    """Argument validation happens before any HIP call: -1 (MMT_ERR_INVALID), no abort. The
    pointers are never dereferenced on these paths, so any aligned non-null value serves."""
    from multi_modal_transformers_tokenmerge_amd import _C
    lib = _C.lib()
    ws_bytes = _C.workspace_size(_C.WS_GRAD_NORM, 1000)
    ptr = 4096  # non-null, 16-B aligned

    def prepare(g=ptr, n=1000, sched=None, state=ptr, opt=ptr, ws=ptr, ws_b=ws_bytes):
        sc = Constant(1e-3).to_c() if sched is None else sched
        return lib.mmt_optim_prepare(g, n, 1.0, 1.0, 0, ctypes.addressof(sc), state, opt, ws, ws_b,
                                     None)

    assert prepare(g=None) == -1 and b"null" in lib.mmt_last_error()
    assert prepare(state=None) == -1 and prepare(opt=None) == -1 and prepare(ws=None) == -1
    assert lib.mmt_optim_prepare(ptr, 1000, 1.0, 1.0, 0, None, ptr, ptr, ptr, ws_bytes, None) == -1
    assert prepare(n=0) == -1 and prepare(n=-5) == -1
    assert prepare(g=ptr + 4) == -1 and b"aligned" in lib.mmt_last_error()
    assert prepare(ws_b=ws_bytes - 1) == -1 and b"workspace" in lib.mmt_last_error()
    bad_kind = Constant(1e-3).to_c()
    bad_kind.kind = 7
    assert prepare(sched=bad_kind) == -1 and b"kind" in lib.mmt_last_error()
    cos = WarmupCosine(0.0, 1e-3, 2, 6).to_c()
    for field, value in (("peak_value", 0.0), ("decay_steps", 2), ("decay_steps", 1),
                         ("warmup_steps", 0)):
        sc = S.LrSchedule.from_buffer_copy(cos)
        setattr(sc, field, value)
        assert prepare(sched=sc) == -1, (field, value)
    rs = WarmupRsqrt(0.0, 1e-3, 2, 10.0).to_c()
    for field, value in (("timescale", 0.0), ("timescale", -1.0), ("warmup_steps", 0)):
        sc = S.LrSchedule.from_buffer_copy(rs)
        setattr(sc, field, value)
        assert prepare(sched=sc) == -1, (field, value)

    def adamw_dev(p=ptr, g=ptr, m=ptr, v=ptr, n=1000, state=ptr, opt=ptr):
        return lib.mmt_adamw_dev(p, g, m, v, None, n, state, opt, 0.9, 0.999, 1e-8, 1e-4, None)
    assert adamw_dev(p=None) == -1 and adamw_dev(g=None) == -1 and adamw_dev(opt=None) == -1
    assert adamw_dev(state=None) == -1 and adamw_dev(n=0) == -1
