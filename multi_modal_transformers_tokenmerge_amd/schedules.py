"""Learning-rate schedules evaluated on the device (include/mmt_api.h mmt_optim_prepare).

The reference takes any optax ``GradientTransformation`` from its caller (octo.py:341,377);
Octo-style runs pass ``optax.chain(clip_by_global_norm, adamw(schedule))``. The step counter lives
on the device (``rng[1]``), and the captured step graph freezes every kernel argument, so a
schedule has to be evaluated there: these dataclasses describe one (``to_c()``: the
``mmt_lr_schedule_t`` the library reads at launch) and restate its closed form on the host in
float64 (``__call__``), which is what the tests compare the device value with.

optax mapping (s = the count before the step's advance, as ``optax.scale_by_schedule``):

* ``Constant(v)``: ``optax.constant_schedule(v)``;
* ``WarmupCosine(init, peak, W, T, end)``: ``optax.warmup_cosine_decay_schedule(init, peak, W, T,
  end)`` (T counts the warm-up steps too; the value stays at ``end`` from T on);
* ``WarmupRsqrt(init, peak, W, timescale)``: the Octo recipe, a linear warm-up joined to
  ``peak * sqrt(timescale / (s - W + timescale))``.

The decay of the parameter EMA (AdamW.ema_decay; include/mmt_api.h mmt_adamw_ema) is a schedule of
the same counter and lives here too: ``EmaDecay`` (the diffusers / Diffusion-Policy ``EMAModel``
warm-up) and ``ConstantEmaDecay``, with ``to_c()``: the ``mmt_ema_decay_t``.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

SCHED_CONSTANT, SCHED_WARMUP_COSINE, SCHED_WARMUP_RSQRT = 0, 1, 2  # include/mmt_api.h


class LrSchedule(ctypes.Structure):
    """mmt_lr_schedule_t (include/mmt_api.h)."""
    _fields_ = [("kind", ctypes.c_int), ("init_value", ctypes.c_double),
                ("peak_value", ctypes.c_double), ("end_value", ctypes.c_double),
                ("warmup_steps", ctypes.c_int64), ("decay_steps", ctypes.c_int64),
                ("timescale", ctypes.c_double)]


def _warmup(init: float, peak: float, step: int, warmup: int) -> float:
    return init + (peak - init) * step / warmup


def _check_warmup(name: str, peak: float, warmup: int):
    if warmup < 1:
        raise ValueError(f"{name}: warmup_steps {warmup} < 1")
    if peak == 0:
        raise ValueError(f"{name}: peak_value must not be 0")


@dataclass(frozen=True)
class Constant:
    value: float

    def __call__(self, step: int) -> float:
        return float(self.value)

    def to_c(self) -> LrSchedule:
        return LrSchedule(kind=SCHED_CONSTANT, peak_value=float(self.value))


@dataclass(frozen=True)
class WarmupCosine:
    init_value: float
    peak_value: float
    warmup_steps: int
    decay_steps: int           # total length, the warm-up included
    end_value: float = 0.0

    def __post_init__(self):
        _check_warmup("WarmupCosine", self.peak_value, self.warmup_steps)
        if self.decay_steps <= self.warmup_steps:
            raise ValueError(f"WarmupCosine: decay_steps {self.decay_steps} <= warmup_steps "
                             f"{self.warmup_steps}")

    def __call__(self, step: int) -> float:
        W, T = self.warmup_steps, self.decay_steps
        if step < W:
            return _warmup(self.init_value, self.peak_value, step, W)
        c = min(step - W, T - W)
        alpha = self.end_value / self.peak_value
        cosine = 0.5 * (1.0 + math.cos(math.pi * c / (T - W)))
        return self.peak_value * ((1.0 - alpha) * cosine + alpha)

    def to_c(self) -> LrSchedule:
        return LrSchedule(kind=SCHED_WARMUP_COSINE, init_value=float(self.init_value),
                          peak_value=float(self.peak_value), end_value=float(self.end_value),
                          warmup_steps=int(self.warmup_steps), decay_steps=int(self.decay_steps))


@dataclass(frozen=True)
class WarmupRsqrt:
    init_value: float
    peak_value: float
    warmup_steps: int
    timescale: float

    def __post_init__(self):
        _check_warmup("WarmupRsqrt", self.peak_value, self.warmup_steps)
        if not self.timescale > 0:
            raise ValueError(f"WarmupRsqrt: timescale {self.timescale} <= 0")

    def __call__(self, step: int) -> float:
        W = self.warmup_steps
        if step < W:
            return _warmup(self.init_value, self.peak_value, step, W)
        return self.peak_value * math.sqrt(self.timescale / ((step - W) + self.timescale))

    def to_c(self) -> LrSchedule:
        return LrSchedule(kind=SCHED_WARMUP_RSQRT, init_value=float(self.init_value),
                          peak_value=float(self.peak_value), warmup_steps=int(self.warmup_steps),
                          timescale=float(self.timescale))


Schedule = (Constant, WarmupCosine, WarmupRsqrt)


# ---------------------------------------------------------------------- parameter EMA decay
EMA_CONSTANT, EMA_WARMUP = 0, 1  # include/mmt_api.h MMT_EMA_*


class EmaDecayC(ctypes.Structure):
    """mmt_ema_decay_t (include/mmt_api.h)."""
    _fields_ = [("kind", ctypes.c_int), ("value", ctypes.c_double),
                ("max_value", ctypes.c_double), ("min_value", ctypes.c_double),
                ("inv_gamma", ctypes.c_double), ("power", ctypes.c_double),
                ("update_after_step", ctypes.c_int64)]


def _check_unit(name: str, what: str, v: float):
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{name}: {what} {v} outside [0, 1]")


@dataclass(frozen=True)
class EmaDecay:
    """The decay of the parameter EMA (AdamW.ema_decay), evaluated on the device from the step
    counter (include/mmt_api.h mmt_adamw_ema, MMT_EMA_WARMUP): the warm-up rule of diffusers'
    ``EMAModel(decay=max_value, min_decay=min_value, inv_gamma=, power=, update_after_step=,
    use_ema_warmup=True)`` and of Diffusion Policy's ``EMAModel``. With s the count before the
    step's advance (as the learning-rate schedules take it) and k = max(0, s - update_after_step
    - 1): 0 if k == 0, else min(max_value, max(min_value, 1 - (1 + k / inv_gamma)^-power)).
    ``__call__`` restates it in float64."""
    max_value: float = 0.9999
    min_value: float = 0.0
    inv_gamma: float = 1.0
    power: float = 0.75
    update_after_step: int = 0

    def __post_init__(self):
        _check_unit("EmaDecay", "max_value", self.max_value)
        _check_unit("EmaDecay", "min_value", self.min_value)
        if self.min_value > self.max_value:
            raise ValueError(f"EmaDecay: min_value {self.min_value} > max_value {self.max_value}")
        if not self.inv_gamma > 0:
            raise ValueError(f"EmaDecay: inv_gamma {self.inv_gamma} <= 0")
        if not self.power >= 0:
            raise ValueError(f"EmaDecay: power {self.power} < 0")
        if self.update_after_step < 0:
            raise ValueError(f"EmaDecay: update_after_step {self.update_after_step} < 0")

    def __call__(self, step: int) -> float:
        k = max(0, step - self.update_after_step - 1)
        if k == 0:
            return 0.0
        d = 1.0 - (1.0 + k / self.inv_gamma) ** -self.power
        return min(self.max_value, max(self.min_value, d))

    def to_c(self) -> EmaDecayC:
        return EmaDecayC(kind=EMA_WARMUP, max_value=float(self.max_value),
                         min_value=float(self.min_value), inv_gamma=float(self.inv_gamma),
                         power=float(self.power), update_after_step=int(self.update_after_step))


@dataclass(frozen=True)
class ConstantEmaDecay:
    """A fixed decay in [0, 1] (what a float AdamW.ema_decay becomes): MMT_EMA_CONSTANT."""
    value: float

    def __post_init__(self):
        _check_unit("ConstantEmaDecay", "value", self.value)

    def __call__(self, step: int) -> float:
        return float(self.value)

    def to_c(self) -> EmaDecayC:
        return EmaDecayC(kind=EMA_CONSTANT, value=float(self.value))
