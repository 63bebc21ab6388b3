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
