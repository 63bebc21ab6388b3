"""Categorical action head, mirroring the reference's ``action_heads/categorical.py:12-41``
(``assign_bins``: uniform ``linspace`` edges + ``jnp.digitize``; ``CategoricalActionHead``: the
readouts regrouped "batch (action timestep) embeddings -> batch action timestep embeddings",
averaged over timestep, Dense to ``num_bins`` logits) and ``Octo.compute_ce_loss``
(models/octo/octo.py:187-198: ``one_hot(assign_bins(...), num_bins)`` +
``optax.softmax_cross_entropy``) averaged as ``categorical_train_step`` does (:292-302).
SURVEY §8f row 4.

The reference's off-by-one is kept: ``digitize`` returns 1..num_bins for in-range actions and
``one_hot(num_bins, num_bins)`` is all zero, so actions in the top bin (and >= max_action) carry
no loss, and the lowest bin's actions train class 1.

Action chunks: ``horizon`` = h makes the reference's ``action`` axis h A groups, step-major
(group g = step A + a), logits (B, h, A, num_bins). With a chunk or a pad mask the loss runs
``mmt_head_categorical`` (csrc/heads.hip: masked mean, no float atomics, the argmax class of
every group beside it); one action without a mask stays on ``mmt_action_head``. ``decode`` is
the way back from logits to actions (``mmt_head_categorical_decode``: argmax or a draw from
``softmax(z / T)``, through ``bin_values``), which the reference leaves out.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _C, _kernels as K
from ..layers import Dense
from ..params import ParamStore
from .continuous import flat_targets


def assign_bins(input_data: np.ndarray, bounds, num_bins: int, bin_strategy: str = "uniform"):
    """Reference categorical.py:12-22 (host helper, float32 edges like jnp.linspace)."""
    if bin_strategy != "uniform":
        raise NotImplementedError
    bins = np.linspace(bounds[0], bounds[1], num_bins + 1, dtype=np.float32)
    return np.digitize(np.asarray(input_data, dtype=np.float32), bins)


def bin_values(bounds, num_bins: int) -> np.ndarray:
    """The action each class stands for, (num_bins,) float32: the inverse of the labels as
    ``one_hot(assign_bins(y), num_bins)`` trains them. Class c >= 1 holds the targets in
    [edges[c - 1], edges[c]) and decodes to that interval's midpoint; class 0 holds the targets
    below the range and decodes to edges[0] = bounds[0]. (The top interval and everything above
    it is bin num_bins, which has no class: the reference's off-by-one.) Computed in float64 from
    the float32 edges and rounded once."""
    edges = np.linspace(bounds[0], bounds[1], num_bins + 1, dtype=np.float32).astype(np.float64)
    v = np.empty(num_bins, dtype=np.float64)
    v[0] = edges[0]
    v[1:] = 0.5 * (edges[:num_bins - 1] + edges[1:num_bins])
    return v.astype(np.float32)


class CategoricalActionHead:
    MODES = {"argmax": _C.DECODE_ARGMAX, "sample": _C.DECODE_SAMPLE}

    def __init__(self, store: ParamStore, name: str, embedding_dim: int, action_dim: int,
                 num_bins: int, max_action: float, horizon: int = 1):
        if horizon < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        self.D, self.A, self.num_bins, self.max_action = embedding_dim, action_dim, num_bins, float(max_action)
        self.h = int(horizon)
        self.G = self.h * self.A  # readout groups per sample, step-major
        self.name = name  # the prefix of the head's parameters in the store
        self.dense = Dense(store, f"{name}/Dense_0", embedding_dim, num_bins)
        self._edges = {}
        self._values = {}
        self._last = None  # (cls or None, logits, actions, mask) of the latest loss_forward

    def edges(self, device) -> torch.Tensor:
        if device not in self._edges:
            e = np.linspace(-self.max_action, self.max_action, self.num_bins + 1, dtype=np.float32)
            self._edges[device] = torch.from_numpy(e).to(device)
        return self._edges[device]

    def values(self, device) -> torch.Tensor:
        """bin_values on the device."""
        if device not in self._values:
            v = bin_values((-self.max_action, self.max_action), self.num_bins)
            self._values[device] = torch.from_numpy(v).to(device)
        return self._values[device]

    def _shape(self, z: torch.Tensor, B: int) -> torch.Tensor:
        if self.h == 1:
            return z.view(B, self.A, self.num_bins)
        return z.view(B, self.h, self.A, self.num_bins)

    def forward(self, group_means: torch.Tensor) -> torch.Tensor:
        """(B, h A, D) bf16 per-group readout means -> logits fp32 (:38-40): (B, A, num_bins), or
        (B, h, A, num_bins) with a horizon > 1."""
        B = group_means.shape[0]
        z = self.dense.fwd(group_means.reshape(B * self.G, self.D), out_mode=K.OUT_F32)
        return self._shape(z, B)

    def loss_forward(self, group_means: torch.Tensor, actions: torch.Tensor,
                     action_pad_mask: torch.Tensor | None = None):
        """mean over (b, step, a) of softmax_cross_entropy(logits, one_hot(assign_bins(actions)));
        with a bool action_pad_mask (B, h, A) / (B, h A), True where a component is real,
        sum m ce / max(sum m, 1). actions (B, h, A) or (B, h A)."""
        B = group_means.shape[0]
        actions, mask = flat_targets(actions, action_pad_mask, B, self.h, self.A)
        x = group_means.reshape(B * self.G, self.D)
        z = self.dense.fwd(x, out_mode=K.OUT_F32)
        R = B * self.G
        dz = torch.empty((R, self.num_bins), dtype=torch.bfloat16, device=z.device)
        e = self.edges(z.device)
        cls = None
        if self.h == 1 and mask is None:
            loss = torch.zeros(1, dtype=torch.float32, device=z.device)
            _C.call("mmt_action_head", 1, _C.ptr(z), z.stride(0), R, self.num_bins, _C.ptr(actions),
                    _C.ptr(e), e.numel(), self.max_action, 1.0 / R, None, _C.ptr(loss), _C.ptr(dz),
                    _C.stream_ptr())
        else:
            loss = torch.empty(1, dtype=torch.float32, device=z.device)
            scratch = torch.empty(R + 1, dtype=torch.float32, device=z.device)
            cls = torch.empty(R, dtype=torch.int32, device=z.device)
            _C.call("mmt_head_categorical", _C.ptr(z), z.stride(0), R, self.num_bins,
                    _C.ptr(actions), _C.ptr(mask), _C.ptr(e), e.numel(), _C.ptr(scratch),
                    _C.ptr(loss), _C.ptr(dz), _C.ptr(cls), _C.stream_ptr())
        self._last = (cls, z, actions, mask)
        return loss, dict(x=x, dz=dz, B=B)

    def last_accuracy(self) -> torch.Tensor:
        """Accuracy of the latest loss_forward, a 0-d device tensor computed when asked:
        sum m [argmax == label] / max(sum m, 1) over the (b, step, a) groups. A target in bin
        num_bins (the off-by-one: no class) counts as wrong, as it counts in the loss's
        denominator. The argmax is the loss kernel's `cls` where it ran."""
        if self._last is None:
            raise RuntimeError("last_accuracy: no loss_forward has run yet")
        cls, z, actions, mask = self._last
        if cls is None:
            cls = z.argmax(dim=-1)
        # right=True: the number of edges <= y (jnp.digitize)
        label = torch.bucketize(actions.reshape(-1), self.edges(z.device), right=True)
        hit = (cls.long() == label).float()
        if mask is None:
            return hit.mean()
        m = mask.reshape(-1).float()
        return (hit * m).sum() / m.sum().clamp_min(1.0)

    def decode(self, logits: torch.Tensor, rng: torch.Tensor | None = None, sample_offset: int = 0,
               mode: str = "argmax", temperature: float = 1.0):
        """Logits (B, A, N), (B, h, A, N) or flat (B h A, N) fp32 -> (actions (B, h, A) fp32,
        classes (B, h, A) int32). mode "argmax" (the first index on ties) or "sample": one draw per
        group from softmax(logits / temperature) by inverse CDF, keyed by rng = {seed, step} and
        the global sample index sample_offset + b (include/mmt_api.h
        mmt_head_categorical_decode). actions = bin_values[classes]."""
        if mode not in self.MODES:
            raise ValueError(f"mode must be 'argmax' or 'sample', got {mode!r}")
        if mode == "sample" and rng is None:
            raise ValueError("decode: sampling needs rng")
        N = self.num_bins
        if logits.dtype != torch.float32 or logits.shape[-1] != N or logits.numel() % (self.G * N):
            raise ValueError(f"logits must be fp32 (B, {self.h}, {self.A}, {N}), got "
                             f"{tuple(logits.shape)} {logits.dtype}")
        z = logits.reshape(-1, N)
        if z.stride(1) != 1:
            z = z.contiguous()
        R = z.shape[0]
        B = R // self.G
        cls = torch.empty(R, dtype=torch.int32, device=z.device)
        act = torch.empty(R, dtype=torch.float32, device=z.device)
        _C.call("mmt_head_categorical_decode", _C.ptr(z), z.stride(0), R, N, self.G,
                _C.ptr(self.values(z.device)), self.MODES[mode], float(temperature), _C.ptr(rng),
                int(sample_offset), _C.ptr(cls), _C.ptr(act), _C.stream_ptr())
        return act.view(B, self.h, self.A), cls.view(B, self.h, self.A)

    def loss_backward(self, sv: dict) -> torch.Tensor:
        """Returns d(group means) (B, h A, D) bf16."""
        return self.dense.bwd(sv["dz"], sv["x"]).view(sv["B"], self.G, self.D)
