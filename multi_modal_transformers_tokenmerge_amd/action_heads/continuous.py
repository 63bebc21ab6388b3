"""Continuous action head, mirroring the reference's ``action_heads/continuous.py:12-26``
(``ContinuousActionHead``: mean over the readouts, Dense, ``tanh(mean / max_action) * max_action``)
and the L2 objective of ``Octo.compute_l2_loss`` (models/octo/octo.py:167-174) averaged over the
batch as ``continuous_train_step`` does (:252-262). SURVEY §8f row 4.

Device path: the readout mean comes from the backbone's fused rows-mean kernel, the Dense is the
library GEMM (fp32 output), and one kernel (``mmt_action_head`` kind 0) applies the tanh squash,
the loss and its gradient.

Action chunks: the reference reshapes the Dense output as ``"batch (seq mean) -> batch seq mean"``
with ``seq=1`` (:24); ``horizon`` gives ``seq`` its general value h, so the Dense is D -> h A and
the prediction (B, h, A). With a chunk, a pad mask or the L1 loss (``loss="l1"``, upstream Octo's
default regression loss) the head runs ``mmt_head_continuous`` (csrc/heads.hip): the masked loss
``A / max(sum m, 1) sum m e`` without float atomics. One action, no mask and the squared error stay
on ``mmt_action_head``.
"""
from __future__ import annotations

import torch

from .. import _C, _kernels as K
from ..layers import Dense
from ..params import ParamStore


def chunk_flat(x: torch.Tensor, h: int, a: int, what: str = "actions") -> torch.Tensor:
    """An action chunk (B, h, a), or the already flat (B, h a), as (B, h a). A flat tensor is
    returned as it is."""
    if x.dim() == 3:
        if tuple(x.shape[1:]) != (h, a):
            raise ValueError(f"{what} must be (B, {h}, {a}) or (B, {h * a}), got {tuple(x.shape)}")
        return x.reshape(x.shape[0], h * a)
    if x.dim() != 2 or x.shape[1] != h * a:
        raise ValueError(f"{what} must be (B, {h}, {a}) or (B, {h * a}), got {tuple(x.shape)}")
    return x


def flat_targets(actions, mask, B: int, h: int, a: int):
    """The heads' view of targets and pad mask: actions fp32 contiguous (B, h a); mask None or
    uint8 contiguous (B, h a) from a bool tensor of either chunk form."""
    actions = chunk_flat(actions, h, a)
    if actions.shape[0] != B or actions.dtype != torch.float32 or not actions.is_contiguous():
        raise ValueError(f"actions must be contiguous fp32 ({B}, {h * a})")
    if mask is not None:
        if mask.dtype != torch.bool:
            raise ValueError("action_pad_mask must be a bool tensor")
        mask = chunk_flat(mask, h, a, "action_pad_mask")
        if mask.shape[0] != B:
            raise ValueError("action_pad_mask and actions differ in batch size")
        mask = mask.contiguous().view(torch.uint8)  # a bool is one byte, 0 / 1: no copy
    return actions, mask


class ContinuousActionHead:
    LOSSES = {"mse": _C.HEAD_LOSS_MSE, "l1": _C.HEAD_LOSS_L1}

    def __init__(self, store: ParamStore, name: str, embedding_dim: int, action_dim: int,
                 max_action: float, horizon: int = 1, loss: str = "mse"):
        if horizon < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        if loss not in self.LOSSES:
            raise ValueError(f"loss must be 'mse' or 'l1', got {loss!r}")
        self.D, self.A, self.max_action = embedding_dim, action_dim, float(max_action)
        self.h, self.loss = int(horizon), loss
        self.W = self.h * self.A
        self.name = name  # the prefix of the head's parameters in the store
        self.dense = Dense(store, f"{name}/Dense_0", embedding_dim, self.W)

    def forward(self, readout_mean: torch.Tensor) -> torch.Tensor:
        """(B, D) bf16 -> actions (B, h, A) fp32 (:23-26)."""
        z = self.dense.fwd(readout_mean, out_mode=K.OUT_F32)
        B = z.shape[0]
        pred = torch.empty((B, self.W), dtype=torch.float32, device=z.device)
        if self.h == 1:
            _C.call("mmt_action_head", 0, _C.ptr(z), z.stride(0), B, self.A, None, None, 0,
                    self.max_action, 1.0, _C.ptr(pred), None, None, _C.stream_ptr())
        else:
            _C.call("mmt_head_continuous", _C.ptr(z), z.stride(0), B, self.h, self.A, None, None,
                    self.LOSSES[self.loss], self.max_action, _C.ptr(pred), None, None, None,
                    _C.stream_ptr())
        return pred.view(B, self.h, self.A)

    def loss_forward(self, readout_mean: torch.Tensor, actions: torch.Tensor,
                     action_pad_mask: torch.Tensor | None = None):
        """mean over (b, step) of sum_a (pred - actions)^2 (octo.py:171-174, :262), or of
        |pred - actions| with loss "l1"; with a bool action_pad_mask (B, h, A) / (B, h A), True
        where a component is real, A / max(sum m, 1) sum m e. actions (B, h, A) or (B, h A).
        Returns (loss (1,), saved)."""
        z = self.dense.fwd(readout_mean, out_mode=K.OUT_F32)
        B = z.shape[0]
        actions, mask = flat_targets(actions, action_pad_mask, B, self.h, self.A)
        dz = torch.empty((B, self.W), dtype=torch.bfloat16, device=z.device)
        if self.h == 1 and mask is None and self.loss == "mse":
            loss = torch.zeros(1, dtype=torch.float32, device=z.device)
            _C.call("mmt_action_head", 0, _C.ptr(z), z.stride(0), B, self.A, _C.ptr(actions), None,
                    0, self.max_action, 1.0 / B, None, _C.ptr(loss), _C.ptr(dz), _C.stream_ptr())
        else:
            loss = torch.empty(1, dtype=torch.float32, device=z.device)
            scratch = torch.empty(B + 1, dtype=torch.float32, device=z.device)
            _C.call("mmt_head_continuous", _C.ptr(z), z.stride(0), B, self.h, self.A,
                    _C.ptr(actions), _C.ptr(mask), self.LOSSES[self.loss], self.max_action, None,
                    _C.ptr(scratch), _C.ptr(loss), _C.ptr(dz), _C.stream_ptr())
        return loss, dict(x=readout_mean, dz=dz)

    def loss_backward(self, sv: dict) -> torch.Tensor:
        """Returns d(readout mean) (B, D) bf16."""
        return self.dense.bwd(sv["dz"], sv["x"])
