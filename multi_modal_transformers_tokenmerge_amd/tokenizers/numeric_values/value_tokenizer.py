"""Value tokens: low-dimensional numbers (proprioception: joint angles, gripper opening,
end-effector pose, the previous action) as sequence rows, mirroring the reference's
``multi_modal_transformers/tokenizers/numeric_values/value_tokenizer.py`` (ActionTokenizer :18-30,
an ``nn.Embed`` over discrete ids; mu_law_encoder :33-34), Gato style: mu-law companding ->
uniform bins -> one trainable embedding table.

For a value v (fp32, expected normalised to [-1, 1]; there are no bounds parameters), N = num_bins:

    s = fminf(fmaxf(v, -1), 1)                      # clamp; IEEE fmax/fmin send NaN to -1
    y = s                                           # encoding "uniform"
    y = copysign(log1pf(mu*|s|) / log1pf(mu), s)    # encoding "mu_law"
    token = min(N - 1, (int)floorf((y + 1) * 0.5f * N))

so -1, -inf and NaN give token 0, 0 gives N // 2, and 1, +inf and anything above 1 give N - 1.
In the model the row of a value is ``embedding[token] + pos_embedding[row]`` (one fp32 add): the
table is shared by every Value set and slot, the encoder's learned position embedding tells the
slots apart. The kernels are csrc/values.hip (mmt_value_tokens_fwd / _bwd, include/mmt_api.h); no
gradient reaches the values.
"""
from __future__ import annotations

import math

import torch

from ... import _C, _kernels as K
from ...module_api import Bindable
from ...params import ParamStore, normal

ENCODINGS = ("mu_law", "uniform")


def mu_law_encoder(x, mu=255):
    """Reference value_tokenizer.py:33-34, ``sign(x) * log(1 + mu |x|) / log(1 + mu)``, on a torch
    tensor (any device): the host-side helper kept for API parity. The tokenizer's kernel
    evaluates the same formula in fp32 on the clamped value."""
    x = torch.as_tensor(x)
    return torch.sign(x) * torch.log1p(mu * torch.abs(x)) / math.log1p(mu)


def check_value_config(num_bins, mu, encoding):
    """ValueError unless num_bins is an integer in 2 .. 4096, encoding a known name and (mu-law)
    mu finite and > 0."""
    if isinstance(num_bins, bool) or not isinstance(num_bins, int) or \
            not _C.VALUE_MIN_BINS <= num_bins <= _C.VALUE_MAX_BINS:
        raise ValueError(f"num_bins must be an integer in {_C.VALUE_MIN_BINS} .. "
                         f"{_C.VALUE_MAX_BINS}, got {num_bins!r}")
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding must be one of {ENCODINGS}, got {encoding!r}")
    if isinstance(mu, bool) or not isinstance(mu, (int, float)) or \
            (encoding == "mu_law" and not (math.isfinite(mu) and mu > 0)):
        raise ValueError(f"mu must be a finite number > 0, got {mu!r}")


class ValueTokenizer(Bindable):
    """``ValueTokenizer(num_bins=256, mu=255.0, encoding="mu_law")`` owns ``<name>/embedding``
    (num_bins, D) fp32, initialised as Flax ``nn.Embed`` does by default,
    ``variance_scaling(1.0, "fan_in", "normal", out_axis=0)``: normal with std 1 / sqrt(D).
    ``bind(store, name, D)`` declares it in a caller's store (Octo); the first call of an unbound
    module creates a private store, and then needs ``embedding_dim``."""

    def __init__(self, num_bins: int = 256, mu: float = 255.0, encoding: str = "mu_law",
                 embedding_dim: int | None = None):
        check_value_config(num_bins, mu, encoding)
        self.num_bins, self.mu, self.encoding = int(num_bins), float(mu), encoding
        self.D = None if embedding_dim is None else int(embedding_dim)
        self.embedding = None

    def _declare(self, store: ParamStore, name: str, embedding_dim: int):
        self.D = int(embedding_dim)
        self.embedding = store.add(f"{name}/embedding", (self.num_bins, self.D),
                                   normal(1.0 / math.sqrt(self.D)))

    # ------------------------------------------------------------------ the hooks Octo uses
    def forward(self, values: torch.Tensor, rows: torch.Tensor, pe: torch.Tensor,
                x0: torch.Tensor) -> torch.Tensor:
        """values (B, n) fp32, rows (n,) int32: writes x0[b, rows[j]] = embedding[token] +
        pe[rows[j]] (no other row of x0) and returns the (B, n) int32 tokens, the backward's
        saved state."""
        return K.value_tokens_fwd(values, rows, self.embedding.data, pe, x0, self.encoding,
                                  self.mu)

    def backward(self, dx0: torch.Tensor, tok: torch.Tensor, rows: torch.Tensor):
        """embedding.grad[k] += the rows dx0[b, rows[j]] of the tokens equal to k: one fp32
        accumulator per entry, ascending (b, j) order, added once (bitwise reproducible)."""
        K.value_tokens_bwd(dx0, tok, rows, self.embedding.grad)

    # ------------------------------------------------------------------ standalone module form
    def _standalone(self, values: torch.Tensor):
        if not torch.is_tensor(values) or values.dtype != torch.float32 or not values.is_cuda \
                or values.dim() < 1:
            raise ValueError("values must be an fp32 device tensor (..., n)")
        if self.embedding is None and self.D is None:
            raise ValueError("an unbound ValueTokenizer needs embedding_dim")
        self._ensure(values.device, self.D)
        n = values.shape[-1]
        v2 = values.reshape(-1, n).contiguous()
        dev = values.device
        out = torch.empty((v2.shape[0], n, self.D), dtype=torch.float32, device=dev)
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        zero = torch.zeros((n, self.D), dtype=torch.float32, device=dev)  # no position term
        tok = self.forward(v2, rows, zero, out)
        return tok.view(values.shape), out.view(*values.shape, self.D)

    def tokens(self, values: torch.Tensor) -> torch.Tensor:
        """The int32 tokens of ``values`` (..., n), the same shape."""
        return self._standalone(values)[0]

    def __call__(self, values: torch.Tensor) -> torch.Tensor:
        """(..., n) fp32 -> (..., n, D) fp32: the table rows alone, no position term."""
        return self._standalone(values)[1]
