"""Torch restatement of QK-norm (flax.linen.SelfAttention(normalize_qk=True): LayerNorm(
use_bias=False) over the head dimension of the projected queries and keys, `query_ln` / `key_ln`),
in the dtype of its inputs (float64 as the reference of the tests, float32 as the yardstick of the
kernels' own rounding) and differentiable by autograd. Flax's fast variance, the form the kernels
use: var = max(0, mean(x^2) - mean(x)^2)."""
import torch


def head_layernorm(x: torch.Tensor, scale: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """x (..., Dh), scale (Dh,): (x - mu) * rsqrt(var + eps) * scale over the last axis."""
    mu = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mu * mu).clamp_min(0)
    return (x - mu) * torch.rsqrt(var + eps) * scale


def qk_norm(qkv: torch.Tensor, H: int, q_scale: torch.Tensor, k_scale: torch.Tensor,
            eps: float = 1e-6) -> torch.Tensor:
    """qkv (..., 3 H Dh), the packed (3, H, Dh) projection: q and k normalised per head, v as is."""
    lead = qkv.shape[:-1]
    q, k, v = qkv.reshape(*lead, 3, H, -1).unbind(-3)
    out = torch.stack([head_layernorm(q, q_scale, eps), head_layernorm(k, k_scale, eps), v], dim=-3)
    return out.reshape(*lead, -1)


def head_layernorm_bwd(x: torch.Tensor, scale: torch.Tensor, dy: torch.Tensor, eps: float = 1e-6):
    """The closed form of the backward, away from the clamp: (dx, dscale) with
    g = dy * scale, dx = rs * (g - mean(g) - xhat * mean(g * xhat)), dscale = sum of dy * xhat over
    every axis but the last."""
    mu = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mu * mu).clamp_min(0)
    rs = torch.rsqrt(var + eps)
    xhat = (x - mu) * rs
    g = dy * scale
    dx = rs * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).reshape(-1, x.shape[-1]).sum(0)
