"""Float reference of the reference's MultiHeadAttentionPooling (attention_blocks/attention.py
:122-150) in torch, written from the Flax semantics (not from the build's kernels):

1. probe = learnt_q_input (1, 1, D), tiled over the batch;
2. a = flax.linen.MultiHeadDotProductAttention(num_heads=H)(probe, x): query / key / value
   DenseGeneral(D -> (H, Dh)) with bias, q / sqrt(Dh), softmax over the n keys, no mask, no
   dropout, out DenseGeneral((H, Dh) -> D) with bias;
3. y = flax.linen.LayerNorm(epsilon, reduction_axes)(a): fast variance max(0, E[x^2] - E[x]^2),
   y = (a - mean) * (rsqrt(var + eps) * scale) + bias (scale / bias over the feature axis);
4. y = MLPBlock(y): Dense -> relu -> Dense, dropouts off (the head calls it without train);
5. a + y, shape (B, 1, D).

Parameters come as a dict in the FLAX layouts (the checkpoint tree's leaves): kernels (in, out),
query / key / value kernels (D, H, Dh) with (H, Dh) biases, the out kernel (H, Dh, D). Everything
is differentiable under torch autograd and runs in the dtype of ``x``.

``storage`` (optional) is applied to every activation a bf16 compute policy keeps in bf16 between
its products: the key / value projections, the pooled context, the attention output a, the
LayerNorm output, the MLP hidden layer and the result. ``bf16_storage`` rounds to bf16 with a
straight-through gradient, the way oracle/octo_ref.py emulates the build's storage points: a relu
unit whose pre-activation lies within one bf16 rounding of zero is then gated the same way on
both sides (in float64 a handful of the B x hidden units flip, which alone costs the gradients
about 3e-2 relative at B = 5: see tests/test_attn_pool_model_gpu.py).
"""
import math

import torch

MHA = "MultiHeadDotProductAttention_0"


def layer_norm(a, scale, bias, eps, axes):
    mean = a.mean(dim=axes, keepdim=True)
    mean2 = (a * a).mean(dim=axes, keepdim=True)
    var = torch.clamp(mean2 - mean * mean, min=0.0)
    return (a - mean) * (torch.rsqrt(var + eps) * scale) + bias


class _RoundBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def bf16_storage(t):
    """Round to bf16 (nearest even), identity gradient."""
    return _RoundBF16.apply(t)


def attention_pool(x, P, eps=1e-6, axes=(-1,), storage=None):
    """x (B, n, D); P: {flax leaf path under the module: tensor}. Returns (out (B, 1, D), aux) with
    aux = dict(p (B, H, n), ctx (B, H * Dh), a (B, 1, D), y (B, 1, D) the LayerNorm output)."""
    st = storage or (lambda t: t)
    B, n, D = x.shape
    wq = P[f"{MHA}/query/kernel"]
    H, Dh = wq.shape[1], wq.shape[2]
    probe = P["learnt_q_input"].expand(B, 1, D)
    q = torch.einsum("bqd,dhk->bqhk", probe, wq) + P[f"{MHA}/query/bias"]
    k = st(torch.einsum("bjd,dhk->bjhk", x, P[f"{MHA}/key/kernel"]) + P[f"{MHA}/key/bias"])
    v = st(torch.einsum("bjd,dhk->bjhk", x, P[f"{MHA}/value/kernel"]) + P[f"{MHA}/value/bias"])
    q = q / math.sqrt(Dh)
    s = torch.einsum("bqhk,bjhk->bhqj", q, k)
    p = torch.softmax(s, dim=-1)
    ctx = st(torch.einsum("bhqj,bjhk->bqhk", p, v))
    a = st(torch.einsum("bqhk,hkd->bqd", ctx, P[f"{MHA}/out/kernel"]) + P[f"{MHA}/out/bias"])
    y = st(layer_norm(a, P["LayerNorm_0/scale"], P["LayerNorm_0/bias"], eps, tuple(axes)))
    h = st(torch.relu(y @ P["MLPBlock_0/Dense_0/kernel"] + P["MLPBlock_0/Dense_0/bias"]))
    m = h @ P["MLPBlock_0/Dense_1/kernel"] + P["MLPBlock_0/Dense_1/bias"]
    return st(a + m), dict(p=p[:, :, 0, :], ctx=ctx.reshape(B, H * Dh), a=a, y=y)


def random_params(D, H, M=None, seed=0, dtype=torch.float64):
    """A random parameter dict in the Flax layouts (hand cases of the CPU tests)."""
    g = torch.Generator().manual_seed(seed)
    M = M or D
    Dh = D // H

    def r(*shape, s=1.0):
        return (torch.randn(shape, generator=g, dtype=torch.float64) * s).to(dtype)
    return {
        "learnt_q_input": r(1, 1, D),
        f"{MHA}/query/kernel": r(D, H, Dh, s=D ** -0.5), f"{MHA}/query/bias": r(H, Dh, s=0.1),
        f"{MHA}/key/kernel": r(D, H, Dh, s=D ** -0.5), f"{MHA}/key/bias": r(H, Dh, s=0.1),
        f"{MHA}/value/kernel": r(D, H, Dh, s=D ** -0.5), f"{MHA}/value/bias": r(H, Dh, s=0.1),
        f"{MHA}/out/kernel": r(H, Dh, D, s=D ** -0.5), f"{MHA}/out/bias": r(D, s=0.1),
        "LayerNorm_0/scale": 1.0 + r(D, s=0.1), "LayerNorm_0/bias": r(D, s=0.1),
        "MLPBlock_0/Dense_0/kernel": r(D, M, s=D ** -0.5), "MLPBlock_0/Dense_0/bias": r(M, s=0.1),
        "MLPBlock_0/Dense_1/kernel": r(M, D, s=M ** -0.5), "MLPBlock_0/Dense_1/bias": r(D, s=0.1),
    }


def module_params(module, dtype=torch.float64, shadow=True):
    """A bound MultiHeadAttentionPooling's weights as the Flax-layout dict, as leaf tensors that
    require grad. shadow: the bf16 shadows the GEMMs read (the fp32 masters of the biases and the
    LayerNorm parameters, which the kernels read in fp32), so both sides compute with the same
    numbers."""
    D, H, Dh = module.D, module.H, module.Dh

    def w(p, master=False):
        t = p.data if (master or not shadow) else p.bf16
        return t.detach().to(dtype)
    kvw, kvb = w(module.kv.w), module.kv.b.data.detach().to(dtype)
    P = {
        "learnt_q_input": w(module.probe),
        f"{MHA}/query/kernel": w(module.query.w).t().reshape(D, H, Dh),
        f"{MHA}/query/bias": w(module.query.b, True).reshape(H, Dh),
        f"{MHA}/key/kernel": kvw[:D].t().reshape(D, H, Dh), f"{MHA}/key/bias": kvb[:D].reshape(H, Dh),
        f"{MHA}/value/kernel": kvw[D:].t().reshape(D, H, Dh), f"{MHA}/value/bias": kvb[D:].reshape(H, Dh),
        f"{MHA}/out/kernel": w(module.out.w).t().reshape(H, Dh, D),
        f"{MHA}/out/bias": w(module.out.b, True),
        "LayerNorm_0/scale": w(module.ln.scale, True), "LayerNorm_0/bias": w(module.ln.bias, True),
        "MLPBlock_0/Dense_0/kernel": w(module.mlp.dense.w).t(),
        "MLPBlock_0/Dense_0/bias": w(module.mlp.dense.b, True),
        "MLPBlock_0/Dense_1/kernel": w(module.mlp.dense_out.w).t(),
        "MLPBlock_0/Dense_1/bias": w(module.mlp.dense_out.b, True),
    }
    return {k: v.contiguous().clone().requires_grad_(True) for k, v in P.items()}


def grads_as_module(P, module):
    """The autograd gradients of a module_params dict in the module's own layouts:
    {store parameter name: tensor}."""
    D = module.D
    name = module._name
    a = f"{name}/{MHA}"
    g = {k: v.grad for k, v in P.items()}
    return {
        f"{name}/learnt_q_input": g["learnt_q_input"],
        f"{a}/query/kernel": g[f"{MHA}/query/kernel"].reshape(D, D).t(),
        f"{a}/query/bias": g[f"{MHA}/query/bias"].reshape(D),
        f"{a}/kv/kernel": torch.cat([g[f"{MHA}/key/kernel"].reshape(D, D).t(),
                                     g[f"{MHA}/value/kernel"].reshape(D, D).t()], 0),
        f"{a}/kv/bias": torch.cat([g[f"{MHA}/key/bias"].reshape(D), g[f"{MHA}/value/bias"].reshape(D)]),
        f"{a}/out/kernel": g[f"{MHA}/out/kernel"].reshape(D, D).t(),
        f"{a}/out/bias": g[f"{MHA}/out/bias"],
        f"{name}/LayerNorm_0/scale": g["LayerNorm_0/scale"],
        f"{name}/LayerNorm_0/bias": g["LayerNorm_0/bias"],
        f"{name}/MLPBlock_0/Dense_0/kernel": g["MLPBlock_0/Dense_0/kernel"].t(),
        f"{name}/MLPBlock_0/Dense_0/bias": g["MLPBlock_0/Dense_0/bias"],
        f"{name}/MLPBlock_0/Dense_1/kernel": g["MLPBlock_0/Dense_1/kernel"].t(),
        f"{name}/MLPBlock_0/Dense_1/bias": g["MLPBlock_0/Dense_1/bias"],
    }
