"""GPU: the attention-pooling kernels of csrc/pool.hip against float64 torch on the same
(bf16-rounded) inputs: the readout gather / scatter pair (exact), the single-query attention core
forward and backward, and the feature-axis LayerNorm forward and backward.

Bars: p rtol 1e-5 / atol 1e-6 (the fp32 per-op bar); the bf16 outputs ctx, dk, dv and
the LayerNorm y 1e-2 / 1e-2 (one bf16 rounding is 2^-9 = 2e-3 relative); the fp32 dqb, dx and
dy * xhat rows rtol 1e-4 / atol 1e-5; mean rtol 1e-5; rstd rtol 1e-4 (at mean 4 the fast
variance's fp32 cancellation error is about 1e-5 of the variance)."""
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("D,rows", [(64, [1, 2, 8, 9]), (192, [5])], ids=["D64-n4", "D192-n1"])
def test_rows_gather_scatter_exact(dev, D, rows):
    B, L = 3, 11
    n = len(rows)
    g = _gen(D)
    # x inside a wider buffer: row stride > D, sample stride > L * row stride
    xs_t, xs_b = D + 8, (L + 2) * (D + 8)
    buf = torch.randn((B * xs_b,), generator=g).to(dev)
    x = torch.as_strided(buf, (B, L, D), (xs_b, xs_t, 1))
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    r = K.rows_gather_bf16(x, rows_d)
    assert r.shape == (B, n, D) and r.dtype == torch.bfloat16
    assert torch.equal(r, x[:, rows, :].to(torch.bfloat16))
    flag = torch.full((L,), -1, dtype=torch.int32)
    flag[rows] = torch.arange(n, dtype=torch.int32)
    dr = torch.randn((B, n, D), generator=g).to(torch.bfloat16).to(dev)
    dx = torch.full((B, L, D), float("nan"), device=dev)       # the kernel writes every element
    K.rows_scatter_bwd(dr, flag.to(dev), out=dx)
    want = torch.zeros((B, L, D), device=dev)
    want[:, rows, :] = dr.float()
    assert torch.equal(dx, want)
    K.device_status()


def test_rows_index_out_of_range_is_reported(dev):
    """A row index past L is replaced by row 0 and recorded (mmt_device_status), never read."""
    x = torch.randn((2, 5, 64), device=dev)
    r = K.rows_gather_bf16(x, torch.tensor([1, 7], dtype=torch.int32, device=dev))
    with pytest.raises(_C.MMTError):
        K.device_status()
    assert torch.equal(r[:, 1], x[:, 0].to(torch.bfloat16))
    K.device_status()  # cleared


# ------------------------------------------------------------------ the attention core
POOL_SHAPES = [(1, 1, 1, 64), (3, 4, 3, 64), (2, 5, 3, 256), (5, 8, 12, 64), (2, 64, 6, 64)]


def _pool_inputs(dev, B, n, H, Dh, split, qscale=1.0, seed=0):
    D = H * Dh
    g = _gen(1000 * B + 10 * n + H + 100000 * seed)
    q = (torch.randn(D, generator=g) * (Dh ** -0.5) * qscale).to(dev)
    kv = torch.randn((B * n, 2 * D), generator=g).to(torch.bfloat16).to(dev)
    if split:     # the two halves of one (B n, 2 D) buffer
        k, v = kv[:, :D], kv[:, D:]
    else:
        k, v = kv[:, :D].contiguous(), kv[:, D:].contiguous()
    dctx = torch.randn((B, D), generator=g).to(torch.bfloat16).to(dev)
    return q, k, v, dctx


def _pool_ref(q, k, v, dctx, B, n, H, Dh):
    q6 = q.double().view(H, Dh)
    k6 = k.double().view(B, n, H, Dh)
    v6 = v.double().view(B, n, H, Dh)
    d6 = dctx.double().view(B, H, Dh)
    s = torch.einsum("hd,bjhd->bhj", q6, k6)
    p = torch.softmax(s, dim=-1)
    ctx = torch.einsum("bhj,bjhd->bhd", p, v6)
    dv = torch.einsum("bhj,bhd->bjhd", p, d6)
    dp = torch.einsum("bhd,bjhd->bhj", d6, v6)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dk = torch.einsum("bhj,hd->bjhd", ds, q6)
    dqb = torch.einsum("bhj,bjhd->bhd", ds, k6)
    D = H * Dh
    return (p, ctx.reshape(B, D), dk.reshape(B * n, D), dv.reshape(B * n, D), dqb.reshape(B, D))


@pytest.mark.parametrize("split", [False, True], ids=["contiguous", "kv-halves"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "B%d-n%d-H%d-Dh%d" % s)
def test_attn_pool_core(dev, shape, split):
    B, n, H, Dh = shape
    q, k, v, dctx = _pool_inputs(dev, B, n, H, Dh, split)
    p_r, ctx_r, dk_r, dv_r, dqb_r = _pool_ref(q, k, v, dctx, B, n, H, Dh)
    ctx, p = K.attn_pool_fwd(q, k, v, B, n, H)
    dk, dv, dqb = K.attn_pool_bwd(dctx, p, q, k, v)
    torch.cuda.synchronize()
    print(f"p max abs err {float((p.double() - p_r).abs().max()):.3e}, "
          f"dqb max abs err {float((dqb.double() - dqb_r).abs().max()):.3e}")
    torch.testing.assert_close(p.double(), p_r, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ctx.double(), ctx_r, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(dv.double(), dv_r, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(dk.double(), dk_r, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(dqb.double(), dqb_r, rtol=1e-4, atol=1e-5)
    if split:   # dk / dv are the halves of one (B n, 2 D) buffer, the kv GEMM's dY
        assert dk.stride(0) == 2 * H * Dh and dv.data_ptr() == dk.data_ptr() + 2 * H * Dh


def test_attn_pool_large_scores_stay_finite(dev):
    """q scaled by 30: scores reach the hundreds; the max-subtracted softmax stays finite and
    every row of p sums to 1."""
    B, n, H, Dh = 2, 64, 6, 64
    for seed in range(64):   # scores ~ N(0, 30^2): the first draw whose largest score passes 100,
        #                      where exp() without the max subtraction overflows fp32 (> 88.7)
        q, k, v, dctx = _pool_inputs(dev, B, n, H, Dh, True, qscale=30.0, seed=seed)
        s = torch.einsum("hd,bjhd->bhj", q.double().view(H, Dh), k.double().view(B, n, H, Dh))
        if float(s.max()) > 100.0:
            break
    assert float(s.max()) > 100.0
    ctx, p = K.attn_pool_fwd(q, k, v, B, n, H)
    dk, dv, dqb = K.attn_pool_bwd(dctx, p, q, k, v)
    for t in (ctx, p, dk, dv, dqb):
        assert bool(torch.isfinite(t.float()).all())
    torch.testing.assert_close(p.sum(-1), torch.ones((B, H), device=dev), rtol=0, atol=1e-5)
    # the winner of each row is the reference's
    assert torch.equal(p.argmax(-1).cpu(), s.argmax(-1).cpu())


def test_attn_pool_argument_errors(dev):
    """n = 65, Dh = 60 and a null output are argument errors: MMTError, nothing launched."""
    B, H = 2, 2
    for n, Dh in ((65, 64), (4, 60)):
        D = H * Dh
        q = torch.zeros(D, device=dev)
        kv = torch.zeros((B * n, D), dtype=torch.bfloat16, device=dev)
        with pytest.raises(_C.MMTError, match="mmt_attn_pool_fwd"):
            K.attn_pool_fwd(q, kv, kv, B, n, H)
        p = torch.zeros((B, H, n), device=dev)
        dctx = torch.zeros((B, D), dtype=torch.bfloat16, device=dev)
        with pytest.raises(_C.MMTError, match="mmt_attn_pool_bwd"):
            K.attn_pool_bwd(dctx, p, q, kv, kv)
    n, Dh = 4, 64
    D = H * Dh
    q = torch.zeros(D, device=dev)
    kv = torch.zeros((B * n, D), dtype=torch.bfloat16, device=dev)
    p = torch.zeros((B, H, n), device=dev)
    with pytest.raises(_C.MMTError, match="null"):
        _C.call("mmt_attn_pool_fwd", _C.ptr(q), _C.ptr(kv), _C.ptr(kv), D, B, n, H, Dh, None, D,
                _C.ptr(p), _C.stream_ptr())
    torch.cuda.synchronize()
    K.device_status()


# ------------------------------------------------------------------ feature-axis LayerNorm
LN_SHAPES = [(1, 64), (37, 192), (5, 768)]
EPS = 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "B%d-D%d" % s)
def test_feature_layernorm(dev, shape, dtype):
    B, D = shape
    g = _gen(B * D)
    x = (4.0 + torch.randn((B, D), generator=g)).to(dtype).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev)
    beta = (0.1 * torch.randn(D, generator=g)).to(dev)
    dy = torch.randn((B, D), generator=g).to(dtype).to(dev)
    addend = torch.randn((B, D), generator=g).to(dtype).to(dev)
    y, mean, rstd = K.layernorm_fwd(x, gamma, beta, EPS)
    dx, dyxh = K.layernorm_bwd(dy, x, mean, rstd, gamma, addend=addend)
    dx0, _ = K.layernorm_bwd(dy, x, mean, rstd, gamma)
    torch.cuda.synchronize()
    # flax.linen.LayerNorm's formula in float64 on the same inputs
    x6, g6, b6 = x.double(), gamma.double(), beta.double()
    mu = x6.mean(-1)
    var = torch.clamp((x6 * x6).mean(-1) - mu * mu, min=0.0)
    rs = torch.rsqrt(var + EPS)
    y_r = (x6 - mu[:, None]) * (rs[:, None] * g6) + b6
    torch.testing.assert_close(mean.double(), mu, rtol=1e-5, atol=0)
    torch.testing.assert_close(rstd.double(), rs, rtol=1e-4, atol=0)
    torch.testing.assert_close(y.double(), y_r, rtol=1e-2, atol=1e-2)
    # the backward from the statistics it is given (the saved fp32 mean / rstd)
    m6, r6 = mean.double()[:, None], rstd.double()[:, None]
    xh = (x6 - m6) * r6
    gg = dy.double() * g6
    dx_r = r6 * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    tol = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    assert dx.dtype == dtype and dyxh.dtype == torch.float32
    torch.testing.assert_close(dx0.double(), dx_r, **tol)
    torch.testing.assert_close(dx.double(), dx_r + addend.double(), **tol)
    torch.testing.assert_close(dyxh.double(), dy.double() * xh, rtol=1e-4, atol=1e-5)


def test_feature_layernorm_strided_rows(dev):
    """Row strides wider than D on every operand (views into wider buffers)."""
    B, D, ld = 6, 64, 136
    g = _gen(7)
    wide = lambda: torch.randn((B, ld), generator=g).to(torch.bfloat16).to(dev)   # noqa: E731
    xb, dyb, ab = wide(), wide(), wide()
    x, dy, ad = xb[:, 8:8 + D], dyb[:, 16:16 + D], ab[:, 72:72 + D]
    gamma = torch.ones(D, device=dev)
    beta = torch.zeros(D, device=dev)
    outb = torch.zeros((B, ld), dtype=torch.bfloat16, device=dev)
    y, mean, rstd = K.layernorm_fwd(x, gamma, beta, EPS, out=outb[:, 64:64 + D])
    y2, mean2, rstd2 = K.layernorm_fwd(x.contiguous(), gamma, beta, EPS)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    assert not outb[:, :64].any() and not outb[:, 64 + D:].any()
    dx, dyxh = K.layernorm_bwd(dy, x, mean, rstd, gamma, addend=ad)
    dx2, dyxh2 = K.layernorm_bwd(dy.contiguous(), x.contiguous(), mean, rstd, gamma,
                                 addend=ad.contiguous())
    assert torch.equal(dx, dx2) and torch.equal(dyxh, dyxh2)
