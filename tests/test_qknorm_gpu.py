"""GPU: the QK-norm kernels (csrc/qknorm.hip: mmt_qk_norm_fwd / mmt_qk_norm_bwd) against the torch
restatement tests/qknorm_ref.py.

The bars are measured per case, not chosen: the float64 restatement, fed the same (bf16-rounded
where applicable) inputs, is the reference, and the restatement in float32 is the yardstick.
  fp32: the kernel's relative L2 error <= 4 x that of the float32 restatement (summation order);
  bf16: <= 1.5 x that of the float32 restatement rounded to bf16, + 1e-6.
The same form holds for y, dx and the two scale gradients (fp32 outputs in both cases, so they take
the fp32 form). Inputs have mean 8 and unit spread, so the fast variance mean(x^2) - mean(x)^2
cancels six bits in float32. Every case prints its figures. The V third, the pad columns of a padded
row stride and qk_pre are compared bit for bit, and two backward runs must agree bit for bit."""
import functools

import pytest
import torch

from tests import qknorm_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
ROWS = {1: (1, 1), 26: (2, 13), 257: (1, 257)}          # token rows -> (B, L)
GRID = [(dt, Dh, H, rows, 0) for dt in DTYPES for Dh in (32, 64, 128, 256) for H in (1, 3)
        for rows in ROWS]
GRID += [(dt, 64, 3, 26, 8) for dt in DTYPES]           # a padded row stride: ld = 3 H Dh + 8
EPS = 1e-6


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def run_case(dt, Dh, H, rows, pad):
    """Forward and backward of one case on the device, and its references: a dict of tensors."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    dev = torch.device("cuda:0")
    dtype = DTYPES[dt]
    B, L = ROWS[rows]
    W, ld = 3 * H * Dh, 3 * H * Dh + pad
    g = torch.Generator().manual_seed(1000 * Dh + 10 * rows + H)
    x = (torch.randn((B, L, ld), generator=g) + 8.0).to(dtype)        # mean 8, unit spread
    dy = torch.randn((B, L, ld), generator=g).to(dtype)
    qs, ks = torch.rand(Dh, generator=g) + 0.5, torch.rand(Dh, generator=g) * 1.5 + 0.25
    g0q, g0k = torch.randn(Dh, generator=g), torch.randn(Dh, generator=g)   # gradients so far
    out = dict(x=x, dy=dy, W=W, g0q=g0q, g0k=g0k)
    # ---- device
    buf = x.to(dev)
    pre = K.qk_norm_fwd(buf[..., :W], H, Dh, qs.to(dev), ks.to(dev), EPS)
    out["y"], out["pre"] = buf.cpu(), pre.cpu()
    for run in (0, 1):
        dbuf, dq, dk = dy.to(dev), g0q.to(dev), g0k.to(dev)
        K.qk_norm_bwd(dbuf[..., :W], pre, H, Dh, qs.to(dev), ks.to(dev), dq, dk, EPS)
        out[f"dx{run}"], out[f"dq{run}"], out[f"dk{run}"] = dbuf.cpu(), dq.cpu(), dk.cpu()
    torch.cuda.synchronize()
    K.device_status()
    # ---- references: float64 and float32 restatements on the same inputs
    for name, ft in (("64", torch.float64), ("32", torch.float32)):
        xr = x[..., :W].to(ft).requires_grad_()
        qr, kr = qs.to(ft).requires_grad_(), ks.to(ft).requires_grad_()
        y = R.qk_norm(xr, H, qr, kr, EPS)
        y.backward(dy[..., :W].to(ft))
        out["y" + name], out["dx" + name] = y.detach(), xr.grad
        out["dq" + name], out["dk" + name] = qr.grad, kr.grad
    return out


def bar(dt, got, r32, r64, out_dtype):
    """(kernel error, yardstick error, allowed) in the form of the output's dtype."""
    ek = rel(got, r64)
    if out_dtype == torch.bfloat16:
        er = rel(r32.to(torch.bfloat16), r64)
        return ek, er, 1.5 * er + 1e-6
    er = rel(r32, r64)
    return ek, er, 4.0 * er


@pytest.mark.parametrize("dt,Dh,H,rows,pad", GRID)
def test_forward(dev, dt, Dh, H, rows, pad):
    c = run_case(dt, Dh, H, rows, pad)
    W, x, y = c["W"], c["x"], c["y"]
    qk = 2 * H * Dh
    ek, er, allowed = bar(dt, y[..., :qk], c["y32"][..., :qk], c["y64"][..., :qk], DTYPES[dt])
    print(f"\nfwd {dt} Dh {Dh} H {H} rows {rows} pad {pad}: kernel {ek:.3e} yardstick {er:.3e} "
          f"allowed {allowed:.3e}")
    assert torch.equal(y[..., qk:], x[..., qk:])                   # V and the pad columns: bits
    assert torch.equal(c["pre"].view(*x.shape[:2], qk), x[..., :qk])
    assert torch.isfinite(y.float()).all()
    assert ek <= allowed, (ek, er)


@pytest.mark.parametrize("dt,Dh,H,rows,pad", GRID)
def test_backward(dev, dt, Dh, H, rows, pad):
    c = run_case(dt, Dh, H, rows, pad)
    dy, dx = c["dy"], c["dx0"]
    qk = 2 * H * Dh
    assert torch.equal(dx[..., qk:], dy[..., qk:])                 # V and the pad columns: bits
    for k in ("dx", "dq", "dk"):
        assert torch.equal(c[k + "0"], c[k + "1"]), f"{k}: two runs differ"
    bad = []
    rows_ = [("dx", dx[..., :qk], c["dx32"][..., :qk], c["dx64"][..., :qk], DTYPES[dt]),
             # added onto the gradient so far, not overwriting it: the sum is what is compared
             ("dq_scale", c["dq0"], c["g0q"] + c["dq32"], c["g0q"].double() + c["dq64"],
              torch.float32),
             ("dk_scale", c["dk0"], c["g0k"] + c["dk32"], c["g0k"].double() + c["dk64"],
              torch.float32)]
    for name, got, r32, r64, odt in rows_:
        ek, er, allowed = bar(dt, got, r32, r64, odt)
        print(f"\nbwd {dt} Dh {Dh} H {H} rows {rows} pad {pad} {name}: kernel {ek:.3e} yardstick "
              f"{er:.3e} allowed {allowed:.3e}")
        if not ek <= allowed:
            bad.append((name, ek, er))
    assert not bad, bad


# ------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("dt", list(DTYPES))
def test_constant_row_and_single_token(dev, dt):
    """One token whose q head rows are constant (var = 0): finite zeros forward, finite gradients
    backward; the k rows are ordinary."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    H, Dh = 2, 64
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((1, 3 * H * Dh), generator=g) + 8.0).to(DTYPES[dt])
    x[:, :H * Dh] = 3.75
    s = (torch.rand(Dh, generator=g) + 0.5).to(dev)
    buf = x.to(dev)
    pre = K.qk_norm_fwd(buf, H, Dh, s, s, EPS)
    y = buf.float().cpu()
    assert torch.equal(y[:, :H * Dh], torch.zeros(1, H * Dh))
    assert torch.isfinite(y).all() and y[:, H * Dh:2 * H * Dh].abs().max() > 0.1
    dbuf = torch.randn((1, 3 * H * Dh), generator=g).to(DTYPES[dt]).to(dev)
    dq, dk = torch.zeros(Dh, device=dev), torch.zeros(Dh, device=dev)
    K.qk_norm_bwd(dbuf, pre, H, Dh, s, s, dq, dk, EPS)
    assert torch.isfinite(dbuf.float()).all() and torch.isfinite(dq).all() and torch.isfinite(dk).all()
    assert torch.equal(dq.cpu(), torch.zeros(Dh)) and dk.abs().max() > 0      # xhat = 0 on q
    K.device_status()


def test_evaluation_forward_saves_nothing(dev):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    H, Dh = 3, 32
    g = torch.Generator().manual_seed(4)
    x = torch.randn((5, 3 * H * Dh), generator=g).to(torch.bfloat16)
    s = torch.ones(Dh, device=dev)
    a, b = x.to(dev), x.to(dev)
    assert K.qk_norm_fwd(a, H, Dh, s, s, EPS, save=False) is None
    K.qk_norm_fwd(b, H, Dh, s, s, EPS)
    assert torch.equal(a, b)
    K.device_status()


# ----------------------------------------------------------------------------------- guards
def test_guards_raise_before_any_launch(dev):
    """Dh = 48, a row stride below 3 H Dh, a misaligned view, a dtype the kernels do not take and
    scales of the wrong length: MMTError each, no kernel runs (the buffers keep their bits) and the
    device status stays clean."""
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    H, Dh, N = 2, 64, 4
    W = 3 * H * Dh
    g = torch.Generator().manual_seed(5)
    x = torch.randn((N, W + 16), generator=g).to(torch.bfloat16).to(dev)
    keep = x.clone()
    s = torch.ones(Dh, device=dev)
    pre = torch.zeros((N, 2 * H * Dh), dtype=torch.bfloat16, device=dev)
    gq, gk = torch.zeros(Dh, device=dev), torch.zeros(Dh, device=dev)
    s48 = torch.ones(48, device=dev)
    cases = {
        "Dh = 48": lambda f: f(x[:, :3 * H * 48], 48, s48, s48, pre[:, :2 * H * 48].contiguous(),
                               torch.zeros(48, device=dev), torch.zeros(48, device=dev)),
        "ld too small": lambda f: f(x[:, :2 * H * Dh].contiguous(), Dh, s, s, pre, gq, gk),
        "misaligned view": lambda f: f(x[:, 4:4 + W], Dh, s, s, pre, gq, gk),
        "odd row stride": lambda f: f(x[:, :W + 12].contiguous()[:, :W], Dh, s, s, pre, gq, gk),
        "wrong dtype": lambda f: f(x[:, :W].to(torch.float16), Dh, s, s, pre.to(torch.float16), gq, gk),
        "short scales": lambda f: f(x[:, :W], Dh, s[:32].contiguous(), s, pre, gq, gk),
        "long scales": lambda f: f(x[:, :W], Dh, s, torch.ones(2 * Dh, device=dev), pre, gq, gk),
    }

    def fwd(buf, dh, qs, ks, pre_, dq, dk):
        K.qk_norm_fwd(buf, H, dh, qs, ks, EPS)

    def bwd(buf, dh, qs, ks, pre_, dq, dk):
        K.qk_norm_bwd(buf, pre_, H, dh, qs, ks, dq, dk, EPS)
    for what, call in cases.items():
        for f in (fwd, bwd):
            with pytest.raises(_C.MMTError):
                call(f)
            K.device_status()
            assert torch.equal(x, keep), what
            assert not gq.any() and not gk.any(), what
    with pytest.raises(_C.MMTError, match="null"):
        _C.call("mmt_qk_norm_fwd", None, 1, W, N, H, Dh, _C.ptr(s), _C.ptr(s), EPS, None,
                _C.stream_ptr())
    K.device_status()
