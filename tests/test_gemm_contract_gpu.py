"""GPU contract of mmt_gemm / mmt_gemm_xs (include/mmt_api.h): leading dimensions, bounds, batch
strides and argument checks, per kernel family — and which kernel ran.

Every operand is a view into a larger buffer: PAD extra columns per row (8 or 24, so no ld is a
power-of-two multiple) and GUARD rows before and after. The pad and guards of the bf16 / fp32 inputs
hold NaN, so a stored output that depends on anything outside [rows) x [cols) becomes NaN (a
kernel may read past M / N where that feeds only outputs it does not store: the TN kernels do).
The pad and guards of an output hold a sentinel NaN pattern (bf16 0x7FC5 as in
tests/test_glue_gpu.py, fp32 0x7FC00005) that must be bit-identical after the launch: an
out-of-bounds store fails the test. Split-K workspaces are exactly split_k*M*N floats inside a
guarded buffer.

Reference: an fp64 matmul of the same bf16 inputs and the epilogue in fp64. Tolerances are those of
tests/test_gemm_gpu.py: bf16 outputs _close_bf16; fp32 outputs rtol 1e-5, atol 1e-5 max|ref|
(products of bf16 are exact in fp32: accumulation order only); long split-K reductions 1e-4.

Every case asserts mmt_gemm_last_route(): a case whose launch takes another kernel than the one
it is written for fails."""
import pytest
import torch

from oracle import rng as R
from tests.test_gemm_gpu import _close_bf16

pytestmark = pytest.mark.gpu

GUARD = 4                # rows before and after every view
SENT16 = 0x7FC5          # bf16 NaN pattern no kernel here produces
SENT32 = 0x7FC00005      # fp32 NaN pattern likewise
LAYOUTS = [(False, True), (False, False), (True, False), (True, True)]
SEED, STEP = 1234, 7     # dropout stream


def _mods():
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as Kn
    return _C, Kn


class Guarded:
    """`n` matrices (rows, cols) as views into one buffer of n x (GUARD + rows + GUARD) x
    (cols + pad), everything outside the views holding NaN (inputs) or the sentinel (outputs)."""

    def __init__(self, rows, cols, pad, dtype, dev, n=1, values=None):
        self.rows, self.cols, self.ld = rows, cols, cols + pad
        self.itype = torch.int16 if dtype == torch.bfloat16 else torch.int32
        sent = SENT16 if dtype == torch.bfloat16 else SENT32
        self.raw = torch.full((n, rows + 2 * GUARD, self.ld), sent, dtype=self.itype, device=dev)
        self.buf = self.raw.view(dtype)
        self.all = self.buf[:, GUARD:GUARD + rows, :cols]   # (n, rows, cols)
        self.v = self.all[0]
        self.stride = (rows + 2 * GUARD) * self.ld          # elements between entries
        if values is not None:
            self.all.copy_(values.to(dev).to(dtype).view(n, rows, cols))
        self.before = self.raw.clone()

    def ptr(self):
        return self.v.data_ptr()

    def guards_intact(self):
        """Bit-identical outside the views (compared as integers)."""
        now = self.raw.clone()
        now[:, GUARD:GUARD + self.rows, :self.cols] = self.before[:, GUARD:GUARD + self.rows, :self.cols]
        return torch.equal(now, self.before)

    def untouched(self):
        return torch.equal(self.raw, self.before)


def _rand(g, *shape):
    return torch.randn(shape, generator=g)


def _operands(g, dev, M, N, K, ta, tb, n=1, nb=None):
    """A (pad 8) and B (pad 24) as stored for the layout, and their fp64 op() forms (n, M, K) /
    (nb, K, N)."""
    nb = n if nb is None else nb
    a = Guarded(*((K, M) if ta else (M, K)), 8, torch.bfloat16, dev, n, _rand(g, n, *((K, M) if ta else (M, K))))
    b = Guarded(*((N, K) if tb else (K, N)), 24, torch.bfloat16, dev, nb, _rand(g, nb, *((N, K) if tb else (K, N))))
    A = a.all.double().transpose(1, 2) if ta else a.all.double()
    B = b.all.double().transpose(1, 2) if tb else b.all.double()
    return a, b, A, B


def _output(g, dev, M, N, mode, pad=24, n=1, finite=False):
    """C buffer: all sentinel, or (fp32 with beta != 0 / accumulate) a finite interior."""
    _, Kn = _mods()
    dt = torch.bfloat16 if mode == Kn.OUT_BF16 else torch.float32
    return Guarded(M, N, pad, dt, dev, n, _rand(g, n, M, N) if finite else None)


def _epi_ref(acc, M, N, dev, bias=None, relu=False, gate=None, gate_scale=1.0, drop=None,
             residual=None, alpha=1.0, beta=0.0, c0=None):
    """The epilogue of include/mmt_api.h in fp64. drop: (layer, site, row_offset, keep_prob)."""
    v = alpha * acc
    if bias is not None:
        v = v + bias.double()
    if relu:
        v = v.clamp_min(0)
    if gate is not None:
        v = v * (gate.double() > 0).double() * gate_scale
    if drop is not None:
        layer, site, off, kp = drop
        keep = torch.from_numpy(R.dropout_mask_2d(SEED, STEP, layer, site, M, N, off, kp)).to(dev)
        v = torch.where(keep, v / kp, torch.zeros_like(v))
    if residual is not None:
        v = v + residual.double()
    if beta != 0.0:
        v = v + beta * c0.double()
    return v


def _check(out, ref, tol=1e-5):
    assert bool(torch.isfinite(out).all()), "non-finite output: the kernel used pad / guard input"
    if out.dtype == torch.bfloat16:
        _close_bf16(out, ref)
    else:
        torch.testing.assert_close(out.double(), ref, rtol=tol, atol=tol * ref.abs().max().item())


def _rng(dev):
    return torch.tensor([SEED, STEP], dtype=torch.int32, device=dev)


class variant:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        _mods()[0].call("mmt_gemm_set_variant", self.v)

    def __exit__(self, *exc):
        _mods()[0].call("mmt_gemm_set_variant", -1)


def _raw_gemm(M, N, K, a, ta, lda, b, tb, ldb, c, mode, ldc, batch=1, sA=0, sB=0, sC=0, split_k=1,
              e=None, ws=None, ws_elems=0):
    """mmt_gemm with every argument the caller's (pointers as integers): batch strides, a guarded
    workspace and deliberately bad arguments, which _kernels.gemm does not forward."""
    _C, Kn = _mods()
    e = Kn._epi() if e is None else e
    return _C.call("mmt_gemm", M, N, K, a, int(ta), lda, b, int(tb), ldb, c, mode, ldc, batch, sA, sB,
                   sC, split_k, _C.ctypes.byref(e), ws, ws_elems, _C.stream_ptr())


def _route():
    return _mods()[0].last_route()


def _generic_route(v):
    _C, _ = _mods()
    return [_C.ROUTE_GENERIC_P0, _C.ROUTE_GENERIC_P1, _C.ROUTE_GENERIC_P1_BK128, _C.ROUTE_BIG,
            _C.ROUTE_GLDS_NT][v]


def _shape_for(v):
    # variants 0-2: K tail of 8 against BK 64 and 128; variant 3: partial 256 x 192 tiles
    return (264, 200, 200) if v == 3 else (200, 136, 200)


# ------------------------------------------------------------------ 1. generic pipelines, big kernel
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("v", [0, 1, 2, 3])
def test_generic_and_big_padded(dev, v, ta, tb):
    """gemm_kernel PIPE 0 / PIPE 1 / PIPE 1 BK 128 and gemm_big_kernel (variants 0-3), every
    layout, padded lda / ldb / ldc, partial M and N tiles, ragged last K-step: bf16, fp32 and
    fp32 with beta = 1 outputs; guards intact."""
    _C, Kn = _mods()
    M, N, K = _shape_for(v)
    g = torch.Generator().manual_seed(100 + 8 * v + 2 * ta + tb)
    a, b, A, B = _operands(g, dev, M, N, K, ta, tb)
    acc = (A @ B)[0]
    for mode, beta in ((Kn.OUT_BF16, 0.0), (Kn.OUT_F32, 0.0), (Kn.OUT_F32, 1.0)):
        c = _output(g, dev, M, N, mode, finite=beta != 0.0)
        c0 = c.v.clone()
        with variant(v):
            Kn.gemm(a.v, b.v, ta, tb, out=c.v, out_mode=mode, split_k=1, beta=beta)
        assert _route() == _generic_route(v)
        assert c.guards_intact()
        _check(c.v, _epi_ref(acc, M, N, dev, beta=beta, c0=c0))
    assert a.untouched() and b.untouched()


@pytest.mark.parametrize("v", [0, 1, 2, 3])
def test_generic_and_big_epilogue_padded(dev, v):
    """The same kernels' epilogue with padded ld_res / ld_gate: bias + relu + dropout + fp32
    residual, and a gate (one layout per variant)."""
    _C, Kn = _mods()
    M, N, K = _shape_for(v)
    ta, tb = LAYOUTS[v]
    g = torch.Generator().manual_seed(200 + v)
    a, b, A, B = _operands(g, dev, M, N, K, ta, tb)
    acc = (A @ B)[0]
    bias = _rand(g, N).to(dev)
    res = Guarded(M, N, 8, torch.float32, dev, 1, _rand(g, M, N))
    gate = Guarded(M, N, 24, torch.bfloat16, dev, 1, _rand(g, M, N))
    c = _output(g, dev, M, N, Kn.OUT_BF16)
    with variant(v):
        Kn.gemm(a.v, b.v, ta, tb, out=c.v, split_k=1, bias=bias, act=Kn.ACT_RELU, rng=_rng(dev),
                drop_layer=3, drop_site=2, keep_prob=0.9, drop_row_offset=5 * M, residual=res.v)
    assert _route() == _generic_route(v)
    assert c.guards_intact()
    _check(c.v, _epi_ref(acc, M, N, dev, bias=bias, relu=True, drop=(3, 2, 5 * M, 0.9), residual=res.v))
    c = _output(g, dev, M, N, Kn.OUT_F32, pad=8)
    with variant(v):
        Kn.gemm(a.v, b.v, ta, tb, out=c.v, out_mode=Kn.OUT_F32, split_k=1, gate=gate.v,
                gate_scale=1 / 0.9)
    assert _route() == _generic_route(v)
    assert c.guards_intact()
    _check(c.v, _epi_ref(acc, M, N, dev, gate=gate.v, gate_scale=1 / 0.9))


# ------------------------------------------------------------------ 2. split-K slabs + combine
@pytest.mark.parametrize("ta,tb", [(False, True), (True, False)])
@pytest.mark.parametrize("split", [2, 3])
@pytest.mark.parametrize("v", [0, 1, 2, 3])
def test_splitk_slabs_and_combine_padded(dev, v, split, ta, tb):
    """Variants 0-3 writing fp32 slabs (OUT 2) into a workspace of exactly split_k*M*N floats and
    splitk_epilogue_kernel storing through a padded ldc: bf16, fp32 and accumulate (alpha = 0.5)
    outputs. K = 200 gives 128-row chunks, so split_k = 3 is reduced to 2 non-empty splits (the
    third slab is never written and must not be summed). TN slabs under variant 3 are the
    direct-to-LDS TN kernel's (the default gemm_tn_dma16_kernel<256>: M % 384 != 0)."""
    _C, Kn = _mods()
    M, N, K = _shape_for(v)
    g = torch.Generator().manual_seed(300 + 16 * v + 4 * split + 2 * ta + tb)
    a, b, A, B = _operands(g, dev, M, N, K, ta, tb)
    acc = (A @ B)[0]
    main = _C.ROUTE_TN_DMA16_256 if (v == 3 and ta and not tb) else _generic_route(v)
    for mode, alpha in ((Kn.OUT_BF16, 1.0), (Kn.OUT_F32, 1.0), (Kn.OUT_F32_ACCUM, 0.5)):
        accum = mode == Kn.OUT_F32_ACCUM
        c = _output(g, dev, M, N, mode, finite=accum)
        c0 = c.v.clone()
        ws = Guarded(1, split * M * N, 0, torch.float32, dev)
        e = Kn._epi(alpha=alpha)
        with variant(v):
            _raw_gemm(M, N, K, a.ptr(), ta, a.ld, b.ptr(), tb, b.ld, c.ptr(), mode, c.ld,
                      split_k=split, e=e, ws=ws.ptr(), ws_elems=split * M * N)
        assert _route() == main | _C.ROUTE_COMBINE
        assert c.guards_intact() and ws.guards_intact()
        _check(c.v, _epi_ref(acc, M, N, dev, alpha=alpha, beta=1.0 if accum else 0.0, c0=c0))


# ------------------------------------------------------------------ 3. glds-NT
@pytest.mark.parametrize("v", [4, -1])
def test_glds_nt_padded(dev, v):
    """gemm_glds_nt_kernel forced (variant 4) and as the automatic choice (K % 64 != 0 keeps the
    shape off nt256), every operand padded: partial tiles, a K tail of 8 zero-filled in LDS."""
    _C, Kn = _mods()
    M, N, K = 300, 200, 136
    g = torch.Generator().manual_seed(400 + v)
    a, b, A, B = _operands(g, dev, M, N, K, False, True)
    acc = (A @ B)[0]
    bias = _rand(g, N).to(dev)
    res = Guarded(M, N, 8, torch.bfloat16, dev, 1, _rand(g, M, N))
    gate = Guarded(M, N, 24, torch.bfloat16, dev, 1, _rand(g, M, N))
    c = _output(g, dev, M, N, Kn.OUT_BF16)
    with variant(v):
        Kn.gemm(a.v, b.v, False, True, out=c.v, split_k=1, bias=bias, gate=gate.v, gate_scale=2.0,
                residual=res.v)
    assert _route() == _C.ROUTE_GLDS_NT
    assert c.guards_intact()
    _check(c.v, _epi_ref(acc, M, N, dev, bias=bias, gate=gate.v, gate_scale=2.0, residual=res.v))
    c = _output(g, dev, M, N, Kn.OUT_F32, pad=8, finite=True)
    c0 = c.v.clone()
    with variant(v):
        Kn.gemm(a.v, b.v, False, True, out=c.v, out_mode=Kn.OUT_F32, split_k=1, beta=1.0)
    assert _route() == _C.ROUTE_GLDS_NT
    assert c.guards_intact()
    _check(c.v, _epi_ref(acc, M, N, dev, beta=1.0, c0=c0))


# ------------------------------------------------------------------ 4. nt256
@pytest.mark.parametrize("bn,N", [(256, 512), (192, 384), (128, 512), (128, 384)])
def test_nt256_padded(dev, bn, N):
    """gemm_nt256_kernel at each tile width (variants 5 / 6 / 7; N = 512 and 384 where the width
    divides N), M = 300 (a partial second row tile), all operands padded: plain bf16 / fp32, bias +
    relu + dropout + bf16 residual, bias + dropout + fp32 residual (fp32 out), gate."""
    _C, Kn = _mods()
    M, K = 300, 192
    v = {256: 5, 192: 6, 128: 7}[bn]
    want = {256: _C.ROUTE_NT256_256, 192: _C.ROUTE_NT256_192, 128: _C.ROUTE_NT256_128}[bn]
    g = torch.Generator().manual_seed(500 + bn + N)
    a, b, A, B = _operands(g, dev, M, N, K, False, True)
    acc = (A @ B)[0]
    bias = _rand(g, N).to(dev)
    res16 = Guarded(M, N, 8, torch.bfloat16, dev, 1, _rand(g, M, N))
    res32 = Guarded(M, N, 24, torch.float32, dev, 1, _rand(g, M, N))
    gate = Guarded(M, N, 24, torch.bfloat16, dev, 1, _rand(g, M, N))
    drop = dict(rng=_rng(dev), drop_layer=3, drop_site=2, keep_prob=0.9, drop_row_offset=5 * M)
    cases = [
        (Kn.OUT_BF16, {}, {}),
        (Kn.OUT_F32, {}, {}),
        (Kn.OUT_BF16, dict(bias=bias, act=Kn.ACT_RELU, residual=res16.v, **drop),
         dict(bias=bias, relu=True, drop=(3, 2, 5 * M, 0.9), residual=res16.v)),
        (Kn.OUT_F32, dict(bias=bias, residual=res32.v, **drop),
         dict(bias=bias, drop=(3, 2, 5 * M, 0.9), residual=res32.v)),
        (Kn.OUT_BF16, dict(gate=gate.v, gate_scale=1 / 0.9), dict(gate=gate.v, gate_scale=1 / 0.9)),
    ]
    for mode, kw, refkw in cases:
        c = _output(g, dev, M, N, mode)
        with variant(v):
            Kn.gemm(a.v, b.v, False, True, out=c.v, out_mode=mode, split_k=1, **kw)
        assert _route() == want
        assert c.guards_intact()
        _check(c.v, _epi_ref(acc, M, N, dev, **refkw))


# ------------------------------------------------------------------ 5. ntw
def _ntw_plan(M, N, n_cu):
    """ntw_plan of csrc/gemm.hip (default knobs): (bn, rows on 256-row tiles, height of the rest)."""
    bn = 384 if N % 384 == 0 else 192
    tn = N // bn
    ppr = n_cu // tn if n_cu % tn == 0 else 0
    max_rounds = M // (256 * ppr) if ppr else 0
    best, best_cost = (bn, 0, 256), None
    for r in range(max_rounds + 1):
        rows_big = r * ppr * 256
        rem = M - rows_big
        for mt in (64, 128, 192, 256):
            if bn == 192 and mt % 128:
                continue
            tiles = -(-rem // mt) * tn if rem > 0 else 0
            cost = r * (256 + bn) + -(-tiles // n_cu) * (mt + bn)
            if best_cost is None or cost < best_cost:
                best, best_cost = (bn, rows_big, mt), cost
    return best


@pytest.mark.parametrize("M,N,K,ep", [(300, 384, 128, "none"), (70, 768, 64, "res"),
                                      (1000, 1152, 192, "relu")])
def test_ntw_padded(dev, M, N, K, ep):
    """gemm_ntw_kernel (variant 8) with padded A, B, C and residual: ragged row counts on the
    tile height its plan picks (asserted through the route), plain / bf16 residual / relu."""
    _C, Kn = _mods()
    g = torch.Generator().manual_seed(600 + M)
    a, b, A, B = _operands(g, dev, M, N, K, False, True)
    acc = (A @ B)[0]
    res = Guarded(M, N, 8, torch.bfloat16, dev, 1, _rand(g, M, N)) if ep == "res" else None
    c = _output(g, dev, M, N, Kn.OUT_BF16)
    with variant(8):
        Kn.gemm(a.v, b.v, False, True, out=c.v, split_k=1, residual=None if res is None else res.v,
                act=Kn.ACT_RELU if ep == "relu" else Kn.ACT_NONE)
    bn, rows_big, mt2 = _ntw_plan(M, N, torch.cuda.get_device_properties(dev).multi_processor_count)
    assert _route() == _C.route_ntw(bn, mt2 if M > rows_big else 256)
    assert c.guards_intact()
    _check(c.v, _epi_ref(acc, M, N, dev, relu=ep == "relu", residual=None if res is None else res.v))


# ------------------------------------------------------------------ 6. ntws
def test_ntws_padded(dev):
    """gemm_ntws_kernel by automatic dispatch (N = 1152: nine 128-wide tiles, M = 4100: a 4-row
    last panel, one K-step), padded operands: bias + relu, and bias + fp32 residual."""
    _C, Kn = _mods()
    M, N, K = 4100, 1152, 64
    g = torch.Generator().manual_seed(700)
    a, b, A, B = _operands(g, dev, M, N, K, False, True)
    acc = (A @ B)[0]
    bias = _rand(g, N).to(dev)
    res = Guarded(M, N, 8, torch.float32, dev, 1, _rand(g, M, N))
    for kw, refkw in ((dict(bias=bias, act=Kn.ACT_RELU), dict(bias=bias, relu=True)),
                      (dict(bias=bias, act=Kn.ACT_RELU, residual=res.v),
                       dict(bias=bias, relu=True, residual=res.v))):
        c = _output(g, dev, M, N, Kn.OUT_BF16)
        Kn.gemm(a.v, b.v, False, True, out=c.v, split_k=1, **kw)
        assert _route() == _C.ROUTE_NTWS
        assert c.guards_intact()
        _check(c.v, _epi_ref(acc, M, N, dev, **refkw))


# ------------------------------------------------------------------ 7. xs
def test_xs_direct_padded(dev):
    """mmt_gemm_xs with padded ldx / ldw / ldc and a bias: three row panels, the last of 188 rows."""
    _C, Kn = _mods()
    M, N, K = 700, 192, 384
    g = torch.Generator().manual_seed(800)
    a, b, A, B = _operands(g, dev, M, N, K, False, True)
    bias = _rand(g, N).to(dev)
    c = _output(g, dev, M, N, Kn.OUT_BF16)
    _C.call("mmt_gemm_xs", M, N, K, a.ptr(), a.ld, b.ptr(), b.ld, c.ptr(), c.ld, bias.data_ptr(),
            _C.stream_ptr())
    assert _route() == _C.ROUTE_XS
    assert c.guards_intact()
    _check(c.v, _epi_ref((A @ B)[0], M, N, dev, bias=bias))


@pytest.mark.parametrize("padded", [False, True])
def test_xs_through_mmt_gemm(dev, padded):
    """mmt_gemm's own route to gemm_xs_kernel (M >= 32768, K = 384, bias-only bf16 product), with
    contiguous and with padded operands: xs_shape_ok (csrc/gemm_xs.hip) asks 16-B rows and
    ld >= extent only, so the padded launch stays on the kernel."""
    _C, Kn = _mods()
    M, N, K = 32800, 64, 384
    g = torch.Generator().manual_seed(810 + padded)
    bias = _rand(g, N).to(dev)
    if padded:
        a, b, A, B = _operands(g, dev, M, N, K, False, True)
        c = _output(g, dev, M, N, Kn.OUT_BF16)
        av, bv, cv = a.v, b.v, c.v
    else:
        av = _rand(g, M, K).to(torch.bfloat16).to(dev)
        bv = _rand(g, N, K).to(torch.bfloat16).to(dev)
        A, B = av.double()[None], bv.double().t()[None]
        c = Guarded(M + 2 * GUARD, N, 0, torch.bfloat16, dev)  # contiguous: extra rows as guards
        cv = c.v[GUARD:GUARD + M]
    Kn.gemm(av, bv, False, True, out=cv, split_k=1, bias=bias)
    assert _route() == _C.ROUTE_XS
    if padded:
        assert c.guards_intact()
    else:
        flat = c.v.view(torch.int16)
        assert bool((flat[:GUARD] == SENT16).all()) and bool((flat[GUARD + M:] == SENT16).all())
    _check(cv, _epi_ref((A @ B)[0], M, N, dev, bias=bias))


# ------------------------------------------------------------------ 8. TN direct-to-LDS kernels
def _tn_routes(M, k_chunk):
    """Kernel per variant as mmt_gemm's TN block chooses it (-1: the default, MMT_TN_KERNEL unset)."""
    _C, _ = _mods()
    if M % 384 == 0:
        return {10: _C.ROUTE_TN_DMA_384, 13: _C.ROUTE_TN_DMA16_384, 18: _C.ROUTE_TN_R4_384,
                -1: _C.ROUTE_TN_R4_384 if k_chunk <= 2048 else _C.ROUTE_TN_DMA16_384}
    return {10: _C.ROUTE_TN_DMA_256, 13: _C.ROUTE_TN_DMA16_256, 18: _C.ROUTE_TN_DMA16_256,
            -1: _C.ROUTE_TN_DMA16_256}


@pytest.mark.parametrize("M,N,K,split", [
    (264, 200, 2040, 32),     # 256-row tiles, partial M and N, one K-step per split, last of 56 rows
    (520, 392, 2840, 15),     # 256-row tiles, three 64-row K-steps per split, last split of 152 rows
    (384, 200, 2040, 32),     # 384-row tiles, partial N, chunks <= 2048 rows (ring by default / 18)
    (1536, 384, 23232, 11)])  # 384-row tiles, 2112-row chunks (dma16<384> by default / 13)
def test_tn_dma_kernels_partial_tiles(dev, M, N, K, split):
    """gemm_tn_dma_kernel / gemm_tn_dma16_kernel / gemm_tn_r4_kernel (variants 10 / 13 / 18 and
    the default) on partial M / N tiles and ragged K chunks, padded lda / ldb / ldc (columns past
    M / N that they read are NaN pad or the next row: no stored output may depend on them), slabs
    in a guarded workspace, C += A^T B against fp64 at 1e-4. A forced 13 takes dma16 also where
    the default takes the ring; 13 and 18 are bit-identical on 384-row tiles (same per-k32 MFMA
    order, gemm.hip)."""
    _C, Kn = _mods()
    k_chunk = -(-(-(-K // split)) // 64) * 64     # ceil(K / split) rounded up to 64 rows
    assert -(-M // 256) * -(-N // 192) * -(-K // k_chunk) >= 128   # mmt_gemm's big_work floor
    want = _tn_routes(M, k_chunk)
    g = torch.Generator().manual_seed(900 + M + K)
    a, b, A, B = _operands(g, dev, M, N, K, True, False)
    ref = _rand(g, M, N).to(dev)       # the C every variant accumulates into
    c0, ref = ref.clone(), ref.double() + (A @ B)[0]
    outs = {}
    for v in (10, 13, 18, -1):
        c = Guarded(M, N, 24, torch.float32, dev, 1, c0)
        ws = Guarded(1, split * M * N, 0, torch.float32, dev)
        with variant(v):
            _raw_gemm(M, N, K, a.ptr(), True, a.ld, b.ptr(), False, b.ld, c.ptr(), Kn.OUT_F32_ACCUM,
                      c.ld, split_k=split, ws=ws.ptr(), ws_elems=split * M * N)
        assert _route() == want[v] | _C.ROUTE_COMBINE, (v, _route())
        assert c.guards_intact() and ws.guards_intact()
        _check(c.v, ref, tol=1e-4)
        outs[v] = c.v
    if M % 384 == 0:
        assert torch.equal(outs[13], outs[18])


# ------------------------------------------------------------------ 9. batch
def _batch_route(v, ta, tb):
    _C, _ = _mods()
    if v >= 0:
        return _generic_route(v)
    return _C.ROUTE_GLDS_NT if (not ta and tb) else _C.ROUTE_GENERIC_P1  # 4 K-steps: single stage


BATCH_CASES = [(v, ta, tb) for ta, tb in LAYOUTS for v in (-1, 0, 1, 2, 3)] + [(4, False, True)]


@pytest.mark.parametrize("v,ta,tb", BATCH_CASES)
def test_batch_strides(dev, v, ta, tb):
    """batch = 3 with sA / sB / sC larger than one entry (guard rows between the entries of C
    stay intact), bias + relu + alpha, every layout under automatic dispatch and variants 0-3
    (4 for NT)."""
    _C, Kn = _mods()
    M, N, K, nb = 136, 72, 200, 3
    g = torch.Generator().manual_seed(1000 + 8 * (v + 1) + 2 * ta + tb)
    a, b, A, B = _operands(g, dev, M, N, K, ta, tb, n=nb)
    bias = _rand(g, N).to(dev)
    c = _output(g, dev, M, N, Kn.OUT_BF16, n=nb)
    e = Kn._epi(bias=bias, act=Kn.ACT_RELU, alpha=0.75)
    with variant(v):
        _raw_gemm(M, N, K, a.ptr(), ta, a.ld, b.ptr(), tb, b.ld, c.ptr(), Kn.OUT_BF16, c.ld, batch=nb,
                  sA=a.stride, sB=b.stride, sC=c.stride, e=e)
    assert _route() == _batch_route(v, ta, tb)
    assert c.guards_intact()
    acc = A @ B
    for z in range(nb):
        _check(c.all[z], _epi_ref(acc[z], M, N, dev, bias=bias, relu=True, alpha=0.75))


@pytest.mark.parametrize("v,ta,tb", [(-1, False, True), (1, True, False), (3, False, False)])
def test_batch_shared_weight_beta_and_residual(dev, v, ta, tb):
    """batch = 3 with sB = 0 (one weight for all entries); fp32 output with beta = 1; a bf16
    residual, and gate + dropout + residual: all three are indexed by the row within an entry and
    so shared by all entries (include/mmt_api.h)."""
    _C, Kn = _mods()
    M, N, K, nb = 136, 72, 200, 3
    g = torch.Generator().manual_seed(1100 + v)
    a, b, A, B = _operands(g, dev, M, N, K, ta, tb, n=nb, nb=1)
    acc = A @ B                      # (3, M, K) @ (1, K, N)
    want = _batch_route(v, ta, tb)
    c = _output(g, dev, M, N, Kn.OUT_BF16, n=nb)
    with variant(v):
        _raw_gemm(M, N, K, a.ptr(), ta, a.ld, b.ptr(), tb, b.ld, c.ptr(), Kn.OUT_BF16, c.ld, batch=nb,
                  sA=a.stride, sB=0, sC=c.stride)
    assert _route() == want and c.guards_intact()
    for z in range(nb):
        _check(c.all[z], acc[z])
    c = _output(g, dev, M, N, Kn.OUT_F32, n=nb, finite=True, pad=8)
    c0 = c.all.clone()
    with variant(v):
        _raw_gemm(M, N, K, a.ptr(), ta, a.ld, b.ptr(), tb, b.ld, c.ptr(), Kn.OUT_F32, c.ld, batch=nb,
                  sA=a.stride, sB=0, sC=c.stride, e=Kn._epi(beta=1.0))
    assert _route() == want and c.guards_intact()
    for z in range(nb):
        _check(c.all[z], _epi_ref(acc[z], M, N, dev, beta=1.0, c0=c0[z]))
    res = Guarded(M, N, 8, torch.bfloat16, dev, 1, _rand(g, M, N))
    c = _output(g, dev, M, N, Kn.OUT_BF16, n=nb)
    with variant(v):
        _raw_gemm(M, N, K, a.ptr(), ta, a.ld, b.ptr(), tb, b.ld, c.ptr(), Kn.OUT_BF16, c.ld, batch=nb,
                  sA=a.stride, sB=0, sC=c.stride, e=Kn._epi(residual=res.v))
    assert _route() == want and c.guards_intact()
    for z in range(nb):
        _check(c.all[z], _epi_ref(acc[z], M, N, dev, residual=res.v))
    gate = Guarded(M, N, 24, torch.bfloat16, dev, 1, _rand(g, M, N))
    rng = _rng(dev)
    c = _output(g, dev, M, N, Kn.OUT_BF16, n=nb)
    e = Kn._epi(gate=gate.v, gate_scale=1.5, rng=rng, drop_layer=2, drop_site=1, keep_prob=0.8,
                drop_row_offset=3 * M, residual=res.v)
    with variant(v):
        _raw_gemm(M, N, K, a.ptr(), ta, a.ld, b.ptr(), tb, b.ld, c.ptr(), Kn.OUT_BF16, c.ld, batch=nb,
                  sA=a.stride, sB=0, sC=c.stride, e=e)
    assert _route() == want and c.guards_intact()
    for z in range(nb):   # the same gate rows and the same dropout keeps in every entry
        _check(c.all[z], _epi_ref(acc[z], M, N, dev, gate=gate.v, gate_scale=1.5,
                                  drop=(2, 1, 3 * M, 0.8), residual=res.v))


def test_batch_with_splitk_is_rejected(dev):
    _C, Kn = _mods()
    M, N, K, nb = 136, 72, 200, 3
    g = torch.Generator().manual_seed(1200)
    a, b, _, _ = _operands(g, dev, M, N, K, False, True, n=nb)
    c = _output(g, dev, M, N, Kn.OUT_BF16, n=nb)
    ws = Guarded(1, 2 * nb * M * N, 0, torch.float32, dev)
    _raw_gemm(M, N, K, a.ptr(), False, a.ld, b.ptr(), True, b.ld, c.ptr(), Kn.OUT_BF16, c.ld, batch=nb,
              sA=a.stride, sB=b.stride, sC=c.stride)       # a valid launch: the route is non-zero
    assert _route() == _C.ROUTE_GLDS_NT
    c = _output(g, dev, M, N, Kn.OUT_BF16, n=nb)
    with pytest.raises(_C.MMTError):
        _raw_gemm(M, N, K, a.ptr(), False, a.ld, b.ptr(), True, b.ld, c.ptr(), Kn.OUT_BF16, c.ld,
                  batch=nb, sA=a.stride, sB=b.stride, sC=c.stride, split_k=2, ws=ws.ptr(),
                  ws_elems=2 * nb * M * N)
    torch.cuda.synchronize()
    assert _route() == _C.ROUTE_NONE
    assert c.untouched() and ws.untouched()


# ------------------------------------------------------------------ 10. rejections
@pytest.mark.parametrize("what", ["lda", "ldc", "c_align", "ws_short", "ld_res"])
def test_rejected_calls_launch_nothing(dev, what):
    """Calls that break the contract raise MMTError (MMT_ERR_INVALID), report route 0 and leave
    the output buffer all sentinel: lda < K, ldc % 8 != 0, C offset by 2 elements (not 16-B
    aligned), a workspace one float short, ld_res % 8 != 0."""
    _C, Kn = _mods()
    M, N, K = 200, 136, 200
    g = torch.Generator().manual_seed(1300)
    a, b, _, _ = _operands(g, dev, M, N, K, False, True)
    res = Guarded(M, N, 8, torch.bfloat16, dev, 1, _rand(g, M, N))
    ws = Guarded(1, 2 * M * N, 0, torch.float32, dev)
    c = _output(g, dev, M, N, Kn.OUT_BF16)
    args = dict(a=a.ptr(), ta=False, lda=a.ld, b=b.ptr(), tb=True, ldb=b.ld, c=c.ptr(),
                mode=Kn.OUT_BF16, ldc=c.ld)
    _raw_gemm(M, N, K, **args)                    # the valid call first: a non-zero route
    assert _route() == _C.ROUTE_GLDS_NT and c.guards_intact()
    c = _output(g, dev, M, N, Kn.OUT_BF16)
    args["c"] = c.ptr()
    if what == "lda":
        args["lda"] = K - 8
    elif what == "ldc":
        args["ldc"] = N + 4
    elif what == "c_align":
        args["c"] = c.ptr() + 2 * 2
    elif what == "ws_short":
        args.update(split_k=2, ws=ws.ptr(), ws_elems=2 * M * N - 1)
    else:
        e = Kn._epi(residual=res.v)
        e.ld_res = N + 4
        args["e"] = e
    with pytest.raises(_C.MMTError):
        _raw_gemm(M, N, K, **args)
    torch.cuda.synchronize()
    assert _route() == _C.ROUTE_NONE
    assert c.untouched() and ws.untouched()
