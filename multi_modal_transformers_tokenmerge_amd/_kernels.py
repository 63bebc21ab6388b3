"""Torch-facing wrappers of the C ABI (device tensors in, device tensors out).

Each wrapper validates shapes/dtypes/devices on the host BEFORE launching (a bad shape must never
reach a kernel) and calls exactly one libmmt_hip entry point on the current HIP stream. Nothing
here computes on the CPU: a missing library raises (see _C.py).
"""
from __future__ import annotations

import os

import torch

from . import _C
from ._C import ptr

DT = {torch.float32: 0, torch.bfloat16: 1}


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype not in DT:
        raise TypeError(f"unsupported dtype {t.dtype}; expected float32 or bfloat16")
    return DT[t.dtype]


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("libmmt_hip ops take device (cuda/HIP) tensors only")


def device_status() -> None:
    """Synchronise the current stream and raise MMTError if a kernel's device-side index check
    fired since the last call (mmt_device_status, include/mmt_api.h: ToMe merge maps, pos_map and
    gathered rows are range-checked on the GPU; an invalid index is replaced by 0 and recorded
    instead of faulting the context). Not capturable: call it after a step / graph replay."""
    _C.call("mmt_device_status", _C.stream_ptr())


# ------------------------------------------------------------------------------------ ToMe
FLAG_CLASS, FLAG_DISTILL, FLAG_PLAIN_SUM, FLAG_NO_SCATTER = 1, 2, 4, 8


def set_tome_match_path(use_mfma: bool) -> None:
    _C.call("mmt_tome_set_match_path", int(bool(use_mfma)))


def tome_match(metric: torch.Tensor, r: int, flags: int = 0, return_node_max: bool = False):
    """metric (n, t, c) or (n, t, heads, c) (any strides with unit inner stride) -> (unm, src, dst
    [, node_max]) int32 device tensors. r must already be clamped (> 0)."""
    _dev(metric)
    if metric.dim() == 3:
        n, t, c = metric.shape
        heads, s_h = 1, 0
        s_n, s_t = metric.stride(0), metric.stride(1)
        if metric.stride(2) != 1:
            raise ValueError("metric must have unit stride along c")
    elif metric.dim() == 4:
        n, t, heads, c = metric.shape
        s_n, s_t, s_h = metric.stride(0), metric.stride(1), metric.stride(2)
        if metric.stride(3) != 1:
            raise ValueError("metric must have unit stride along c")
    else:
        raise ValueError("metric must be (n, t, c) or (n, t, heads, c)")
    ta = (t + 1) // 2
    dev = metric.device
    unm = torch.empty((n, ta - r), dtype=torch.int32, device=dev)
    src = torch.empty((n, r), dtype=torch.int32, device=dev)
    dst = torch.empty((n, r), dtype=torch.int32, device=dev)
    nmax = torch.empty((n, ta), dtype=torch.float32, device=dev) if return_node_max else None
    ws = torch.empty(_C.workspace_size(_C.WS_TOME_MATCH, n, t, c), dtype=torch.uint8, device=dev)
    _C.call("mmt_tome_match", ptr(metric), _dtype_code(metric), n, t, heads, c, s_n, s_t, s_h, r,
            flags, ptr(unm), ptr(src), ptr(dst), ptr(nmax), ptr(ws), ws.numel(), _C.stream_ptr())
    return (unm, src, dst, nmax) if return_node_max else (unm, src, dst)


def tome_merge_fwd(x: torch.Tensor, set_start: int, t: int, r: int, unm, src, dst,
                   size_in: torch.Tensor | None = None, flags: int = 0, out: torch.Tensor | None = None,
                   want_pos_map: bool = True):
    """x (n, L, D) sequence; merges rows [set_start, set_start+t). Returns (x_out (n, L-r, D),
    size_out (n, t-r) fp32, pos_map (n, t) int32 or None)."""
    _dev(x, size_in, unm, src, dst)
    n, L, D = x.shape
    if x.stride(2) != 1:
        raise ValueError("x must have unit stride along D")
    if not (0 <= set_start and set_start + t <= L):
        raise ValueError("token set out of range")
    for a, shape in ((unm, (n, (t + 1) // 2 - r)), (src, (n, r)), (dst, (n, r))):
        if tuple(a.shape) != shape or a.dtype != torch.int32 or not a.is_contiguous():
            raise ValueError(f"index tensor must be contiguous int32 {shape}")
    if size_in is not None:
        if tuple(size_in.shape) != (n, t) or size_in.dtype != torch.float32 or not size_in.is_contiguous():
            raise ValueError("size_in must be contiguous fp32 (n, t)")
    if out is None:
        out = torch.empty((n, L - r, D), dtype=x.dtype, device=x.device)
    size_out = torch.empty((n, t - r), dtype=torch.float32, device=x.device)
    pos_map = torch.empty((n, t), dtype=torch.int32, device=x.device) if want_pos_map else None
    _C.call("mmt_tome_merge_wavg_fwd", ptr(x), _dtype_code(x), n, L, D, x.stride(0), x.stride(1),
            set_start, t, r, flags, ptr(size_in), ptr(unm), ptr(src), ptr(dst), ptr(out),
            out.stride(0), out.stride(1), ptr(size_out), ptr(pos_map), _C.stream_ptr())
    return out, size_out, pos_map


def tome_merge_seqnorm_fwd(x: torch.Tensor, set_start: int, t: int, r: int, unm, src, dst,
                           gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                           size_in: torch.Tensor | None = None, flags: int = 0,
                           out: torch.Tensor | None = None, y_out: torch.Tensor | None = None,
                           mean_out: torch.Tensor | None = None,
                           rstd_out: torch.Tensor | None = None):
    """tome_merge_fwd (fp32 x) followed by seqnorm_fwd in one launch: returns (x_out, size_out,
    pos_map, y bf16, mean, rstd), each bit-identical to the two-launch form. out / y_out /
    mean_out / rstd_out: optional destinations of x_out / y (strided views allowed) and the
    statistics."""
    _dev(x, size_in, unm, src, dst, gamma, beta, out, y_out, mean_out, rstd_out)
    n, L, D = x.shape
    if x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("tome_merge_seqnorm_fwd takes an fp32 (n, L, D) sequence, unit stride along D")
    if not (0 <= set_start and set_start + t <= L):  # (L - r <= 512 is the library's check)
        raise ValueError("token set out of range")
    for a, shape in ((unm, (n, (t + 1) // 2 - r)), (src, (n, r)), (dst, (n, r))):
        if tuple(a.shape) != shape or a.dtype != torch.int32 or not a.is_contiguous():
            raise ValueError(f"index tensor must be contiguous int32 {shape}")
    if size_in is not None and (tuple(size_in.shape) != (n, t) or size_in.dtype != torch.float32
                                or not size_in.is_contiguous()):
        raise ValueError("size_in must be contiguous fp32 (n, t)")
    out = _seq_out(out, (n, L - r, D), torch.float32, x.device, "out")
    size_out = torch.empty((n, t - r), dtype=torch.float32, device=x.device)
    pos_map = torch.empty((n, t), dtype=torch.int32, device=x.device)
    y = _seq_out(y_out, (n, L - r, D), torch.bfloat16, x.device, "y_out")
    mean = _stat_out(mean_out, n, D, x.device, "mean_out")
    rstd = _stat_out(rstd_out, n, D, x.device, "rstd_out")
    _C.call("mmt_tome_merge_seqnorm_fwd", ptr(x), n, L, D, x.stride(0), x.stride(1), set_start, t,
            r, flags, ptr(size_in), ptr(unm), ptr(src), ptr(dst), ptr(out), out.stride(0),
            out.stride(1), ptr(size_out), ptr(pos_map), ptr(gamma), ptr(beta), eps, ptr(y),
            y.stride(0), y.stride(1), ptr(mean), ptr(rstd), _C.stream_ptr())
    return out, size_out, pos_map, y, mean, rstd


def tome_merge_bwd(g_out: torch.Tensor, set_start: int, t: int, r: int, pos_map: torch.Tensor,
                   size_in: torch.Tensor | None, size_out: torch.Tensor | None,
                   out: torch.Tensor | None = None):
    _dev(g_out, pos_map, size_in, size_out)
    n, Lr, D = g_out.shape
    L = Lr + r
    if out is None:
        out = torch.empty((n, L, D), dtype=g_out.dtype, device=g_out.device)
    _C.call("mmt_tome_merge_wavg_bwd", ptr(g_out), _dtype_code(g_out), n, L, D, g_out.stride(0),
            g_out.stride(1), set_start, t, r, ptr(size_in), ptr(size_out), ptr(pos_map), ptr(out),
            out.stride(0), out.stride(1), _C.stream_ptr())
    return out


def _check_i32(a: torch.Tensor, shape, what: str):
    if tuple(a.shape) != tuple(shape) or a.dtype != torch.int32 or not a.is_contiguous():
        raise ValueError(f"{what} must be contiguous int32 {tuple(shape)}, got "
                         f"{a.dtype} {tuple(a.shape)}")


def tome_pos_map(unm, src, dst, t: int, r: int, flags: int = 0,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """The (n, t) int32 pos_map tome_merge_fwd writes for the same indices and flags (set token ->
    merged row of the set), without a merge."""
    _dev(unm, src, dst, out)
    n = src.shape[0]
    for a, shape, what in ((unm, (n, (t + 1) // 2 - r), "unm"), (src, (n, r), "src"),
                           (dst, (n, r), "dst")):
        _check_i32(a, shape, what)
    if out is None:
        out = torch.empty((n, t), dtype=torch.int32, device=src.device)
    _check_i32(out, (n, t), "pos_map")
    _C.call("mmt_tome_pos_map", ptr(unm), ptr(src), ptr(dst), n, t, r, flags, ptr(out),
            _C.stream_ptr())
    return out


def tome_source_step(pos_map: torch.Tensor, r: int, source: torch.Tensor,
                     first: bool = False) -> torch.Tensor:
    """One merge layer of ToMe's merge_source, in place: source[b, p] = pos_map[b, source[b, p]]
    (first: source[b, p] = pos_map[b, p], the identity start). pos_map (n, t) -> [0, t - r),
    source (n, t0) int32. Returns source."""
    _dev(pos_map, source)
    if pos_map.dim() != 2 or source.dim() != 2:
        raise ValueError("pos_map must be (n, t) and source (n, t0)")
    n, t = pos_map.shape
    t0 = source.shape[1]
    _check_i32(pos_map, (n, t), "pos_map")
    _check_i32(source, (n, t0), "source")
    if first and t0 != t:
        raise ValueError(f"the identity start needs t0 == t, got t0={t0}, t={t}")
    _C.call("mmt_tome_source_step", ptr(pos_map), n, t, r, ptr(source), t0, int(bool(first)),
            _C.stream_ptr())
    return source


def tome_source_groups(source: torch.Tensor, tf: int):
    """The inverse of source (n, t0) -> [0, tf) in CSR form: (group_start (n, tf + 1), members
    (n, t0)) int32, each group's patches in ascending order."""
    _dev(source)
    if source.dim() != 2:
        raise ValueError("source must be (n, t0)")
    n, t0 = source.shape
    _check_i32(source, (n, t0), "source")
    group_start = torch.empty((n, tf + 1), dtype=torch.int32, device=source.device)
    members = torch.empty((n, t0), dtype=torch.int32, device=source.device)
    _C.call("mmt_tome_source_groups", ptr(source), n, t0, tf, ptr(group_start), ptr(members),
            _C.stream_ptr())
    return group_start, members


def _check_seq16(x: torch.Tensor, what: str):
    if x.dim() != 3 or x.stride(2) != 1:
        raise ValueError(f"{what} must be (n, L, D) with unit stride along D")
    _dtype_code(x)
    if x.shape[2] % 8:
        raise ValueError(f"{what}: D={x.shape[2]} must be a multiple of 8")
    if (x.stride(0) * x.element_size()) % 16 or (x.stride(1) * x.element_size()) % 16 \
            or x.data_ptr() % 16:
        raise ValueError(f"{what}: strides and base must be multiples of 16 bytes")


def tome_unmerge_fwd(x: torch.Tensor, set_start: int, tf: int, source: torch.Tensor,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """x (n, L, D) with a merged set of tf rows at set_start -> (n, L - tf + t0, D): the set's rows
    expanded to out[b, set_start + p] = x[b, set_start + source[b, p]], the others copied."""
    _dev(x, source, out)
    _check_seq16(x, "x")
    n, L, D = x.shape
    if source.dim() != 2:
        raise ValueError("source must be (n, t0)")
    t0 = source.shape[1]
    _check_i32(source, (n, t0), "source")
    if not (0 <= set_start and 0 < tf <= t0 and set_start + tf <= L):
        raise ValueError("token set out of range")
    if out is None:
        out = torch.empty((n, L - tf + t0, D), dtype=x.dtype, device=x.device)
    _check_seq16(out, "out")
    if tuple(out.shape) != (n, L - tf + t0, D) or out.dtype != x.dtype:
        raise ValueError(f"out must be {x.dtype} {(n, L - tf + t0, D)}")
    _C.call("mmt_tome_unmerge_fwd", ptr(x), _dtype_code(x), n, L, D, x.stride(0), x.stride(1),
            set_start, tf, ptr(source), t0, ptr(out), out.stride(0), out.stride(1), _C.stream_ptr())
    return out


def tome_unmerge_bwd(g: torch.Tensor, set_start: int, tf: int, group_start: torch.Tensor,
                     members: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The adjoint of tome_unmerge_fwd: g (n, L - tf + t0, D) -> (n, L, D); set row j = the fp32
    sum of its group's rows of g in ascending patch order (tome_source_groups), no atomics."""
    _dev(g, group_start, members, out)
    _check_seq16(g, "g")
    n, Lg, D = g.shape
    if members.dim() != 2:
        raise ValueError("members must be (n, t0)")
    t0 = members.shape[1]
    _check_i32(members, (n, t0), "members")
    _check_i32(group_start, (n, tf + 1), "group_start")
    L = Lg - t0 + tf
    if not (0 <= set_start and 0 < tf <= t0 and set_start + tf <= L):
        raise ValueError("token set out of range")
    if out is None:
        out = torch.empty((n, L, D), dtype=g.dtype, device=g.device)
    _check_seq16(out, "out")
    if tuple(out.shape) != (n, L, D) or out.dtype != g.dtype:
        raise ValueError(f"out must be {g.dtype} {(n, L, D)}")
    _C.call("mmt_tome_unmerge_bwd", ptr(g), _dtype_code(g), n, L, D, g.stride(0), g.stride(1),
            set_start, tf, ptr(group_start), ptr(members), t0, ptr(out), out.stride(0),
            out.stride(1), _C.stream_ptr())
    return out


# ------------------------------------------------------------------------------------ GEMM
OUT_BF16, OUT_F32, OUT_F32_ACCUM = 0, 1, 2
ACT_NONE, ACT_RELU = 0, 1


def _epi(bias=None, act=ACT_NONE, rng=None, drop_layer=0, drop_site=0, keep_prob=1.0,
         drop_row_offset=0, gate=None, gate_scale=1.0, residual=None, alpha=1.0, beta=0.0,
         colsum=None, relu_bits=None, gate_bits=None, keep_bits=None):
    e = _C.Epilogue()
    e.colsum = ptr(colsum)
    e.relu_bits = ptr(relu_bits)
    e.gate_bits = ptr(gate_bits)
    e.keep_bits = ptr(keep_bits)
    e.bias = ptr(bias)
    e.act = act
    e.rng = ptr(rng)
    e.drop_layer, e.drop_site = drop_layer, drop_site
    e.keep_prob = keep_prob
    e.drop_row_offset = drop_row_offset
    e.gate = ptr(gate)
    e.ld_gate = gate.stride(0) if gate is not None else 0
    e.gate_scale = gate_scale
    e.residual = ptr(residual)
    e.ld_res = residual.stride(0) if residual is not None else 0
    e.res_dtype = _dtype_code(residual) if residual is not None else 1
    e.alpha, e.beta = alpha, beta
    return e


def auto_split_k(M: int, N: int, K: int) -> int:
    """Split of the reduction for launches with too few 128x128 tiles to fill 256 CUs (e.g. the
    T5 projections at M = B*32): fp32 slabs + a combine kernel that applies the epilogue."""
    tiles = -(-M // 128) * -(-N // 128)
    if tiles >= 192 or K < 512:
        return 1
    return int(max(1, min(-(-384 // tiles), K // 256, 8)))


def gemm(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False,
         out: torch.Tensor | None = None, out_mode: int = OUT_BF16, split_k: int | None = None,
         **epi):
    """2-D GEMM: op(a) (M x K) . op(b) (K x N). a/b bf16 with unit inner stride.
    trans_a: a is stored (K, M); trans_b: b is stored (N, K) (a weight W[N][K]).
    split_k None: auto_split_k."""
    _dev(a, b, out)
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise TypeError("gemm operands must be bfloat16")
    if a.stride(-1) != 1 or b.stride(-1) != 1:
        raise ValueError("gemm operands need unit inner stride")
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N, Kb = (b.shape[0], b.shape[1]) if trans_b else (b.shape[1], b.shape[0])
    if K != Kb:
        raise ValueError(f"gemm inner dims differ: {K} vs {Kb}")
    odt = torch.bfloat16 if out_mode == OUT_BF16 else torch.float32
    if out is None:
        out = (torch.zeros if out_mode == OUT_F32_ACCUM else torch.empty)(
            (M, N), dtype=odt, device=a.device)
    if out.dtype != odt or tuple(out.shape) != (M, N) or out.stride(-1) != 1:
        raise ValueError("bad gemm output tensor")
    for name, dts in (("gate", (torch.bfloat16,)), ("residual", (torch.bfloat16, torch.float32))):
        t = epi.get(name)
        if t is not None and (tuple(t.shape) != (M, N) or t.dtype not in dts or t.stride(-1) != 1):
            raise ValueError(f"gemm {name} must be {dts} (M, N) with unit inner stride")
    bias = epi.get("bias")
    if bias is not None and (bias.numel() != N or bias.dtype != torch.float32):
        raise ValueError("gemm bias must be fp32 [N]")
    if epi.get("keep_bits") is not None and (epi.get("relu_bits") is None or epi.get("rng") is not None):
        raise ValueError("gemm keep_bits replaces rng's dropout draws in a relu_bits launch")
    for name in ("relu_bits", "gate_bits", "keep_bits"):
        t = epi.get(name)
        if t is not None:
            if not gemm_bits_supported(M, N, K, trans_a, trans_b, out_mode, split_k):
                raise ValueError(f"gemm {name}: this launch shape has no 1-bit gate path")
            rows = -(-M // 256) * 256
            if t.dtype != torch.int32 or tuple(t.shape) != (rows, N // 32) or not t.is_contiguous():
                raise ValueError(f"gemm {name} must be contiguous int32 ({rows}, {N // 32})")
            split_k = 1
    cs = epi.get("colsum")
    if cs is not None:
        rows = gemm_colsum_rows(M, N, K, trans_a, trans_b, out_mode, 1 if split_k is None else split_k)
        if not rows or cs.dtype != torch.float32 or tuple(cs.shape) != (rows, N) or not cs.is_contiguous():
            raise ValueError(f"gemm colsum must be fp32 ({rows}, {N}) and this launch must support it")
        split_k = 1
    e = _epi(**epi)
    if split_k is None:
        split_k = auto_split_k(M, N, K)
    ws = None
    if split_k > 1:  # fp32 partial slabs, summed into `out` by the library's reduce kernel
        ws = torch.empty(split_k * M * N, dtype=torch.float32, device=a.device)
    _C.call("mmt_gemm", M, N, K, ptr(a), int(trans_a), a.stride(0), ptr(b), int(trans_b),
            b.stride(0), ptr(out), out_mode, out.stride(0), 1, 0, 0, 0, split_k,
            _C.ctypes.byref(e), ptr(ws), 0 if ws is None else ws.numel(), _C.stream_ptr())
    return out


def gemm_bits_supported(M: int, N: int, K: int, trans_a: bool = False, trans_b: bool = True,
                        out_mode: int = OUT_BF16, split_k: int | None = 1) -> bool:
    """Whether gemm(..., relu_bits= / gate_bits=) works for this launch (the 256-wide bf16 NT
    path, the same launches that can write epilogue column sums)."""
    return gemm_colsum_rows(M, N, K, trans_a, trans_b, out_mode, 1 if split_k is None else split_k) > 0


def gemm_dropout_keep_bits(rng: torch.Tensor, layer: int, site: int, M: int, N: int,
                           keep_prob: float, row_offset: int = 0, out: torch.Tensor | None = None):
    """The counter-RNG dropout keeps of an (M, N) gemm output in the relu_bits layout: pass as
    gemm(..., relu_bits=, keep_bits=, keep_prob=) without rng for outputs bit-identical to
    gemm(..., rng=, drop_layer=layer, drop_site=site, drop_row_offset=row_offset) — the draws run
    as their own kernel (e.g. on a side stream) instead of in the GEMM epilogue."""
    _dev(rng, out)
    rows = -(-M // 256) * 256
    if out is None:
        out = torch.empty((rows, N // 32), dtype=torch.int32, device=rng.device)
    if N % 256 or out.dtype != torch.int32 or tuple(out.shape) != (rows, N // 32) or not out.is_contiguous():
        raise ValueError(f"gemm_dropout_keep_bits: N % 256 == 0, out contiguous int32 ({rows}, {N // 32})")
    _C.call("mmt_gemm_dropout_keep_bits", ptr(rng), layer, site, M, N, keep_prob, row_offset, ptr(out),
            _C.stream_ptr())
    return out


def gemm_colsum_rows(M: int, N: int, K: int, trans_a: bool = False, trans_b: bool = True,
                     out_mode: int = OUT_BF16, split_k: int = 1) -> int:
    """Rows of the (rows, N) fp32 slab a gemm(..., colsum=slab) fills with the column sums of
    each 256-row panel of its bf16 output; 0 when that launch cannot (use colsum instead)."""
    return _C.call("mmt_gemm_colsum_rows", M, N, K, int(trans_a), int(trans_b), out_mode, split_k)


def quant_rows_fp8(x2d: torch.Tensor, out=None, scale=None):
    """bf16 (R, K) rows -> (e4m3 uint8 (R, K), fp32 scale (R,)): scale = amax / 448 per row."""
    _dev(x2d)
    if x2d.dtype != torch.bfloat16 or x2d.dim() != 2 or x2d.stride(1) != 1:
        raise ValueError("quant_rows_fp8 takes bf16 (rows, K) with unit inner stride")
    R, Kd = x2d.shape
    out = torch.empty((R, Kd), dtype=torch.uint8, device=x2d.device) if out is None else out
    scale = torch.empty(R, dtype=torch.float32, device=x2d.device) if scale is None else scale
    _C.call("mmt_quant_rows_fp8", ptr(x2d), x2d.stride(0), R, Kd, ptr(out), out.stride(0),
            ptr(scale), _C.stream_ptr())
    return out, scale


def gemm_fp8(aq: torch.Tensor, sa: torch.Tensor, bq: torch.Tensor, sb: torch.Tensor,
             out: torch.Tensor | None = None, out_mode: int = OUT_BF16, **epi):
    """(aq (M, K) e4m3 . bq (N, K)^T e4m3) * sa[m] * sb[n] with the GEMM epilogue."""
    _dev(aq, sa, bq, sb, out)
    if aq.dtype != torch.uint8 or bq.dtype != torch.uint8:
        raise TypeError("gemm_fp8 operands are e4m3 bytes (uint8)")
    M, Kd = aq.shape
    N, Kb = bq.shape
    if Kd != Kb or sa.numel() != M or sb.numel() != N:
        raise ValueError("gemm_fp8 shapes")
    if out_mode not in (OUT_BF16, OUT_F32):
        raise ValueError("gemm_fp8 writes bf16 or fp32")
    odt = torch.bfloat16 if out_mode == OUT_BF16 else torch.float32
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=aq.device)
    for name, dts in (("gate", (torch.bfloat16,)), ("residual", (torch.bfloat16, torch.float32))):
        t = epi.get(name)
        if t is not None and (tuple(t.shape) != (M, N) or t.dtype not in dts or t.stride(-1) != 1):
            raise ValueError(f"gemm_fp8 {name} must be {dts} (M, N) with unit inner stride")
    e = _epi(**epi)
    _C.call("mmt_gemm_fp8", M, N, Kd, ptr(aq), aq.stride(0), ptr(sa), ptr(bq), bq.stride(0), ptr(sb),
            ptr(out), out_mode, out.stride(0), _C.ctypes.byref(e), _C.stream_ptr())
    return out


# ----------------------------------------------------------------------------- top-k pruning
def topk_gather(x: torch.Tensor, scores: torch.Tensor, tokenset_idx, tokenset_k):
    """x (B, L, D) fp32/bf16, scores (B, L) fp32; tokenset_idx [(start, num)], tokenset_k [k].
    Returns (out (B, sum k, D), idx (B, sum k) int32)."""
    _dev(x, scores)
    B, L, D = x.shape
    if scores.shape != (B, L) or scores.dtype != torch.float32 or scores.stride(1) != 1:
        raise ValueError("scores must be fp32 (B, L) with unit inner stride")
    n = len(tokenset_idx)
    if n != len(tokenset_k):
        raise ValueError("tokenset_idx and tokenset_k differ in length")
    starts = (_C.ctypes.c_int32 * n)(*[int(s) for s, _ in tokenset_idx])
    lens = (_C.ctypes.c_int32 * n)(*[int(m) for _, m in tokenset_idx])
    ks = (_C.ctypes.c_int32 * n)(*[int(k) for k in tokenset_k])
    K = int(sum(int(k) for k in tokenset_k))
    out = torch.empty((B, K, D), dtype=x.dtype, device=x.device)
    idx = torch.empty((B, K), dtype=torch.int32, device=x.device)
    _C.call("mmt_topk_gather", ptr(x), _dtype_code(x), B, L, D, x.stride(0), x.stride(1),
            ptr(scores), scores.stride(0), n, starts, lens, ks, ptr(out), out.stride(0),
            out.stride(1), ptr(idx), _C.stream_ptr())
    return out, idx


def prune_importance(wsum: torch.Tensor) -> torch.Tensor:
    """(B, H, L) post-dropout attention row sums -> (B, L) importance (mean over keys, heads)."""
    _dev(wsum)
    B, H, L = wsum.shape
    scores = torch.empty((B, L), dtype=torch.float32, device=wsum.device)
    _C.call("mmt_prune_importance", ptr(wsum), B, H, L, ptr(scores), _C.stream_ptr())
    return scores


def gather_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out[b, i] = x[b, idx[b, i]]: x (B, L, D) fp32/bf16, idx (B, K) int32."""
    _dev(x, idx)
    B, L, D = x.shape
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != B or not idx.is_contiguous():
        raise ValueError("idx must be contiguous int32 (B, K)")
    K = idx.shape[1]
    out = torch.empty((B, K, D), dtype=x.dtype, device=x.device)
    _C.call("mmt_gather_rows", ptr(x), _dtype_code(x), B, L, D, x.stride(0), x.stride(1), ptr(idx),
            K, ptr(out), out.stride(0), out.stride(1), _C.stream_ptr())
    return out


def topk_scatter_bwd(dout: torch.Tensor, idx: torch.Tensor, L: int):
    _dev(dout, idx)
    B, K, D = dout.shape
    dx = torch.empty((B, L, D), dtype=dout.dtype, device=dout.device)
    _C.call("mmt_topk_scatter_bwd", ptr(dout), _dtype_code(dout), B, K, D, dout.stride(0),
            dout.stride(1), ptr(idx), L, ptr(dx), dx.stride(0), dx.stride(1), _C.stream_ptr())
    return dx


# ------------------------------------------------------------------------------- attention
class SetTable:
    """Host-side token-set table of one layer: contiguous sets tiling [0, L) and, per query set,
    the bitmask of key sets it attends to (the blockwise mask of token_sequencer.py:94-183)."""

    CAUSAL = 1 << 31  # MMT_SET_CAUSAL: causal within the set (Text, token_sequencer.py:76-82)

    def __init__(self, starts, lens, vis, causal=None):
        n = len(starts)
        if n > 16:
            raise ValueError("at most 16 token sets")
        self.n = n
        self.starts = (_C.ctypes.c_int32 * max(n, 1))(*starts)
        self.lens = (_C.ctypes.c_int32 * max(n, 1))(*lens)
        causal = causal or [False] * n
        self.vis = (_C.ctypes.c_uint32 * max(n, 1))(*[(v & 0xFFFF) | (self.CAUSAL if c else 0)
                                                     for v, c in zip(vis, causal)])
        self.L = int(sum(lens))

    @staticmethod
    def none(L):
        return SetTable([0], [L], [1])


def dropout_bits(rng: torch.Tensor, layer: int, site: int, rows: int, cols: int, keep_prob: float,
                 out: torch.Tensor | None = None):
    """Keep bitmask words (rows, ceil(cols/32)) int32, bit j of word (r, w) = keep(r, 32w + j).
    For a square (attention) mask the result is (2, W, LP), LP = roundup(L, 64): [0] the query-word
    image (bit j of word (w, pos(k)) = keep(32w + j, k), read by the forward and dQ kernels),
    [1] the key-word image (bit j of word (w, pos(q)) = keep(q, 32w + j), read by dK/dV), with
    pos(8g + 4h + i) = 8g + 2i + h (csrc/attention.hip TileMasks: SGPR lane masks)."""
    words = (cols + 31) // 32
    square = rows == cols
    if out is None:
        shape = (2, words, (rows + 63) // 64 * 64) if square else (rows, words)
        out = torch.empty(shape, dtype=torch.int32, device=rng.device)
    out_t = ptr(out[1]) if square else None
    _C.call("mmt_dropout_bits", ptr(rng), layer, site, rows, cols, keep_prob,
            ptr(out[0] if square else out), out_t, _C.stream_ptr())
    return out


def _qkv_geo(qkv: torch.Tensor, H: int):
    if qkv.dim() != 3 or qkv.stride(2) != 1 or qkv.dtype != torch.bfloat16:
        raise ValueError("qkv must be bf16 (B, L, 3*H*Dh) with unit inner stride")
    B, L, three_d = qkv.shape
    if three_d % (3 * H):
        raise ValueError("qkv last dim must be 3*H*Dh")
    return B, L, three_d // (3 * H)


def _check_attn_bits(bits: torch.Tensor, L: int):
    want = (2, (L + 31) // 32, (L + 63) // 64 * 64)
    if tuple(bits.shape) != want or bits.dtype != torch.int32 or not bits.is_contiguous():
        raise ValueError(f"attention dropout needs the square mask of dropout_bits(.., L, L, ..): "
                         f"contiguous int32 {want}, got {tuple(bits.shape)}")


def attn_fwd_resident(L: int, Dh: int, bias: bool = False) -> bool:
    """Whether mmt_attn_fwd takes the K/V-resident kernel (attn_fwd_res_kernel: Dh 64,
    32 < L <= 320, no additive bias; MMT_ATTN_RES=0 disables it) — csrc/attention.hip."""
    import os
    return os.environ.get("MMT_ATTN_RES", "1") != "0" and Dh == 64 and not bias and 32 < L <= 320


def attn_bwd_resident(L: int, Dh: int) -> bool:
    """Whether mmt_attn_bwd takes the two-phase K/V-resident kernel (attn_bwd_res_kernel: Dh 64,
    32 < L <= 320; MMT_ATTN_RES_BWD=0 disables it) — csrc/attention.hip."""
    import os
    return os.environ.get("MMT_ATTN_RES_BWD", "1") != "0" and Dh == 64 and 32 < L <= 320


def _check_key_bias(key_bias: torch.Tensor, B: int, L: int):
    """key_bias: fp32 (B, >= L) rows with unit inner stride. The row stride rule (a multiple of 4,
    >= attn_lp(L): the kernels load aligned float4s up to the padded length) is the library's check."""
    if (key_bias.dim() != 2 or key_bias.dtype != torch.float32 or key_bias.shape[0] != B
            or key_bias.shape[1] < L or key_bias.stride(1) != 1):
        raise ValueError(f"key_bias must be fp32 (B={B}, >= L={L}) with unit inner stride "
                         "(K.tome_size_bias builds it)")
    # a stride the library accepts makes it read attn_lp(L) floats of every row: the last row's
    # must lie inside the tensor's storage (a narrow view of a wider buffer is fine)
    lp, sb = attn_lp(L), key_bias.stride(0)
    if sb >= lp and key_bias.shape[1] < lp:
        have = key_bias.untyped_storage().nbytes() // 4 - key_bias.storage_offset()
        if (B - 1) * sb + lp > have:
            raise ValueError(f"key_bias rows must be readable up to attn_lp(L) = {lp} floats")


def attn_fwd(qkv: torch.Tensor, H: int, scale: float, table: SetTable | None = None,
             drop_bits: torch.Tensor | None = None, keep_prob: float = 1.0,
             bias: torch.Tensor | None = None, out: torch.Tensor | None = None,
             wsum: torch.Tensor | None = None, key_bias: torch.Tensor | None = None):
    """wsum (optional fp32 (B, H, L)): receives the per-query sum of the post-dropout attention
    weights (the pruning importance, compressed_attention.py:302-306).
    key_bias (optional fp32 (B, attn_lp(L)) rows): an additive logit per (sample, key) shared by
    heads and queries — ToMe proportional attention's log token size (tome_size_bias); entries past
    L are ignored. Not with wsum or bias (include/mmt_api.h mmt_attn_fwd_keybias)."""
    _dev(qkv, drop_bits, bias, out, wsum, key_bias)
    B, L, Dh = _qkv_geo(qkv, H)
    t = table or SetTable.none(L)
    if t.L != L:
        raise ValueError(f"set table covers {t.L} tokens, sequence has {L}")
    if bias is not None and (tuple(bias.shape) != (H, L, L) or bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise ValueError("bias must be contiguous fp32 (H, L, L)")
    if out is None:
        out = torch.empty((B, L, H * Dh), dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    if drop_bits is not None:
        _check_attn_bits(drop_bits, L)
        drop_bits = drop_bits[0]
    if wsum is not None and (tuple(wsum.shape) != (B, H, L) or wsum.dtype != torch.float32
                             or not wsum.is_contiguous()):
        raise ValueError("wsum must be contiguous fp32 (B, H, L)")
    args = (ptr(qkv), qkv.stride(0), qkv.stride(1), B, L, H, Dh, scale, t.n, t.starts, t.lens,
            t.vis, ptr(drop_bits), keep_prob, ptr(bias), ptr(out), out.stride(0), out.stride(1),
            ptr(lse), ptr(wsum))
    if key_bias is None:
        _C.call("mmt_attn_fwd", *args, _C.stream_ptr())
    else:
        _check_key_bias(key_bias, B, L)
        _C.call("mmt_attn_fwd_keybias", *args, ptr(key_bias), key_bias.stride(0), _C.stream_ptr())
    return out, lse


def attn_lp(L: int) -> int:
    """Padded row length of the attention dropout words and backward workspace (roundup(L, 64))."""
    return (L + 63) & ~63


def attn_bwd(qkv, o, dout, lse, H: int, scale: float, table: SetTable | None = None,
             drop_bits=None, keep_prob: float = 1.0, dqkv: torch.Tensor | None = None,
             bias_grad: torch.Tensor | None = None, key_bias: torch.Tensor | None = None):
    """bias_grad (fp32 [3*H*Dh], optional) += column sums of dqkv (the QKV bias gradient).
    key_bias: the forward's (lse includes it; it gets no gradient)."""
    _dev(qkv, o, dout, lse, drop_bits, dqkv, bias_grad, key_bias)
    B, L, Dh = _qkv_geo(qkv, H)
    t = table or SetTable.none(L)
    if dout.stride(-1) != 1 or o.stride(-1) != 1:
        raise ValueError("o/dout need unit inner stride")
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    # workspace: rowsum(dO O) of the tiled kernels / the row constants of the resident one
    delta = torch.empty((B * H * 2 * attn_lp(L),), dtype=torch.float32, device=qkv.device)
    if drop_bits is not None:
        _check_attn_bits(drop_bits, L)
    bits, bits_t = (None, None) if drop_bits is None else (drop_bits[0], drop_bits[1])
    if bias_grad is not None and (bias_grad.dtype != torch.float32 or bias_grad.numel() != 3 * H * Dh
                                  or not bias_grad.is_contiguous()):
        raise ValueError("bias_grad must be contiguous fp32 [3*H*Dh]")
    args = (ptr(qkv), qkv.stride(0), qkv.stride(1), B, L, H, Dh, scale, t.n, t.starts, t.lens,
            t.vis, ptr(bits), ptr(bits_t), keep_prob, ptr(o), o.stride(0), o.stride(1), ptr(dout),
            dout.stride(0), dout.stride(1), ptr(lse), ptr(delta), ptr(dqkv), dqkv.stride(0),
            dqkv.stride(1), ptr(bias_grad))
    if key_bias is None:
        _C.call("mmt_attn_bwd", *args, _C.stream_ptr())
    else:
        _check_key_bias(key_bias, B, L)
        _C.call("mmt_attn_bwd_keybias", *args, ptr(key_bias), key_bias.stride(0), _C.stream_ptr())
    return dqkv


def tome_size_bias(B: int, L: int, sets, out: torch.Tensor | None = None) -> torch.Tensor:
    """Proportional attention's key bias of a ToMe layer: fp32 (B, attn_lp(L)) with
    log(size[b, j]) at set_start + j for each (set_start, t, size) of `sets` (size: fp32 (B, t), the
    token sizes a merge handed on) and 0 for the tokens of every other set and the padding.
    One launch per set, no memset (the first launch also zeroes the rest)."""
    sets = list(sets)
    if not sets:
        raise ValueError("tome_size_bias needs at least one (set_start, t, size)")
    _dev(*[s[2] for s in sets], out)
    if out is None:
        out = torch.empty((B, attn_lp(L)), dtype=torch.float32, device=sets[0][2].device)
    elif (tuple(out.shape) != (B, attn_lp(L)) or out.dtype != torch.float32 or out.stride(1) != 1):
        raise ValueError(f"out must be fp32 (B, attn_lp(L)) = {(B, attn_lp(L))}")
    for i, (start, t, size) in enumerate(sets):
        if tuple(size.shape) != (B, t) or size.dtype != torch.float32 or not size.is_contiguous():
            raise ValueError(f"size must be contiguous fp32 (B, t) = {(B, t)}, got {tuple(size.shape)}")
        _C.call("mmt_tome_size_bias", ptr(size), B, t, start, L, ptr(out), out.stride(0),
                1 if i == 0 else 0, _C.stream_ptr())
    return out


# ----------------------------------------------------------------- observation pad masks
PAD_MASK_LOGIT = _C.PAD_MASK_LOGIT   # MMT_PAD_MASK_LOGIT: the key logit of a masked token


def _pad_sets(sets):
    """(n, starts, lens) of a layer's set table — a SetTable, a LayerSets or any (starts, lens)
    pair — as the host int32 arrays the C ABI takes."""
    if isinstance(sets, SetTable):
        return sets.n, sets.starts, sets.lens
    starts, lens = (sets.starts, sets.lens) if hasattr(sets, "starts") else sets
    n = len(starts)
    if len(lens) != n:
        raise ValueError("set table: starts and lens differ in length")
    return n, (_C.ctypes.c_int32 * max(n, 1))(*starts), (_C.ctypes.c_int32 * max(n, 1))(*lens)


def _pad_mask_args(B: int, words, text_mask, text_set: int):
    """Host checks of the (words, text mask) pair every pad-mask kernel takes; returns T."""
    _dev(words, text_mask)
    if words is None and text_mask is None:
        raise ValueError("pad mask: neither the packed set mask nor a text mask")
    if words is not None and (words.dtype != torch.int32 or tuple(words.shape) != (B,)
                              or not words.is_contiguous()):
        raise ValueError(f"words must be contiguous int32 ({B},) (pad_mask_pack builds it)")
    if text_mask is None:
        return 0
    if (text_mask.dtype != torch.bool or text_mask.dim() != 2 or text_mask.shape[0] != B
            or not text_mask.is_contiguous()):
        raise ValueError(f"text_mask must be a contiguous bool (B={B}, T) tensor")
    if text_set < 0:
        raise ValueError("text_mask needs the index of its token set (text_set)")
    return text_mask.shape[1]


def pad_mask_pack(set_mask: torch.Tensor, readout_bits: int = 0,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """set_mask bool (B, n_sets), True = the set is present -> int32 (B,) words of present-bits
    (mmt_pad_mask_pack). readout_bits: the bit mask of the Readout sets; one flagged absent is
    reported by device_status() (MMT_FAULT_PAD_MASK) and treated as present."""
    _dev(set_mask, out)
    if set_mask.dim() != 2 or set_mask.dtype != torch.bool or not set_mask.is_contiguous():
        raise ValueError("set_mask must be a contiguous bool (B, n_sets) tensor")
    B, n = set_mask.shape
    if out is None:
        out = torch.empty((B,), dtype=torch.int32, device=set_mask.device)
    elif tuple(out.shape) != (B,) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f"out must be contiguous int32 ({B},)")
    _C.call("mmt_pad_mask_pack", ptr(set_mask), B, n, readout_bits, ptr(out), _C.stream_ptr())
    return out


def pad_mask_pack_counts(set_mask: torch.Tensor | None, n_sets: int, readout_bits: int,
                         counts: torch.Tensor, pc_sets, min_points,
                         out: torch.Tensor | None = None) -> torch.Tensor:
    """pad_mask_pack with thin clouds as absent sets (mmt_pad_mask_pack_counts): bit pc_sets[s]
    of words[b] is cleared where counts[b, s] < min_points[s]. set_mask: bool (B, n_sets) or None
    (every set present); counts: int32 (B, S) on the device, read by the kernel (no host
    synchronisation: a replayed graph follows its contents); pc_sets, min_points: S host
    integers, the token set of each cloud and the points it needs (its token count)."""
    if not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 2 or \
            not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 (B, S) tensor")
    _dev(set_mask, counts, out)
    B, S = counts.shape
    pc_sets, min_points = [int(v) for v in pc_sets], [int(v) for v in min_points]
    if len(pc_sets) != S or len(min_points) != S:
        raise ValueError(f"pc_sets and min_points must name the {S} clouds of counts, got "
                         f"{len(pc_sets)} and {len(min_points)}")
    if not 1 <= n_sets <= _C.PAD_MASK_MAX_SETS or not 1 <= S <= n_sets:
        raise ValueError(f"n_sets must be in 1 .. {_C.PAD_MASK_MAX_SETS} and S in 1 .. n_sets, "
                         f"got {n_sets} and {S}")
    for s, m in zip(pc_sets, min_points):
        if not 0 <= s < n_sets or (readout_bits >> s) & 1 or m < 0:
            raise ValueError(f"a cloud's set must be in [0, {n_sets}) and no Readout set, its "
                             f"min_points >= 0, got set {s}, min_points {m}")
    if set_mask is not None and (set_mask.dim() != 2 or set_mask.dtype != torch.bool
                                 or tuple(set_mask.shape) != (B, n_sets)
                                 or not set_mask.is_contiguous()
                                 or set_mask.device != counts.device):
        raise ValueError(f"set_mask must be a contiguous bool ({B}, {n_sets}) tensor on the "
                         "counts' device")
    if out is None:
        out = torch.empty((B,), dtype=torch.int32, device=counts.device)
    elif tuple(out.shape) != (B,) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f"out must be contiguous int32 ({B},)")
    arr = _C.ctypes.c_int32 * S
    _C.call("mmt_pad_mask_pack_counts", ptr(set_mask), B, n_sets, readout_bits, ptr(counts), S,
            arr(*pc_sets), arr(*min_points), ptr(out), _C.stream_ptr())
    return out


def pad_mask_images(images: torch.Tensor, words: torch.Tensor, image_sets, n_sets: int,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """A copy of the camera images (B, I, H, W, C), uint8 or fp32, contiguous, with the pixels of
    image (b, i) zeroed where set image_sets[i] is absent in words[b] (mmt_pad_mask_images): what
    the image stem reads under a set pad mask, since its GroupNorm runs over all patches of all
    cameras of a sample. `images` itself is not changed."""
    _dev(images, words, out)
    if images.dim() < 3 or not images.is_contiguous():
        raise ValueError("images must be a contiguous (B, I, ...) tensor")
    B, I = images.shape[:2]
    image_sets = list(image_sets)
    if len(image_sets) != I:
        raise ValueError(f"image_sets names {len(image_sets)} sets for {I} images per sample")
    if words.dtype != torch.int32 or tuple(words.shape) != (B,) or not words.is_contiguous():
        raise ValueError(f"words must be contiguous int32 ({B},) (pad_mask_pack builds it)")
    if out is None:
        out = torch.empty_like(images)
    elif out.shape != images.shape or out.dtype != images.dtype or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor of the images' shape and dtype")
    nbytes = images[0, 0].numel() * images.element_size()
    _C.call("mmt_pad_mask_images", ptr(words), (_C.ctypes.c_int32 * max(I, 1))(*image_sets), n_sets,
            B, I, nbytes, ptr(images), ptr(out), _C.stream_ptr())
    return out


def pad_mask_bias(B: int, L: int, sets, words: torch.Tensor | None,
                  text_mask: torch.Tensor | None = None, out: torch.Tensor | None = None,
                  accumulate: bool = False, text_set: int = 0) -> torch.Tensor:
    """The pad masks as the key bias of one layer (mmt_pad_mask_bias): fp32 (B, attn_lp(L)) with
    PAD_MASK_LOGIT on the keys of absent sets (words: pad_mask_pack's, None = all present) and on
    the padded tokens of set text_set (text_mask bool (B, T), True = real), 0 elsewhere and on the
    padding. sets: the layer's set table. accumulate (out given): PAD_MASK_LOGIT is added to the
    masked entries of the rows tome_size_bias wrote and nothing else is touched. out may be a
    (B, attn_lp(L)) view of wider rows."""
    n, starts, lens = _pad_sets(sets)
    T = _pad_mask_args(B, words, text_mask, text_set)
    _dev(out)
    if out is None:
        if accumulate:
            raise ValueError("pad_mask_bias(accumulate=True) needs the rows to add to (out=)")
        dev = (words if words is not None else text_mask).device
        out = torch.empty((B, attn_lp(L)), dtype=torch.float32, device=dev)
    elif (tuple(out.shape) != (B, attn_lp(L)) or out.dtype != torch.float32 or out.stride(1) != 1):
        raise ValueError(f"out must be fp32 (B, attn_lp(L)) = {(B, attn_lp(L))}, unit inner stride")
    _C.call("mmt_pad_mask_bias", ptr(words), B, L, n, starts, lens, ptr(text_mask), text_set, T,
            ptr(out), out.stride(0), int(bool(accumulate)), _C.stream_ptr())
    return out


def _pad_rows(name: str, x: torch.Tensor, sets, words, text_mask, text_set, pe):
    _dev(x, pe)
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("the sequence must be fp32 (B, L, D) with unit stride along D")
    B, L, D = x.shape
    n, starts, lens = _pad_sets(sets)
    T = _pad_mask_args(B, words, text_mask, text_set)
    args = (ptr(words), B, L, D, n, starts, lens, ptr(text_mask), text_set, T)
    if pe is not None:
        if tuple(pe.shape) != (L, D) or pe.dtype != torch.float32 or not pe.is_contiguous():
            raise ValueError(f"pe must be contiguous fp32 (L, D) = {(L, D)}")
        args += (ptr(pe),)
    _C.call(name, *args, ptr(x), x.stride(0), x.stride(1), _C.stream_ptr())
    return x


def pad_mask_rows_fwd(x0: torch.Tensor, pe: torch.Tensor, sets, words,
                      text_mask: torch.Tensor | None = None, text_set: int = 0) -> torch.Tensor:
    """x0[b, l] = pe[l] on the masked rows of the assembled fp32 (B, L, D) sequence, in place
    (mmt_pad_mask_rows_fwd); the other rows are not touched. sets: layer 0's table."""
    return _pad_rows("mmt_pad_mask_rows_fwd", x0, sets, words, text_mask, text_set, pe)


def pad_mask_rows_bwd(dx0: torch.Tensor, sets, words, text_mask: torch.Tensor | None = None,
                      text_set: int = 0) -> torch.Tensor:
    """dx0[b, l] = 0 on the masked rows, in place (mmt_pad_mask_rows_bwd)."""
    return _pad_rows("mmt_pad_mask_rows_bwd", dx0, sets, words, text_mask, text_set, None)


# ------------------------------------------------------------------------ seq LayerNorm etc.
def _seq_out(out, shape, dtype, device, what: str):
    """`out` or a fresh (B, L, D) tensor; a given one may be a strided view (unit stride along D)."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.stride(-1) != 1:
        raise ValueError(f"{what} must be {dtype} {tuple(shape)} with unit stride along D")
    return out


def _stat_out(out, B: int, D: int, device, what: str):
    """`out` or a fresh contiguous fp32 (B, D) tensor (mean / rstd)."""
    if out is None:
        return torch.empty((B, D), dtype=torch.float32, device=device)
    if tuple(out.shape) != (B, D) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"{what} must be contiguous fp32 {(B, D)}")
    return out


def seqnorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                out: torch.Tensor | None = None, mean_out: torch.Tensor | None = None,
                rstd_out: torch.Tensor | None = None):
    """x (B, L, D) bf16 or fp32 (the residual stream) -> y bf16, mean, rstd (B, D) fp32."""
    _dev(x, gamma, beta, out, mean_out, rstd_out)
    B, L, D = x.shape
    if out is None:
        out = torch.empty((B, L, D), dtype=torch.bfloat16, device=x.device)
    mean = _stat_out(mean_out, B, D, x.device, "mean_out")
    rstd = _stat_out(rstd_out, B, D, x.device, "rstd_out")
    _C.call("mmt_seqnorm_fwd", ptr(x), _dtype_code(x), x.stride(0), x.stride(1), B, L, D,
            ptr(gamma), ptr(beta), eps, ptr(out), out.stride(0), out.stride(1), ptr(mean),
            ptr(rstd), _C.stream_ptr())
    return out, mean, rstd


def seqnorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, addend=None, out=None):
    """dx (dtype of x) = LN backward (+ addend, dtype of x); dy bf16 or fp32."""
    _dev(dy, x, mean, rstd, gamma, dgamma, dbeta, addend, out)
    B, L, D = x.shape
    if addend is not None and addend.dtype != x.dtype:
        raise TypeError("addend must have the residual (x) dtype")
    if out is None:
        out = torch.empty((B, L, D), dtype=x.dtype, device=x.device)
    a_sb, a_st = (addend.stride(0), addend.stride(1)) if addend is not None else (0, 0)
    _C.call("mmt_seqnorm_bwd", ptr(dy), _dtype_code(dy), dy.stride(0), dy.stride(1), ptr(x),
            _dtype_code(x), x.stride(0), x.stride(1), B, L, D, ptr(mean), ptr(rstd), ptr(gamma),
            ptr(addend), a_sb, a_st, ptr(out), out.stride(0), out.stride(1), ptr(dgamma),
            ptr(dbeta), _C.stream_ptr())
    return out


def colsum(x2d: torch.Tensor, out: torch.Tensor):
    _dev(x2d, out)
    M, N = x2d.shape
    _C.call("mmt_colsum", ptr(x2d), _dtype_code(x2d), x2d.stride(0), M, N, ptr(out), _C.stream_ptr())
    return out


def seqnorm_dropout_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, addend, rng, layer: int,
                        site: int, keep_prob: float, row_offset: int, colsum=None, out=None,
                        z_out=None):
    """seqnorm_bwd (bf16 dy, fp32 x / addend) returning (dx fp32, z bf16), z = the previous
    block's dropout backward of dx (dropout_bwd semantics, colsum += its column sums).
    out / z_out: optional (strided) destinations of dx / z."""
    _dev(dy, x, mean, rstd, gamma, dgamma, dbeta, addend, rng, colsum, out, z_out)
    B, L, D = x.shape
    if x.dtype != torch.float32 or dy.dtype != torch.bfloat16 or (addend is not None and addend.dtype != torch.float32):
        raise TypeError("seqnorm_dropout_bwd takes bf16 dy and fp32 x / addend")
    dx = _seq_out(out, (B, L, D), torch.float32, x.device, "out")
    z = _seq_out(z_out, (B, L, D), torch.bfloat16, x.device, "z_out")
    a_sb, a_st = (addend.stride(0), addend.stride(1)) if addend is not None else (0, 0)
    _C.call("mmt_seqnorm_dropout_bwd", ptr(dy), dy.stride(0), dy.stride(1), ptr(x), x.stride(0),
            x.stride(1), B, L, D, ptr(mean), ptr(rstd), ptr(gamma), ptr(addend), a_sb, a_st, ptr(dx),
            dx.stride(0), dx.stride(1), ptr(dgamma), ptr(dbeta), ptr(rng), layer, site, keep_prob,
            row_offset, ptr(z), z.stride(0), z.stride(1), ptr(colsum), _C.stream_ptr())
    return dx, z


UNMERGE_MAX_L = 512          # csrc/norm.hip kUnmergeMax: unmerged rows per sample
UNMERGE_MAX_L2 = 96 * 1024 // (64 * 4)   # the merged (L2, 64-column) fp32 panel in <= 96 KB LDS


def ln_unmerge_ok(L: int, L2: int) -> bool:
    """The shapes mmt_ln_unmerge_dropout_bwd accepts (its C-side check, csrc/norm.hip): at most
    512 unmerged rows AND a merged panel of at most 384 rows; otherwise the caller takes the
    three-kernel path (seqnorm_bwd -> tome_merge_bwd -> dropout_bwd)."""
    return L <= UNMERGE_MAX_L and L2 <= UNMERGE_MAX_L2


def ln_unmerge_dropout_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, addend, tome, rng, layer: int,
                           site: int, keep_prob: float, row_offset: int, bias_grad=None, out=None,
                           z_out=None):
    """seqnorm_bwd (merged layout: dy bf16, x / addend fp32) -> tome_merge_bwd -> dropout_bwd in one
    launch: returns (g_in fp32 (B, L, D), z bf16 (B, L, D)); dgamma / dbeta / bias_grad accumulated.
    tome = (set_start, t, r, pos_map, size_in, size_out). out / z_out: optional (strided)
    destinations of g_in / z."""
    _dev(dy, x, mean, rstd, gamma, dgamma, dbeta, addend, rng, bias_grad, out, z_out)
    B, L2, D = x.shape
    s0, t, r, pos, size_in, size_out = tome
    L = L2 + r
    if x.dtype != torch.float32 or dy.dtype != torch.bfloat16 or (addend is not None and addend.dtype != torch.float32):
        raise TypeError("ln_unmerge_dropout_bwd takes bf16 dy and fp32 x / addend")
    g_in = _seq_out(out, (B, L, D), torch.float32, x.device, "out")
    z = _seq_out(z_out, (B, L, D), torch.bfloat16, x.device, "z_out")
    a_sb, a_st = (addend.stride(0), addend.stride(1)) if addend is not None else (0, 0)
    _C.call("mmt_ln_unmerge_dropout_bwd", ptr(dy), dy.stride(0), dy.stride(1), ptr(x), x.stride(0),
            x.stride(1), B, L2, D, ptr(mean), ptr(rstd), ptr(gamma), ptr(addend), a_sb, a_st,
            ptr(dgamma), ptr(dbeta), L, s0, t, r, ptr(size_in), ptr(size_out), ptr(pos), ptr(g_in),
            g_in.stride(0), g_in.stride(1), ptr(rng), layer, site, keep_prob, row_offset, ptr(z),
            z.stride(0), z.stride(1), ptr(bias_grad), _C.stream_ptr())
    return g_in, z


def dropout_bwd(dy2d: torch.Tensor, rng, layer: int, site: int, keep_prob: float,
                row_offset: int = 0, out: torch.Tensor | None = None, colsum_out=None):
    """dz (bf16) = dy * keep / keep_prob; rng None: plain cast. colsum_out += column sums."""
    _dev(dy2d, rng, out, colsum_out)
    M, N = dy2d.shape
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=dy2d.device)
    _C.call("mmt_dropout_bwd", ptr(dy2d), _dtype_code(dy2d), dy2d.stride(0), M, N, ptr(rng), layer,
            site, keep_prob, row_offset, ptr(out), out.stride(0), ptr(colsum_out), _C.stream_ptr())
    return out


# ------------------------------------------------------------------------------- image stem
IMG_F32, IMG_U8 = 0, 2


def patch_im2col(img: torch.Tensor, patch: int, kh: int, kw: int, stride: int, normalize: bool = True,
                 out: torch.Tensor | None = None):
    """img (B, I, H, H, C) fp32 or uint8 -> bf16 [B*I*NP*OH*OW][kh*kw*C]."""
    _dev(img, out)
    if img.dim() != 5 or img.shape[2] != img.shape[3] or not img.is_contiguous():
        raise ValueError("image must be contiguous (B, I, H, H, C) (square, image_tokenizer.py:49-50)")
    B, I, H, _, C = img.shape
    if H % patch:
        raise ValueError(f"image size {H} not divisible by patch {patch}")
    code = {torch.float32: IMG_F32, torch.uint8: IMG_U8}.get(img.dtype)
    if code is None:
        raise TypeError("image dtype must be float32 or uint8")
    oh, ow = (patch - kh) // stride + 1, (patch - kw) // stride + 1
    rows = B * I * (H // patch) ** 2 * oh * ow
    if out is None:
        out = torch.empty((rows, kh * kw * C), dtype=torch.bfloat16, device=img.device)
    _C.call("mmt_patch_im2col", ptr(img), code, B, I, H, C, patch, kh, kw, stride, int(normalize),
            ptr(out), _C.stream_ptr())
    return out


def _f32(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(f"{what} must be contiguous fp32")


def maxpool_patch(conv: torch.Tensor, win: int):
    """conv fp32 (npatch*win, C) -> pooled fp32 (npatch, C), first-max argmax uint8."""
    _f32(conv, "conv output")
    rows, C = conv.shape
    npatch = rows // win
    pooled = torch.empty((npatch, C), dtype=torch.float32, device=conv.device)
    arg = torch.empty((npatch, C), dtype=torch.uint8, device=conv.device)
    _C.call("mmt_maxpool_patch", ptr(conv), npatch, win, C, ptr(pooled), ptr(arg), _C.stream_ptr())
    return pooled, arg


def maxpool_patch_bwd(dpooled: torch.Tensor, arg: torch.Tensor, win: int, out=None):
    _f32(dpooled, "dpooled")
    npatch, C = dpooled.shape
    if out is None:
        out = torch.empty((npatch * win, C), dtype=torch.bfloat16, device=dpooled.device)
    _C.call("mmt_maxpool_patch_bwd", ptr(dpooled), ptr(arg), npatch, win, C, ptr(out), _C.stream_ptr())
    return out


def maxpool2d(x: torch.Tensor, npatch: int, OH: int, OW: int, KP: int):
    """x fp32 (npatch*OH*OW, C) -> pooled fp32 (npatch*PH*PW, C) (KP x KP, stride 1, VALID) and
    the window slot of the first maximum (uint8)."""
    _f32(x, "conv output")
    C = x.shape[-1]
    if x.numel() != npatch * OH * OW * C:
        raise ValueError("maxpool2d: x is not (npatch*OH*OW, C)")
    rows = npatch * (OH - KP + 1) * (OW - KP + 1)
    y = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    arg = torch.empty((rows, C), dtype=torch.uint8, device=x.device)
    _C.call("mmt_maxpool2d", ptr(x), npatch, OH, OW, C, KP, ptr(y), ptr(arg), _C.stream_ptr())
    return y, arg


def maxpool2d_bwd(dy: torch.Tensor, arg: torch.Tensor, npatch: int, OH: int, OW: int, KP: int):
    """-> bf16 (npatch*OH*OW, C): the gradient routed to each window's first maximum."""
    _f32(dy, "dpooled")
    C = dy.shape[-1]
    G = torch.empty((npatch * OH * OW, C), dtype=torch.bfloat16, device=dy.device)
    _C.call("mmt_maxpool2d_bwd", ptr(dy), ptr(arg), npatch, OH, OW, C, KP, ptr(G), _C.stream_ptr())
    return G


def im2col_same(x: torch.Tensor, npatch: int, H: int, W: int, KS: int):
    """x bf16 (npatch*H*W, C) -> (npatch*H*W, KS*KS*C) bf16 columns of a SAME KS x KS conv."""
    _dev(x)
    C = x.shape[-1]
    if x.dtype != torch.bfloat16 or x.numel() != npatch * H * W * C or not x.is_contiguous():
        raise ValueError("im2col_same: x must be contiguous bf16 (npatch*H*W, C)")
    cols = torch.empty((npatch * H * W, KS * KS * C), dtype=torch.bfloat16, device=x.device)
    _C.call("mmt_im2col_same", ptr(x), npatch, H, W, C, KS, ptr(cols), _C.stream_ptr())
    return cols


def col2im_same(dcols: torch.Tensor, npatch: int, H: int, W: int, C: int, KS: int):
    _f32(dcols, "column gradient")
    dx = torch.empty((npatch * H * W, C), dtype=torch.float32, device=dcols.device)
    _C.call("mmt_col2im_same", ptr(dcols), npatch, H, W, C, KS, ptr(dx), _C.stream_ptr())
    return dx


def groupnorm_gelu_fwd(x: torch.Tensor, groups: int, gamma, beta, eps: float, out=None):
    """x (B, R, C) fp32 contiguous -> gelu(GroupNorm(x)) bf16."""
    _f32(x, "groupnorm input")
    B, R, C = x.shape
    if out is None:
        out = torch.empty((B, R, C), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty((B, groups), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, groups), dtype=torch.float32, device=x.device)
    _C.call("mmt_groupnorm_gelu_fwd", ptr(x), B, R, C, groups, eps, ptr(gamma), ptr(beta), ptr(out),
            ptr(mean), ptr(rstd), _C.stream_ptr())
    return out, mean, rstd


def groupnorm_gelu_bwd(dy, x, groups, gamma, beta, mean, rstd, dgamma, dbeta, dx=None,
                       accumulate=False):
    """dy, x, dx fp32 (B, R, C); accumulate: dx += result."""
    _f32(dy, "dy")
    _f32(x, "x")
    B, R, C = x.shape
    if dx is None:
        dx = torch.empty_like(x)
    _C.call("mmt_groupnorm_gelu_bwd", ptr(dy), ptr(x), B, R, C, groups, ptr(gamma), ptr(beta),
            ptr(mean), ptr(rstd), ptr(dx), int(accumulate), ptr(dgamma), ptr(dbeta), _C.stream_ptr())
    return dx


def stem_conv_pool(images: torch.Tensor, w: torch.Tensor, bias: torch.Tensor):
    """images (B, I, H, H, 3) uint8, w (64, 432) bf16 [out][(ky, kx, c)], bias fp32 (64,) ->
    (pooled (B*I*NP, 64) fp32, argmax (B*I*NP, 64) uint8): 12x12 s2 conv of each normalised
    16x16 patch + bias, max over its 3x3 map (first maximum)."""
    _dev(images, w, bias)
    if images.dtype != torch.uint8 or images.dim() != 5 or images.shape[-1] != 3 or \
            images.shape[2] != images.shape[3] or images.shape[2] % 16 or not images.is_contiguous():
        raise ValueError("stem_conv_pool takes contiguous uint8 (B, I, H, H, 3) images, H % 16 == 0")
    if w.dtype != torch.bfloat16 or tuple(w.shape) != (64, 432) or not w.is_contiguous():
        raise ValueError("stem_conv_pool weight must be contiguous bf16 (64, 432)")
    if bias.dtype != torch.float32 or bias.numel() != 64:
        raise ValueError("stem_conv_pool bias must be fp32 (64,)")
    B, I, H = images.shape[:3]
    n = B * I * (H // 16) ** 2
    pooled = torch.empty((n, 64), dtype=torch.float32, device=images.device)
    arg = torch.empty((n, 64), dtype=torch.uint8, device=images.device)
    _C.call("mmt_stem_conv_pool", ptr(images), B, I, H, ptr(w), ptr(bias), ptr(pooled), ptr(arg),
            _C.stream_ptr())
    return pooled, arg


def stem_conv_wgrad(images: torch.Tensor, dpooled: torch.Tensor, arg: torch.Tensor,
                    wgrad: torch.Tensor):
    """wgrad (64, 432) fp32 += the stem conv weight gradient from the pooled gradient (fp32
    (B*I*NP, 64)) and the forward's argmax, straight from the uint8 images (no im2col)."""
    _dev(images, dpooled, arg, wgrad)
    B, I, H = images.shape[:3]
    n = B * I * (H // 16) ** 2
    if tuple(dpooled.shape) != (n, 64) or dpooled.dtype != torch.float32 or not dpooled.is_contiguous():
        raise ValueError("dpooled must be contiguous fp32 (B*I*NP, 64)")
    if tuple(arg.shape) != (n, 64) or arg.dtype != torch.uint8 or not arg.is_contiguous():
        raise ValueError("argmax must be contiguous uint8 (B*I*NP, 64)")
    if tuple(wgrad.shape) != (64, 432) or wgrad.dtype != torch.float32 or not wgrad.is_contiguous():
        raise ValueError("wgrad must be contiguous fp32 (64, 432)")
    rows = _C.call("mmt_stem_conv_wgrad_slabs", B, I, H)
    slab = torch.empty((rows, 64 * 432), dtype=torch.float32, device=images.device)
    _C.call("mmt_stem_conv_wgrad", ptr(images), B, I, H, ptr(dpooled), ptr(arg), ptr(slab),
            slab.numel(), _C.stream_ptr())
    colsum(slab, wgrad.view(-1))
    return wgrad


def patch_positions(B: int, I: int, H: int, patch: int, Q: int, train: bool, rng=None, site: int = 0,
                    sample_offset: int = 0, device=None):
    npatch = (H // patch) ** 2
    dev = device if device is not None else rng.device
    rt = torch.empty((B, I * npatch), dtype=torch.int32, device=dev)
    ct = torch.empty((B, I * npatch), dtype=torch.int32, device=dev)
    _C.call("mmt_patch_positions", ptr(rng), site, B, I, H, patch, Q, int(train), sample_offset,
            ptr(rt), ptr(ct), _C.stream_ptr())
    return rt, ct


# ---------------------------------------------------------------------------------- glue
def rmsnorm(x2d: torch.Tensor, w: torch.Tensor, eps: float, out=None):
    rows, D = x2d.shape
    if out is None:
        out = torch.empty_like(x2d)
    _C.call("mmt_rmsnorm_fwd", ptr(x2d), rows, D, ptr(w), eps, ptr(out), _C.stream_ptr())
    return out


def embedding_gather(ids: torch.Tensor, table: torch.Tensor, out=None):
    n = ids.numel()
    vocab, D = table.shape
    if out is None:
        out = torch.empty((n, D), dtype=table.dtype, device=table.device)
    _C.call("mmt_embedding_gather", ptr(ids), n, D, ptr(table), vocab, ptr(out), _C.stream_ptr())
    return out


def cast_f32_bf16(a: torch.Tensor, out: torch.Tensor):
    _C.call("mmt_cast_f32_bf16", ptr(a), ptr(out), a.numel(), _C.stream_ptr())
    return out


# ---------------------------------------------------------------------- attention pooling
def _rows2d(t: torch.Tensor, D: int, what: str, dtypes=(torch.bfloat16,)):
    if t.dim() != 2 or t.shape[1] != D or t.dtype not in dtypes or t.stride(1) != 1:
        raise ValueError(f"{what} must be {dtypes} (rows, {D}) with unit inner stride")


def rows_gather_bf16(x: torch.Tensor, rows: torch.Tensor, out: torch.Tensor | None = None):
    """x (B, L, D) fp32 (strided, unit inner stride), rows (n,) int32 -> (B, n, D) bf16."""
    _dev(x, rows, out)
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("x must be fp32 (B, L, D) with unit inner stride")
    B, L, D = x.shape
    n = rows.numel()
    _check_i32(rows, (n,), "rows")
    if out is None:
        out = torch.empty((B, n, D), dtype=torch.bfloat16, device=x.device)
    if tuple(out.shape) != (B, n, D) or out.dtype != torch.bfloat16 or not out.is_contiguous():
        raise ValueError(f"out must be contiguous bf16 {(B, n, D)}")
    _C.call("mmt_rows_gather_bf16", ptr(x), x.stride(0), x.stride(1), B, L, D, ptr(rows), n,
            ptr(out), _C.stream_ptr())
    return out


def rows_scatter_bwd(dr: torch.Tensor, row_flag: torch.Tensor, out: torch.Tensor | None = None):
    """dr (B, n, D) bf16 contiguous, row_flag (L,) int32 (slot index or -1) -> the whole fp32
    (B, L, D) gradient: dr[b, row_flag[l]] in the flagged rows, 0 elsewhere."""
    _dev(dr, row_flag, out)
    if dr.dim() != 3 or dr.dtype != torch.bfloat16 or not dr.is_contiguous():
        raise ValueError("dr must be contiguous bf16 (B, n, D)")
    B, n, D = dr.shape
    L = row_flag.numel()
    _check_i32(row_flag, (L,), "row_flag")
    if out is None:
        out = torch.empty((B, L, D), dtype=torch.float32, device=dr.device)
    if tuple(out.shape) != (B, L, D) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be contiguous fp32 {(B, L, D)}")
    _C.call("mmt_rows_scatter_bwd", ptr(dr), B, L, D, ptr(row_flag), n, ptr(out), _C.stream_ptr())
    return out


def _check_pool_kv(q, k, v, B, n, H, Dh):
    D = H * Dh
    if q.dtype != torch.float32 or q.numel() != D or not q.is_contiguous():
        raise ValueError(f"q must be contiguous fp32 ({D},)")
    _rows2d(k, D, "k")
    _rows2d(v, D, "v")
    if k.shape[0] != B * n or v.shape[0] != B * n or k.stride(0) != v.stride(0):
        raise ValueError(f"k and v must hold {B * n} rows with one row stride")


def attn_pool_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, n: int, H: int,
                  ctx: torch.Tensor | None = None):
    """Single-query attention: q (H*Dh,) fp32 (projected, scaled), k / v (B*n, H*Dh) bf16 rows
    (one shared row stride) -> ctx (B, H*Dh) bf16, p (B, H, n) fp32."""
    _dev(q, k, v, ctx)
    D = q.numel()
    Dh = D // max(H, 1)
    _check_pool_kv(q, k, v, B, n, H, Dh)
    if ctx is None:
        ctx = torch.empty((B, D), dtype=torch.bfloat16, device=k.device)
    _rows2d(ctx, D, "ctx")
    p = torch.empty((B, H, n), dtype=torch.float32, device=k.device)
    _C.call("mmt_attn_pool_fwd", ptr(q), ptr(k), ptr(v), k.stride(0), B, n, H, Dh, ptr(ctx),
            ctx.stride(0), ptr(p), _C.stream_ptr())
    return ctx, p


def attn_pool_bwd(dctx: torch.Tensor, p: torch.Tensor, q: torch.Tensor, k: torch.Tensor,
                  v: torch.Tensor, dk: torch.Tensor | None = None, dv: torch.Tensor | None = None):
    """-> dk, dv (B*n, H*Dh) bf16 (halves of one (B*n, 2 H*Dh) buffer unless given), dqb (B, H*Dh)
    fp32: the per-sample query gradient."""
    _dev(dctx, p, q, k, v, dk, dv)
    B, H, n = p.shape
    D = q.numel()
    Dh = D // H
    _check_pool_kv(q, k, v, B, n, H, Dh)
    _rows2d(dctx, D, "dctx")
    if p.dtype != torch.float32 or not p.is_contiguous() or dctx.shape[0] != B:
        raise ValueError("p must be contiguous fp32 (B, H, n) and dctx hold B rows")
    if dk is None or dv is None:
        dkv = torch.empty((B * n, 2 * D), dtype=torch.bfloat16, device=k.device)
        dk, dv = dkv[:, :D], dkv[:, D:]
    _rows2d(dk, D, "dk")
    _rows2d(dv, D, "dv")
    if dk.shape[0] != B * n or dv.shape[0] != B * n or dk.stride(0) != dv.stride(0):
        raise ValueError(f"dk and dv must hold {B * n} rows with one row stride")
    dqb = torch.empty((B, D), dtype=torch.float32, device=k.device)
    _C.call("mmt_attn_pool_bwd", ptr(dctx), dctx.stride(0), ptr(p), ptr(q), ptr(k), ptr(v),
            k.stride(0), B, n, H, Dh, ptr(dk), ptr(dv), dk.stride(0), ptr(dqb), _C.stream_ptr())
    return dk, dv, dqb


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                  out: torch.Tensor | None = None):
    """Feature-axis LayerNorm of x (B, D) bf16 or fp32 rows -> y bf16, mean, rstd (B,) fp32."""
    _dev(x, gamma, beta, out)
    B, D = x.shape
    _rows2d(x, D, "x", (torch.float32, torch.bfloat16))
    if out is None:
        out = torch.empty((B, D), dtype=torch.bfloat16, device=x.device)
    _rows2d(out, D, "out")
    mean = torch.empty(B, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, dtype=torch.float32, device=x.device)
    _C.call("mmt_layernorm_fwd", ptr(x), _dtype_code(x), x.stride(0), B, D, ptr(gamma), ptr(beta),
            eps, ptr(out), out.stride(0), ptr(mean), ptr(rstd), _C.stream_ptr())
    return out, mean, rstd


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, mean, rstd, gamma, addend=None, out=None):
    """-> dx (dtype of x; + addend, dtype of x), dyxhat (B, D) fp32 (dy * xhat per row)."""
    _dev(dy, x, mean, rstd, gamma, addend, out)
    B, D = x.shape
    both = (torch.float32, torch.bfloat16)
    _rows2d(x, D, "x", both)
    _rows2d(dy, D, "dy", both)
    if addend is not None:
        _rows2d(addend, D, "addend", (x.dtype,))
    if out is None:
        out = torch.empty((B, D), dtype=x.dtype, device=x.device)
    _rows2d(out, D, "out", (x.dtype,))
    dyxhat = torch.empty((B, D), dtype=torch.float32, device=x.device)
    _C.call("mmt_layernorm_bwd", ptr(dy), _dtype_code(dy), dy.stride(0), ptr(x), _dtype_code(x),
            x.stride(0), B, D, ptr(mean), ptr(rstd), ptr(gamma), ptr(addend),
            addend.stride(0) if addend is not None else 0, ptr(out), out.stride(0), ptr(dyxhat),
            _C.stream_ptr())
    return out, dyxhat


# ------------------------------------------------------------------------------------ value tokens
VALUE_ENCODINGS = {"uniform": _C.VALUE_UNIFORM, "mu_law": _C.VALUE_MU_LAW}


def _check_value_rows(x: torch.Tensor, rows: torch.Tensor, what: str):
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError(f"{what} must be fp32 (B, L, D) with unit inner stride")
    _check_i32(rows, (rows.numel(),), "rows")


def value_tokens_fwd(values: torch.Tensor, rows: torch.Tensor, table: torch.Tensor,
                     pe: torch.Tensor, x0: torch.Tensor, encoding: str = "mu_law",
                     mu: float = 255.0, tok: torch.Tensor | None = None) -> torch.Tensor:
    """values (B, n) fp32 (row stride >= n), rows (n,) int32, table (N, D) and pe (L, D) fp32
    contiguous, x0 (B, L, D) fp32 (strided): writes x0[b, rows[j]] = table[token(b, j)] + pe[rows[j]]
    and nothing else of x0; returns the (B, n) int32 tokens (mmt_value_tokens_fwd)."""
    _dev(values, rows, table, pe, x0, tok)
    _check_value_rows(x0, rows, "x0")
    B, L, D = x0.shape
    n = rows.numel()
    if values.dtype != torch.float32 or tuple(values.shape) != (B, n) or \
            (n > 1 and values.stride(1) != 1):
        raise ValueError(f"values must be fp32 {(B, n)} with unit inner stride")
    if encoding not in VALUE_ENCODINGS:
        raise ValueError(f"encoding must be one of {sorted(VALUE_ENCODINGS)}, got {encoding!r}")
    N = table.shape[0]
    for t, shape, what in ((table, (N, D), "table"), (pe, (L, D), "pe")):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous fp32 {shape}")
    if tok is None:
        tok = torch.empty((B, n), dtype=torch.int32, device=x0.device)
    _check_i32(tok, (B, n), "tok")
    _C.call("mmt_value_tokens_fwd", ptr(values), values.stride(0) if B > 1 else n, B, n,
            VALUE_ENCODINGS[encoding], float(mu), N, ptr(table), ptr(pe), ptr(rows), D, ptr(x0),
            x0.stride(0), x0.stride(1), ptr(tok), _C.stream_ptr())
    return tok


def value_tokens_bwd(dx0: torch.Tensor, tok: torch.Tensor, rows: torch.Tensor,
                     dtable: torch.Tensor) -> torch.Tensor:
    """dtable (N, D) fp32 += the rows dx0[b, rows[j]] of the tokens tok[b, j] == k, summed in one
    fp32 accumulator per entry in ascending (b, j) order (mmt_value_tokens_bwd: no atomics)."""
    _dev(dx0, tok, rows, dtable)
    _check_value_rows(dx0, rows, "dx0")
    B, _, D = dx0.shape
    n = rows.numel()
    _check_i32(tok, (B, n), "tok")
    if dtable.dim() != 2 or dtable.dtype != torch.float32 or dtable.shape[1] != D or \
            not dtable.is_contiguous():
        raise ValueError(f"dtable must be contiguous fp32 (N, {D})")
    _C.call("mmt_value_tokens_bwd", ptr(dx0), dx0.stride(0), dx0.stride(1), B, n, ptr(tok),
            ptr(rows), D, dtable.shape[0], ptr(dtable), _C.stream_ptr())
    return dtable


# ------------------------------------------------------------------------------- point-cloud tokens
def check_pc_limits(P: int, C: int, n: int, k: int, F1: int | None = None, F2: int | None = None):
    """ValueError unless max(n, k) <= P <= 4096, 1 <= n <= 256, 1 <= k <= 32, 3 <= C <= 8 and
    (when given) F1, F2 in {32, 64, 128}: the limits of mmt_pc_sample_group / mmt_pc_embed_*."""
    for v, what in ((P, "num_points"), (C, "point_features"), (n, "the token count"),
                    (k, "num_neighbours_knn")):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what} must be an integer, got {v!r}")
    if not _C.PC_MIN_FEATURES <= C <= _C.PC_MAX_FEATURES:
        raise ValueError(f"point_features must be in {_C.PC_MIN_FEATURES} .. "
                         f"{_C.PC_MAX_FEATURES}, got {C}")
    if not 1 <= n <= _C.PC_MAX_TOKENS:
        raise ValueError(f"a cloud gives 1 .. {_C.PC_MAX_TOKENS} tokens, got {n}")
    if not 1 <= k <= _C.PC_MAX_NEIGHBOURS:
        raise ValueError(f"num_neighbours_knn must be in 1 .. {_C.PC_MAX_NEIGHBOURS}, got {k}")
    if not max(n, k) <= P <= _C.PC_MAX_POINTS:
        raise ValueError(f"num_points must be in max(n, k) = {max(n, k)} .. {_C.PC_MAX_POINTS}, "
                         f"got {P}")
    for F in (F1, F2):
        if F is not None and (isinstance(F, bool) or F not in _C.PC_HIDDEN_WIDTHS):
            raise ValueError(f"hidden widths must be among {_C.PC_HIDDEN_WIDTHS}, got {F!r}")


def _pc_points(points: torch.Tensor):
    """(B, S, P, C) fp32 whose clouds are contiguous -> (B, S, P, C, ld_b, ld_s)."""
    if points.dim() != 4 or points.dtype != torch.float32:
        raise ValueError("points must be fp32 (B, S, P, C)")
    B, S, P, C = points.shape
    if points.stride(3) != 1 or points.stride(2) != C or (S > 1 and points.stride(1) < P * C) or \
            (B > 1 and points.stride(0) < (S - 1) * points.stride(1) + P * C):
        raise ValueError("points: every (P, C) cloud must be contiguous (the batch and set "
                         "strides may be padded)")
    ld_s = points.stride(1) if S > 1 else P * C
    ld_b = points.stride(0) if B > 1 else S * ld_s
    return B, S, P, C, ld_b, ld_s


def pc_sample_group(points: torch.Tensor, n: int, k: int, start: torch.Tensor | None = None,
                    rng: torch.Tensor | None = None, sample_offset: int = 0,
                    counts: torch.Tensor | None = None):
    """Farthest-point sampling and kNN grouping of every cloud of points (B, S, P, C) fp32
    (mmt_pc_sample_group): (centroid_idx (B, S, n), neighbour_idx (B, S, n, k)) int32. The first
    centroid: start (B, S) int32 if given, else drawn from rng (the two-word RNG state) for the
    global cloud index (sample_offset + b) * S + s, else point 0. counts (B, S) int32: ragged
    clouds, the leading counts[b, s] rows of a cloud are its points and the rest is never read
    (mmt_pc_sample_group_counts: centroids repeat periodically past the count, neighbour slots
    past it repeat slot 0; a count outside [0, P] or a start not below it: device_status())."""
    _dev(points, start, rng, counts)
    B, S, P, C, ld_b, ld_s = _pc_points(points)
    check_pc_limits(P, C, n, k)
    if start is not None:
        _check_i32(start, (B, S), "start")
    if counts is not None:
        if not torch.is_tensor(counts) or counts.device != points.device:
            raise ValueError("counts must be an int32 tensor on the points' device")
        _check_i32(counts, (B, S), "counts")
    cidx = torch.empty((B, S, n), dtype=torch.int32, device=points.device)
    nidx = torch.empty((B, S, n, k), dtype=torch.int32, device=points.device)
    if counts is None:
        _C.call("mmt_pc_sample_group", ptr(points), ld_b, ld_s, B, S, P, C, n, k, ptr(start),
                ptr(rng), int(sample_offset), ptr(cidx), ptr(nidx), _C.stream_ptr())
    else:
        _C.call("mmt_pc_sample_group_counts", ptr(points), ld_b, ld_s, B, S, P, C, n, k, ptr(start),
                ptr(rng), int(sample_offset), ptr(counts), ptr(cidx), ptr(nidx), _C.stream_ptr())
    return cidx, nidx


def depth_unproject(depth: torch.Tensor, intrinsics: torch.Tensor, num_points: int,
                    depth_scale: float = 0.001, z_min: float = 0.1, z_max: float = 3.0,
                    pose: torch.Tensor | None = None, rgb: torch.Tensor | None = None,
                    out: torch.Tensor | None = None, counts: torch.Tensor | None = None):
    """Depth images (B, S, H, W), uint16 or fp32, contiguous -> (points fp32 (B, S, P, C),
    counts int32 (B, S)) (mmt_depth_unproject): the valid pixels back-projected with intrinsics
    fp32 (B, S, 4) = fx fy cx cy, moved by pose fp32 (B, S, 3, 4) if given, coloured by rgb uint8
    (B, S, H, W, 3) if given (C = 6, else 3); at most P = num_points of them, evenly strided in
    raster order; the slots past counts are zeros. ValueError before any launch: dtypes, shapes,
    devices, 1 <= P <= 4096, H W <= 2^20 and a multiple of 8 (uint16) / 4 (fp32), depth_scale > 0,
    z_min <= z_max. fx, fy (device data) must be non-zero: the coordinates are unspecified else."""
    if not torch.is_tensor(depth) or depth.dim() != 4 or depth.dtype not in (torch.uint16,
                                                                             torch.float32):
        raise ValueError("depth must be a uint16 or fp32 (B, S, H, W) tensor")
    if not depth.is_cuda:
        raise ValueError("depth must live on the GPU")
    _dev(depth, intrinsics, pose, rgb, out, counts)
    B, S, H, W = depth.shape
    f32 = depth.dtype == torch.float32
    if isinstance(num_points, bool) or not isinstance(num_points, int) or \
            not 1 <= num_points <= _C.PC_MAX_POINTS:
        raise ValueError(f"num_points must be an integer in 1 .. {_C.PC_MAX_POINTS}, "
                         f"got {num_points!r}")
    if B < 1 or S < 1 or H < 1 or W < 1 or H * W > _C.DEPTH_MAX_PIXELS:
        raise ValueError(f"depth {tuple(depth.shape)}: need B, S, H, W >= 1 and H * W <= "
                         f"{_C.DEPTH_MAX_PIXELS}")
    epv = 4 if f32 else 8
    if not depth.is_contiguous() or (H * W) % epv or depth.data_ptr() % 16:
        raise ValueError(f"depth must be contiguous and 16-B aligned with H * W a multiple of "
                         f"{epv} (images are read as 16-B vectors), got H * W = {H * W}")
    depth_scale, z_min, z_max = float(depth_scale), float(z_min), float(z_max)
    if not depth_scale > 0.0 or not z_min <= z_max:
        raise ValueError(f"need depth_scale > 0 and z_min <= z_max, got {depth_scale}, "
                         f"({z_min}, {z_max})")
    for t, shape, dt, what in ((intrinsics, (B, S, 4), torch.float32, "intrinsics"),
                               (pose, (B, S, 3, 4), torch.float32, "pose"),
                               (rgb, (B, S, H, W, 3), torch.uint8, "rgb")):
        if t is None and what != "intrinsics":
            continue
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or \
                not t.is_contiguous() or t.device != depth.device:
            raise ValueError(f"{what} must be a contiguous {dt} {shape} tensor on the depth's "
                             "device")
    C = 6 if rgb is not None else 3
    P = num_points
    if out is None:
        out = torch.empty((B, S, P, C), dtype=torch.float32, device=depth.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, S, P, C) or \
            not out.is_contiguous() or out.device != depth.device:
        raise ValueError(f"out must be contiguous fp32 {(B, S, P, C)} on the depth's device")
    if counts is None:
        counts = torch.empty((B, S), dtype=torch.int32, device=depth.device)
    elif counts.device != depth.device:
        raise ValueError("counts must live on the depth's device")
    else:
        _check_i32(counts, (B, S), "counts")
    _C.call("mmt_depth_unproject", ptr(depth), int(f32), B, S, H, W, ptr(intrinsics), ptr(pose),
            ptr(rgb), depth_scale, z_min, z_max, P, ptr(out), ptr(counts), _C.stream_ptr())
    return out, counts


AUGMENT_FIELDS = ("scale_lo", "scale_hi", "ratio_lo", "ratio_hi", "brightness", "contrast_lo",
                  "contrast_hi", "sat_lo", "sat_hi")   # a row of mmt_image_augment's cam_params


def check_augment_tables(image_camera, cam_params, n_images: int | None = None):
    """The host values behind mmt_image_augment's two device tables, checked: image_camera, one
    camera index per image slot, and cam_params, one row of AUGMENT_FIELDS per camera. Returns
    (list of ints, list of 9-tuples of floats). ValueError: no or more than 64 image slots (or not
    n_images of them), no or more than 16 cameras, a row that is not 9 finite numbers, a camera
    index outside 0 .. n_cam - 1 or no integer, lo > hi in a range, scale_lo <= 0, scale_hi > 1,
    ratio_lo <= 0, brightness outside [0, 1], a negative contrast or saturation bound."""
    import math
    try:
        rows = [tuple(float(v) for v in row) for row in cam_params]
        cams = list(image_camera)
    except (TypeError, ValueError):
        raise ValueError("image_camera must be a sequence of camera indices and cam_params a "
                         f"sequence of rows {AUGMENT_FIELDS}") from None
    n_cam = len(rows)
    if not 1 <= n_cam <= _C.AUGMENT_MAX_CAMERAS:
        raise ValueError(f"cam_params holds {n_cam} cameras, need 1 .. {_C.AUGMENT_MAX_CAMERAS}")
    if not 1 <= len(cams) <= _C.AUGMENT_MAX_IMAGES or (n_images is not None
                                                        and len(cams) != n_images):
        want = f"{n_images}" if n_images is not None else f"1 .. {_C.AUGMENT_MAX_IMAGES}"
        raise ValueError(f"image_camera names {len(cams)} image slots, need {want}")
    for c in cams:
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < n_cam:
            raise ValueError(f"image_camera entry {c!r} is no camera index in 0 .. {n_cam - 1}")
    for i, row in enumerate(rows):
        if len(row) != 9 or not all(math.isfinite(v) for v in row):
            raise ValueError(f"camera {i}: need 9 finite numbers {AUGMENT_FIELDS}, got {row}")
        slo, shi, rlo, rhi, br, clo, chi, tlo, thi = row
        if slo > shi or rlo > rhi or clo > chi or tlo > thi:
            raise ValueError(f"camera {i}: a range has lo > hi: {row}")
        if not 0.0 < slo or shi > 1.0:
            raise ValueError(f"camera {i}: need 0 < scale_lo <= scale_hi <= 1, got ({slo}, {shi})")
        if not 0.0 < rlo:
            raise ValueError(f"camera {i}: need ratio_lo > 0, got {rlo}")
        if not 0.0 <= br <= 1.0:
            raise ValueError(f"camera {i}: brightness {br} outside [0, 1]")
        if clo < 0.0 or tlo < 0.0:
            raise ValueError(f"camera {i}: contrast and saturation bounds must be >= 0, got "
                             f"({clo}, {chi}), ({tlo}, {thi})")
    return [int(c) for c in cams], rows


def image_augment_workspace(B: int, I: int) -> int:
    """Bytes of mmt_image_augment's workspace for B samples of I image slots."""
    return _C.call("mmt_image_augment_workspace", int(B), int(I))


def image_augment(images: torch.Tensor, rng: torch.Tensor, image_camera: torch.Tensor,
                  cam_params: torch.Tensor, sample_offset: int = 0,
                  out: torch.Tensor | None = None, params_out: torch.Tensor | None = None,
                  workspace: torch.Tensor | None = None, tables=None) -> torch.Tensor:
    """uint8 camera frames (B, I, H, W, 3), contiguous -> their augmented copy (mmt_image_augment,
    include/mmt_api.h "image augmentation"): a random resized crop resampled bilinearly to (H, W)
    plus brightness, contrast and saturation jitter, one draw per (global sample sample_offset + b,
    camera) from rng = the int32 {seed, step} words on the device. image_camera: int32 (I,) on the
    device, the camera of each image slot; cam_params: fp32 (n_cam, 9) on the device, a row of
    AUGMENT_FIELDS per camera. params_out (optional): fp32 (B, n_cam, 8), receives w, h, x0, y0,
    d, fc, fs, 0. workspace (optional): a uint8 buffer of image_augment_workspace(B, I) bytes;
    allocated when missing. tables: the host values of (image_camera, cam_params) as
    check_augment_tables returned them; None reads the two tensors back (a synchronisation: pass
    tables inside a graph capture). ValueError before any launch: a dtype, device, contiguity or
    shape fault, H or W above 2048, I above 64, out overlapping images, and
    check_augment_tables' faults."""
    for t, what in ((images, "images"), (rng, "rng"), (image_camera, "image_camera"),
                    (cam_params, "cam_params")):
        if not torch.is_tensor(t):
            raise ValueError(f"{what} must be a tensor")
    if images.dtype != torch.uint8 or images.dim() != 5 or images.shape[-1] != 3:
        raise ValueError(f"images must be uint8 (B, I, H, W, 3), got {images.dtype} "
                         f"{tuple(images.shape)}")
    if not images.is_cuda:
        raise ValueError("images must live on the GPU")
    dev = images.device
    for t, what in ((rng, "rng"), (image_camera, "image_camera"), (cam_params, "cam_params"),
                    (out, "out"), (params_out, "params_out"), (workspace, "workspace")):
        if t is not None and t.device != dev:
            raise ValueError(f"{what} must live on the images' device")
    B, I, H, W, _ = images.shape
    if B < 1 or not 1 <= I <= _C.AUGMENT_MAX_IMAGES or B * I > _C.AUGMENT_MAX_FRAMES or \
            not 1 <= H <= _C.AUGMENT_MAX_SIDE or not 1 <= W <= _C.AUGMENT_MAX_SIDE:
        raise ValueError(f"images {tuple(images.shape)}: need B >= 1, 1 <= I <= "
                         f"{_C.AUGMENT_MAX_IMAGES}, 1 <= H, W <= {_C.AUGMENT_MAX_SIDE}")
    if not images.is_contiguous() or images.data_ptr() % 16:
        raise ValueError("images must be contiguous and 16-B aligned")
    if rng.dtype != torch.int32 or rng.numel() != 2 or not rng.is_contiguous():
        raise ValueError("rng must be the contiguous int32 {seed, step} pair")
    _check_i32(image_camera, (I,), "image_camera")
    if cam_params.dtype != torch.float32 or cam_params.dim() != 2 or cam_params.shape[1] != 9 or \
            not cam_params.is_contiguous():
        raise ValueError("cam_params must be contiguous fp32 (n_cam, 9)")
    n_cam = cam_params.shape[0]
    if tables is None:
        tables = check_augment_tables(image_camera.tolist(), cam_params.tolist(), I)
    elif len(tables[0]) != I or len(tables[1]) != n_cam:
        raise ValueError(f"tables describe {len(tables[0])} image slots and {len(tables[1])} "
                         f"cameras, the tensors {I} and {n_cam}")
    if isinstance(sample_offset, bool) or int(sample_offset) != sample_offset or sample_offset < 0:
        raise ValueError(f"sample_offset must be an integer >= 0, got {sample_offset!r}")
    if out is None:
        out = torch.empty_like(images)
    else:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.shape != images.shape or \
                not out.is_contiguous() or out.data_ptr() % 16:
            raise ValueError("out must be a contiguous 16-B aligned uint8 tensor of the images' "
                             "shape")
        n = images.numel()
        if out.data_ptr() < images.data_ptr() + n and images.data_ptr() < out.data_ptr() + n:
            raise ValueError("out must not overlap images (the crop gathers: no in-place form)")
    if params_out is not None and (params_out.dtype != torch.float32
                                   or tuple(params_out.shape) != (B, n_cam, 8)
                                   or not params_out.is_contiguous()):
        raise ValueError(f"params_out must be contiguous fp32 {(B, n_cam, 8)}")
    need = image_augment_workspace(B, I)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or \
            not workspace.is_contiguous() or workspace.data_ptr() % 16:
        raise ValueError(f"workspace must be a contiguous 16-B aligned uint8 buffer of at least "
                         f"{need} bytes")
    _C.call("mmt_image_augment", ptr(images), B, I, H, W, ptr(rng), int(sample_offset),
            ptr(image_camera), ptr(cam_params), n_cam, ptr(out), ptr(params_out), ptr(workspace),
            workspace.numel(), _C.stream_ptr())
    return out


def _pc_weights(C: int, w1, b1, w2, b2, w_out, b_out):
    F1, F2, D = w1.shape[1], w2.shape[1], w_out.shape[1]
    for t, shape, what in ((w1, (2 * C, F1), "w1"), (b1, (F1,), "b1"), (w2, (F1, F2), "w2"),
                           (b2, (F2,), "b2"), (w_out, (F2, D), "w_out"), (b_out, (D,), "b_out")):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous fp32 {shape}, got {tuple(t.shape)}")
    return F1, F2, D


def _pc_rows(x: torch.Tensor, rows: torch.Tensor, B: int, S: int, n: int, D: int, what: str):
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1 or x.shape[0] != B or \
            x.shape[2] != D:
        raise ValueError(f"{what} must be fp32 ({B}, L, {D}) with unit inner stride")
    _check_i32(rows, (S * n,), "rows")


def pc_embed_fwd(points, cidx, nidx, w1, b1, w2, b2, w_out, b_out, pe, rows, x0):
    """The rows of the point-cloud tokens (mmt_pc_embed_fwd): x0[b, rows[s n + m]] =
    (max_k relu(relu(feat W1 + b1) W2 + b2)) W_out + b_out + pe[rows[s n + m]] and no other row of
    x0 (B, L, D) fp32 (strided). Returns argmax (B, S, n, F2) uint8, the backward's saved state."""
    _dev(points, cidx, nidx, w1, b1, w2, b2, w_out, b_out, pe, rows, x0)
    B, S, P, C, ld_b, ld_s = _pc_points(points)
    n, k = cidx.shape[-1], nidx.shape[-1]
    F1, F2, D = _pc_weights(C, w1, b1, w2, b2, w_out, b_out)
    check_pc_limits(P, C, n, k, F1, F2)
    _check_i32(cidx, (B, S, n), "centroid_idx")
    _check_i32(nidx, (B, S, n, k), "neighbour_idx")
    _pc_rows(x0, rows, B, S, n, D, "x0")
    if pe.dtype != torch.float32 or tuple(pe.shape) != (x0.shape[1], D) or not pe.is_contiguous():
        raise ValueError(f"pe must be contiguous fp32 {(x0.shape[1], D)}")
    argmax = torch.empty((B, S, n, F2), dtype=torch.uint8, device=points.device)
    _C.call("mmt_pc_embed_fwd", ptr(points), ld_b, ld_s, B, S, P, C, n, k, ptr(cidx), ptr(nidx), F1,
            F2, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w_out), ptr(b_out), ptr(pe), ptr(rows), D,
            ptr(x0), x0.stride(0), x0.stride(1), ptr(argmax), _C.stream_ptr())
    return argmax


def pc_embed_bwd(dx0, rows, points, cidx, nidx, argmax, w1, b1, w2, b2, w_out, grads):
    """grads = (dw1, db1, dw2, db2, dw_out, db_out), fp32 like the weights: each += its gradient
    from the rows dx0[b, rows[s n + m]] (mmt_pc_embed_bwd: chunk partials summed in a fixed order
    and added once, no atomics)."""
    dw1, db1, dw2, db2, dw_out, db_out = grads
    _dev(dx0, rows, points, cidx, nidx, argmax, w1, b1, w2, b2, w_out, *grads)
    B, S, P, C, ld_b, ld_s = _pc_points(points)
    n, k = cidx.shape[-1], nidx.shape[-1]
    F1, F2, D = _pc_weights(C, w1, b1, w2, b2, w_out, db_out)
    _pc_weights(C, dw1, db1, dw2, db2, dw_out, db_out)
    check_pc_limits(P, C, n, k, F1, F2)
    _check_i32(cidx, (B, S, n), "centroid_idx")
    _check_i32(nidx, (B, S, n, k), "neighbour_idx")
    if argmax.dtype != torch.uint8 or tuple(argmax.shape) != (B, S, n, F2) or \
            not argmax.is_contiguous():
        raise ValueError(f"argmax must be contiguous uint8 {(B, S, n, F2)}")
    _pc_rows(dx0, rows, B, S, n, D, "dx0")
    nbytes = _C.call("mmt_pc_embed_bwd_workspace", B, S, n, C, F1, F2, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    _C.call("mmt_pc_embed_bwd", ptr(dx0), dx0.stride(0), dx0.stride(1), ptr(rows), D, ptr(points),
            ld_b, ld_s, B, S, P, C, n, k, ptr(cidx), ptr(nidx), ptr(argmax), F1, F2, ptr(w1),
            ptr(b1), ptr(w2), ptr(b2), ptr(w_out), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2),
            ptr(dw_out), ptr(db_out), ptr(ws), nbytes, _C.stream_ptr())
    return grads


# ------------------------------------------------------------------------------------------ QK-norm
QK_NORM_WIDTHS = _C.QK_NORM_WIDTHS


def _qk_norm_args(qkv: torch.Tensor, H: int, Dh: int, q_scale, k_scale, what: str):
    """(n_tokens, dtype code, ld) of a packed (rows, >= 3 H Dh) or (B, L, >= 3 H Dh) buffer with
    unit inner stride and one row stride. The library checks the rest (Dh, ld, alignment, dtype:
    MMTError); scales that are not contiguous fp32 (Dh,) are an MMTError here, before any launch."""
    if qkv.dim() == 3 and (qkv.shape[0] == 1 or qkv.stride(0) == qkv.shape[1] * qkv.stride(1)):
        N, ld = qkv.shape[0] * qkv.shape[1], qkv.stride(1)
    elif qkv.dim() == 2:
        N, ld = qkv.shape[0], qkv.stride(0)
    else:
        raise ValueError(f"{what} must be (rows, 3 H Dh) or (B, L, 3 H Dh) with one row stride")
    W = qkv.shape[-1]
    if (W > 1 and qkv.stride(-1) != 1) or N < 1:
        raise ValueError(f"{what} must have unit inner stride and at least one row")
    if N == 1 or W < 3 * H * Dh:   # a buffer narrower than 3 H Dh: the library rejects its ld
        ld = W
    for s, name in ((q_scale, "q_scale"), (k_scale, "k_scale")):
        if s.dtype != torch.float32 or tuple(s.shape) != (Dh,) or not s.is_contiguous():
            raise _C.MMTError(f"{what}: {name} must be contiguous fp32 ({Dh},), got {s.dtype} "
                              f"{tuple(s.shape)}")
    return N, DT.get(qkv.dtype, -1), ld


def qk_norm_fwd(qkv: torch.Tensor, H: int, Dh: int, q_scale: torch.Tensor, k_scale: torch.Tensor,
                eps: float = 1e-6, save: bool = True):
    """LayerNorm(use_bias=False) over the head dimension of the q and k thirds of the packed qkv
    (rows, 3 H Dh) / (B, L, 3 H Dh) fp32 or bf16 buffer, in place (mmt_qk_norm_fwd); the V third is
    untouched. Returns qk_pre (rows, 2 H Dh), the pre-norm q and k for qk_norm_bwd (None with
    save=False: an evaluation-only forward)."""
    _dev(qkv, q_scale, k_scale)
    N, code, ld = _qk_norm_args(qkv, H, Dh, q_scale, k_scale, "qk_norm_fwd")
    pre = torch.empty((N, 2 * H * Dh), dtype=qkv.dtype, device=qkv.device) if save else None
    _C.call("mmt_qk_norm_fwd", ptr(qkv), code, ld, N, H, Dh, ptr(q_scale), ptr(k_scale), float(eps),
            ptr(pre), _C.stream_ptr())
    return pre


def qk_norm_bwd(dqkv: torch.Tensor, qk_pre: torch.Tensor, H: int, Dh: int, q_scale: torch.Tensor,
                k_scale: torch.Tensor, dq_scale: torch.Tensor, dk_scale: torch.Tensor,
                eps: float = 1e-6) -> torch.Tensor:
    """dqkv (the layout of qkv): its q and k thirds become the gradient of the pre-norm q and k,
    in place; dq_scale / dk_scale (Dh,) fp32 += the scale gradients, ordered sums without atomics
    (mmt_qk_norm_bwd). Returns dqkv."""
    _dev(dqkv, qk_pre, q_scale, k_scale, dq_scale, dk_scale)
    N, code, ld = _qk_norm_args(dqkv, H, Dh, q_scale, k_scale, "qk_norm_bwd")
    _qk_norm_args(dqkv, H, Dh, dq_scale, dk_scale, "qk_norm_bwd (gradients)")
    if qk_pre.dtype != dqkv.dtype or tuple(qk_pre.shape) != (N, 2 * H * Dh) or \
            not qk_pre.is_contiguous():
        raise ValueError(f"qk_pre must be contiguous {dqkv.dtype} {(N, 2 * H * Dh)}")
    nbytes = _C.call("mmt_qk_norm_bwd_workspace", N, H, Dh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dqkv.device)
    _C.call("mmt_qk_norm_bwd", ptr(dqkv), code, ld, N, H, Dh, ptr(qk_pre), ptr(q_scale),
            ptr(k_scale), float(eps), ptr(dq_scale), ptr(dk_scale), ptr(ws), nbytes,
            _C.stream_ptr())
    return dqkv
