"""GPU: the value-token kernels (csrc/values.hip: mmt_value_tokens_fwd / _bwd) against the numpy
restatement tests/value_tokens_ref.py, bit for bit, and the sequence assembly's early-out for the
rows they own (kind 3).

Inputs are bin-centre values (value_tokens_ref.bin_centre_values: at least a quarter of a bin from
every edge; tests/test_value_tokens_cpu.py shows fp32 reproduces their token with log1p and with
log(1 + x)), so every token is demanded exactly, with the fixed points (-1, 0, 1, +-inf, NaN, 1.5,
-7) on top. The forward is one fp32 add and the backward a sequential fp32 sum in a fixed order:
both are compared bitwise."""
import numpy as np
import pytest
import torch

from tests import value_tokens_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 16), (3, 7, 64, 256), (2, 8, 384, 1024), (5, 5, 200, 2)]   # (B, n, D, N)
SENTINEL = -12345.5


def _K():
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    return K


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(n, L0):
    """Non-contiguous, ascending sequence rows: [3, 4, 9, ...] style."""
    rows = np.array([3 + j + 4 * (j // 2) for j in range(n)], np.int32)
    assert rows[-1] < L0 and len(set(rows.tolist())) == n
    return rows


def _case(B, n, D, N, mu, encoding, seed):
    rng = np.random.default_rng(seed)
    want = rng.integers(0, N, (B, n))
    vals = R.bin_centre_values(want, N, mu, encoding, rng)
    flat = vals.reshape(-1)
    fp = R.FIXED_POINTS[: flat.size]             # the fixed points over the first elements
    flat[: fp.size] = fp
    want = want.reshape(-1)
    want[: fp.size] = R.fixed_point_tokens(N)[: fp.size]
    table = rng.standard_normal((N, D)).astype(np.float32)
    L0 = 3 + n + 4 * (n // 2) + 2
    pe = rng.standard_normal((L0, D)).astype(np.float32)
    return vals, want.reshape(B, n).astype(np.int32), table, pe, L0


@pytest.mark.parametrize("B,n,D,N", SHAPES)
@pytest.mark.parametrize("encoding", R.ENCODINGS)
@pytest.mark.parametrize("mu", [255.0, 100.0])
@pytest.mark.parametrize("padded", [False, True])
def test_forward_tokens_rows_and_nothing_else(dev, B, n, D, N, encoding, mu, padded):
    K = _K()
    vals, want, table, pe, L0 = _case(B, n, D, N, mu, encoding, seed=B * 1000 + N)
    np.testing.assert_array_equal(R.tokens(vals, N, mu, encoding), want)   # the reference itself
    rows = _rows(n, L0)
    # a padded batch stride (and padded value rows): views into larger buffers
    buf = torch.full((B, L0 + (3 if padded else 0), D), SENTINEL, device=dev)
    x0 = buf[:, :L0]
    vbuf = torch.full((B, n + (5 if padded else 0)), 0.25, device=dev)
    v = vbuf[:, :n]
    v.copy_(torch.from_numpy(vals))
    tok = K.value_tokens_fwd(v, torch.from_numpy(rows).to(dev), torch.from_numpy(table).to(dev),
                             torch.from_numpy(pe).to(dev), x0, encoding, mu)
    torch.cuda.synchronize()
    assert tok.dtype == torch.int32 and tuple(tok.shape) == (B, n)
    np.testing.assert_array_equal(tok.cpu().numpy(), want)                 # every element, exact
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(_bits(got[:, rows]), _bits(R.forward_rows(want, table, pe, rows)))
    other = np.ones(got.shape[1], bool)
    other[rows] = False
    assert (got[:, other] == np.float32(SENTINEL)).all()                   # no other row touched
    K.device_status()


def _bwd_case(dev, B, n, D, N, tok, seed, pad=0):
    rng = np.random.default_rng(seed)
    L0 = 3 + n + 4 * (n // 2) + 2
    rows = _rows(n, L0)
    full = rng.standard_normal((B, L0 + pad, D)).astype(np.float32)
    dx0 = torch.from_numpy(full).to(dev)[:, :L0]
    return dx0, full[:, :L0], rows, torch.from_numpy(rows).to(dev), \
        torch.from_numpy(np.ascontiguousarray(tok, np.int32)).to(dev)


@pytest.mark.parametrize("B,n,D,N", SHAPES + [(64, 8, 64, 16)])
def test_backward_is_the_ordered_sum(dev, B, n, D, N):
    """Spread tokens; a non-zero initial dtable; a second run into a fresh buffer, bitwise equal;
    a padded batch stride."""
    K = _K()
    rng = np.random.default_rng(B + N)
    tok = rng.integers(0, N, (B, n)).astype(np.int32)
    dx0, dx0_np, rows, rows_d, tok_d = _bwd_case(dev, B, n, D, N, tok, seed=N, pad=2)
    init = rng.standard_normal((N, D)).astype(np.float32)
    a = K.value_tokens_bwd(dx0, tok_d, rows_d, torch.zeros((N, D), device=dev))
    b = K.value_tokens_bwd(dx0, tok_d, rows_d, torch.from_numpy(init).to(dev))
    c = K.value_tokens_bwd(dx0, tok_d, rows_d, torch.zeros((N, D), device=dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(a), _bits(R.table_grad(dx0_np, tok, rows, N)))
    np.testing.assert_array_equal(_bits(b), _bits(R.table_grad(dx0_np, tok, rows, N, init)))
    assert torch.equal(a, c)
    K.device_status()


def test_backward_all_tokens_in_one_bin(dev):
    """B = 64, n = 8: 512 ordered adds into one table entry (an order-dependent fp32 sum: any
    other order, tree or atomic arrival gives other bits)."""
    K = _K()
    B, n, D, N, k = 64, 8, 200, 256, 77
    tok = np.full((B, n), k, np.int32)
    dx0, dx0_np, rows, rows_d, tok_d = _bwd_case(dev, B, n, D, N, tok, seed=5)
    want = R.table_grad(dx0_np, tok, rows, N)
    rev = np.zeros(D, np.float32)                      # the inputs do tell orders apart
    for b in reversed(range(B)):
        for j in reversed(range(n)):
            rev = rev + dx0_np[b, rows[j]]
    assert not np.array_equal(_bits(rev), _bits(want[k]))
    got = K.value_tokens_bwd(dx0, tok_d, rows_d, torch.zeros((N, D), device=dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert not got[:k].any() and not got[k + 1:].any()
    K.device_status()


def test_backward_bits_do_not_depend_on_the_deterministic_mode(dev):
    """dtable inside the registered gradient buffer of a store in deterministic mode: the same
    bits as outside the mode, and the fixed-point shadow stays empty (no atomics to redirect)."""
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore, const
    K = _K()
    B, n, D, N = 64, 8, 64, 16
    rng = np.random.default_rng(9)
    tok = rng.integers(0, 3, (B, n)).astype(np.int32)         # ~170 adds per busy entry
    dx0, dx0_np, rows, rows_d, tok_d = _bwd_case(dev, B, n, D, N, tok, seed=11)
    store = ParamStore()
    emb = store.add("ValueTokenizer_0/embedding", (N, D), const(0.0))
    store.materialize(dev, 0)
    store.zero_grad()
    K.value_tokens_bwd(dx0, tok_d, rows_d, emb.grad)
    torch.cuda.synchronize()
    plain = emb.grad.clone()
    with store.deterministic():
        store.zero_grad()
        K.value_tokens_bwd(dx0, tok_d, rows_d, emb.grad)
        torch.cuda.synchronize()
        assert not store.det_fx.any()
        store.det_flush()
        torch.cuda.synchronize()
        det = emb.grad.clone()
    np.testing.assert_array_equal(_bits(plain), _bits(R.table_grad(dx0_np, tok, rows, N)))
    assert torch.equal(plain, det)
    K.device_status()


def test_out_of_range_token_is_skipped_and_reported(dev):
    """One saved token equal to N (written by the test): the backward completes, the status word
    names the row-index check once and is clear afterwards, and every entry of dtable is the
    ordered sum over the valid tokens. Nothing faults: the entry is skipped, never followed."""
    from multi_modal_transformers_tokenmerge_amd._C import MMTError
    K = _K()
    B, n, D, N = 3, 7, 64, 256
    rng = np.random.default_rng(3)
    tok = rng.integers(0, N, (B, n)).astype(np.int32)
    tok[1, 4] = N
    dx0, dx0_np, rows, rows_d, tok_d = _bwd_case(dev, B, n, D, N, tok, seed=4)
    K.device_status()                                           # clean start
    got = K.value_tokens_bwd(dx0, tok_d, rows_d, torch.zeros((N, D), device=dev))
    with pytest.raises(MMTError, match="row index out of range"):
        K.device_status()
    K.device_status()                                           # cleared by the report
    np.testing.assert_array_equal(_bits(got), _bits(R.table_grad(dx0_np, tok, rows, N)))


def test_assemble_leaves_value_rows_alone(dev):
    """mmt_seq_assemble_fwd does not write a row of kind 3 and mmt_seq_assemble_bwd does not read
    one: the sentinel survives, and d(readout_pe) sums the readout rows only (before the
    early-out a value row fell into the readout branch and indexed readout_pe by its slot)."""
    from multi_modal_transformers_tokenmerge_amd import _C
    B, D, T, NI, NV, NR = 2, 64, 2, 3, 4, 2
    kinds = [(0, j) for j in range(T)] + [(1, j) for j in range(NI)] + \
            [(3, j) for j in range(NV)] + [(2, j) for j in range(NR)]
    L = len(kinds)
    row_src = torch.tensor([(k << 24) | j for k, j in kinds], dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(0)
    text = torch.randn((B, T, D), generator=g).bfloat16().to(dev)
    img = torch.randn((B, NI, D), generator=g).bfloat16().to(dev)
    Q = 4
    rt = torch.randint(0, Q, (B, NI), generator=g, dtype=torch.int32).to(dev)
    ct = torch.randint(0, Q, (B, NI), generator=g, dtype=torch.int32).to(dev)
    row_emb = torch.randn((Q, D), generator=g).to(dev)
    col_emb = torch.randn((Q, D), generator=g).to(dev)
    rpe = torch.randn((NR, D), generator=g).to(dev)            # fewer rows than value slots
    pe = torch.randn((L, D), generator=g).to(dev)
    x0 = torch.full((B, L, D), SENTINEL, device=dev)
    _C.call("mmt_seq_assemble_fwd", B, L, D, _C.ptr(row_src), _C.ptr(text), T, _C.ptr(img), NI,
            _C.ptr(rt), _C.ptr(ct), _C.ptr(row_emb), _C.ptr(col_emb), _C.ptr(rpe), _C.ptr(pe),
            _C.ptr(x0), _C.stream_ptr())
    torch.cuda.synchronize()
    vrows = [l for l, (k, _) in enumerate(kinds) if k == 3]
    rrows = [l for l, (k, _) in enumerate(kinds) if k == 2]
    assert (x0[:, vrows] == SENTINEL).all()
    assert torch.equal(x0[:, rrows], (rpe + pe[rrows])[None].expand(B, -1, -1))
    assert torch.equal(x0[:, :T], text.float() + pe[:T])
    assert not (x0[:, T:T + NI] == SENTINEL).any()
    dx0 = torch.randn((B, L, D), generator=g).to(dev)
    dtext = torch.zeros((B, T, D), dtype=torch.bfloat16, device=dev)
    dimg = torch.zeros((B, NI, D), dtype=torch.bfloat16, device=dev)
    img_rows = torch.arange(T, T + NI, dtype=torch.int32, device=dev)
    # the gradient sits in a larger buffer whose other elements must stay as they are
    dbuf = torch.full((NR + NV + 2, D), SENTINEL, device=dev)
    drpe = dbuf[1:1 + NR]
    drpe.zero_()
    _C.call("mmt_seq_assemble_bwd", B, L, D, _C.ptr(row_src), _C.ptr(dx0), _C.ptr(dtext), T,
            _C.ptr(dimg), NI, _C.ptr(rt), _C.ptr(ct), _C.ptr(img_rows), Q, None, None,
            _C.ptr(drpe), _C.stream_ptr())
    torch.cuda.synchronize()
    want = dx0[:, rrows].double().sum(0)
    np.testing.assert_allclose(drpe.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=1e-6)
    assert (dbuf[0] == SENTINEL).all() and (dbuf[1 + NR:] == SENTINEL).all()
    assert torch.equal(dimg, dx0[:, T:T + NI].bfloat16())
    _C.call("mmt_device_status", _C.stream_ptr())
