"""GPU numerics of the attention key bias (ToMe proportional attention):
logits = scale q.k + key_bias[b, k], then mask, softmax and dropout as without it.

Every kernel path that takes the bias (resident forward in both ONEPASS forms, two-phase resident
backward, tiled forward incl. the one-wave L <= 32 form, tiled dQ and dK/dV at Dh 64 / 128 / 256)
against a plain fp32 torch attention on the same bf16 inputs, with the bars of
tests/test_attn_norm_gpu.py: O rel-L2 < 1e-2, dq / dk / dv rel-L2 < 2e-2, the fused QKV bias
gradient against the column sums of dqkv. The bias rows' padding [L, roundup(L, 64)) is filled with
1e30 to prove the kernels ignore it."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 1e30  # what the ignored tail of a key_bias row holds in these tests


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def dense_mask(starts, lens, vis, L, dev, causal=None):
    sid = torch.zeros(L, dtype=torch.long)
    for i, (s, n) in enumerate(zip(starts, lens)):
        sid[s:s + n] = i
    v = torch.tensor(vis, dtype=torch.long)
    m = ((v[sid][:, None] >> sid[None, :]) & 1).bool()
    for i, c in enumerate(causal or []):
        if c:
            s, n = starts[i], lens[i]
            m[s:s + n, s:s + n] &= torch.tril(torch.ones((n, n), dtype=torch.bool))
    return m.to(dev)


def bits_to_keep(bits, L):
    """(L, L) bool keep mask from the query-word image of K.dropout_bits' square layout."""
    b = bits[0].cpu().numpy().view(np.uint32)                      # (W, LP)
    W, LP = b.shape
    ex = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)
    p = np.arange(LP)
    idx = (p & ~7) | ((p & 1) << 2) | ((p >> 1) & 3)
    m = np.zeros((W * 32, LP), dtype=bool)
    m[:, idx] = ex.transpose(0, 2, 1).reshape(W * 32, LP)
    return torch.from_numpy(np.ascontiguousarray(m[:L, :L]))


def ref_attention(qkv, H, scale, mask, keep, keep_prob, key_bias=None):
    """fp32 attention with ref_attention's semantics of tests/test_attn_norm_gpu.py plus the key
    bias; also returns the softmax normaliser lse (B, H, L)."""
    B, L, three = qkv.shape
    Dh = three // (3 * H)
    q, k, v = qkv.float().view(B, L, 3, H, Dh).unbind(2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    if key_bias is not None:
        s = s + key_bias[:, None, None, :L]
    if mask is not None:
        s = torch.where(mask[None, None], s, torch.finfo(torch.float32).min)
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = torch.where(keep[None, None], p / keep_prob, torch.zeros_like(p))
    return torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(B, L, H * Dh), torch.logsumexp(s, -1)


def make_table(K, mode, L, dev):
    """(SetTable or None, dense mask or None, (start, len) of the set that carries sizes)."""
    if mode == "none":
        return None, None, (L // 4, L // 2)
    if mode == "octo":  # T sees T; I sees T, I; R sees T, I, R
        nt = min(32, L // 4)
        starts, lens, vis = [0, nt, L - 4], [nt, L - nt - 4, 4], [0b001, 0b011, 0b111]
        return K.SetTable(starts, lens, vis), dense_mask(starts, lens, vis, L, dev), (nt, L - nt - 4)
    # the causal two-step table of test_resident_attention_vs_tiled_and_torch
    n = (L - 7) // 2
    starts, lens = [0, 3, 3 + n, 4 + n, 7 + n], [3, n, 1, 3, L - 7 - n]
    vis = [0b00001, 0b00011, 0b00111, 0b01001, 0b11011]
    causal = [False, True, False, False, True]
    return (K.SetTable(starts, lens, vis, causal), dense_mask(starts, lens, vis, L, dev, causal),
            (3, n))


def make_bias(K, B, L, rng_set, dev, g, kind="sizes"):
    """fp32 (B, attn_lp(L)): log of random integers 1..8 on one set's range and 0 elsewhere
    ("sizes"), or uniform in [-4, 4] on every key ("generic"); different rows per sample; the
    padding holds PAD."""
    kb = torch.zeros((B, K.attn_lp(L)))
    if kind == "sizes":
        s0, n = rng_set
        kb[:, s0:s0 + n] = torch.log(torch.randint(1, 9, (B, n), generator=g).float())
    else:
        kb[:, :L] = torch.rand((B, L), generator=g) * 8 - 4
    kb[:, L:] = PAD
    return kb.to(dev)


def expected_routes(L, Dh):
    """mmt_attn_last_route() of a key-bias forward and backward as the environment stands: the
    resident forward (one-pass unless MMT_ATTN_ONEPASS=0) and, whatever MMT_ATTN_BWD8 says, the
    two-phase resident backward (the concurrent-phase kernel has no key-bias form); else the tiled
    forward (one wave at L <= 32; NQ = 2 up to L = 256 and past 320, Dh 64) and tiled backward."""
    import os
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    ntile = 2 * ((L + 63) // 64)
    if K.attn_fwd_resident(L, Dh):
        one = os.environ.get("MMT_ATTN_ONEPASS", "1") != "0"
        fwd = _C.attn_route(_C.ATTN_ROUTE_FWD_RES_ONEPASS if one else _C.ATTN_ROUTE_FWD_RES_TWOPASS, ntile)
    elif Dh == 64 and L <= 32:
        fwd = _C.attn_route(_C.ATTN_ROUTE_FWD_TILED_1W, 1, 64)
    else:
        nq = 2 if Dh == 64 and (L <= 256 or L > 320) else 1
        fwd = _C.attn_route(_C.ATTN_ROUTE_FWD_TILED_4W, nq, Dh)
    if K.attn_bwd_resident(L, Dh):
        bwd = _C.attn_route(_C.ATTN_ROUTE_BWD_RES, ntile)
    else:
        f64, f128 = L / (-(-L // 64) * 64), L / (-(-L // 128) * 128)
        bwd = _C.attn_route(_C.ATTN_ROUTE_BWD_TILED, 2 if f64 > f128 + 0.10 else 4, Dh)
    return fwd, bwd


def run_case(dev, L, H, Dh, mode, drop, kind="sizes", B=2):
    """One forward + backward with a key bias. Returns (o, lse, dqkv, bgrad - 0.5) of the kernels
    and (o, lse, dqkv) of the torch reference. Asserts the route of both launches
    (expected_routes)."""
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    want_fwd, want_bwd = expected_routes(L, Dh)
    g = torch.Generator().manual_seed(L * 7 + H + Dh)
    qkv = torch.randn((B, L, 3 * H * Dh), generator=g).bfloat16().to(dev)
    dout = torch.randn((B, L, H * Dh), generator=g).bfloat16().to(dev)
    scale = Dh ** -0.5
    table, mask, rng_set = make_table(K, mode, L, dev)
    kb = make_bias(K, B, L, rng_set, dev, g, kind)
    kp = 0.9 if drop else 1.0
    rng = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    bits = K.dropout_bits(rng, 1, 2, L, L, kp) if drop else None
    keep = bits_to_keep(bits, L).to(dev) if drop else None
    o, lse = K.attn_fwd(qkv, H, scale, table, bits, kp, key_bias=kb)
    assert _C.attn_last_route() == want_fwd, hex(_C.attn_last_route())
    bg = torch.full((3 * H * Dh,), 0.5, device=dev)
    dq = K.attn_bwd(qkv, o, dout, lse, H, scale, table, bits, kp, bias_grad=bg, key_bias=kb)
    assert _C.attn_last_route() == want_bwd, hex(_C.attn_last_route())
    torch.cuda.synchronize()
    K.device_status()
    qf = qkv.float().requires_grad_()
    ro, rl = ref_attention(qf, H, scale, mask, keep, kp, kb)
    ro.backward(dout.float())
    return (o.float(), lse, dq.float(), bg - 0.5), (ro.detach(), rl.detach(), qf.grad)


def check_vs_torch(got, ref, B, L):
    (o, lse, dq, bg), (ro, rl, rdq) = got, ref
    assert torch.isfinite(o).all() and torch.isfinite(dq).all() and torch.isfinite(bg).all()
    eo = rel(o, ro)
    eg = [rel(dq.view(B, L, 3, -1)[:, :, i], rdq.view(B, L, 3, -1)[:, :, i]) for i in range(3)]
    el = (lse - rl).abs().max().item()
    print(f"L={L}: rel o {eo:.3e}  dq {eg[0]:.3e}  dk {eg[1]:.3e}  dv {eg[2]:.3e}  |dlse| {el:.2e}")
    assert eo < 1e-2, eo
    for i in range(3):
        assert eg[i] < 2e-2, ("qkv"[i], eg[i])
    assert el < 1e-3, el  # lse includes the bias
    # fused QKV bias gradient = column sums of dqkv (summed before the bf16 rounding of dqkv)
    cs = dq.sum((0, 1))
    torch.testing.assert_close(bg, cs, rtol=2e-2, atol=2e-2 * float(cs.abs().max()) + 1e-3)


@pytest.mark.parametrize("L,H,mode,drop,env", [
    (33, 3, "none", True, {}), (65, 3, "octo", True, {}), (101, 3, "causal", True, {}),
    (292, 6, "octo", False, {}), (320, 3, "octo", True, {}),
    (65, 3, "octo", True, {"MMT_ATTN_ONEPASS": "0"}),
    (292, 6, "octo", False, {"MMT_ATTN_BWD8": "0"})])
def test_resident_path_vs_torch(dev, L, H, mode, drop, env, monkeypatch):
    """Resident forward (one-pass and exact-max forms) and the two-phase resident backward, which
    a key bias takes under either setting of MMT_ATTN_BWD8 (routes asserted in run_case)."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert K.attn_fwd_resident(L, 64) and K.attn_bwd_resident(L, 64)
    got, ref = run_case(dev, L, H, 64, mode, drop)
    check_vs_torch(got, ref, 2, L)


@pytest.mark.parametrize("L,H,Dh,mode,drop", [
    (20, 3, 64, "none", True),      # the one-wave form
    (330, 3, 64, "octo", True),     # just past the resident limit, L % 4 != 0
    (200, 2, 128, "octo", True),
    (70, 2, 256, "octo", False)])
def test_tiled_path_vs_torch(dev, L, H, Dh, mode, drop):
    """The tiled kernels (routes asserted in run_case): one wave at L = 20, four waves with
    NQ = 2 at L = 330 and NQ = 1 at Dh 128 / 256."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    assert not K.attn_fwd_resident(L, Dh) and not K.attn_bwd_resident(L, Dh)
    got, ref = run_case(dev, L, H, Dh, mode, drop)
    check_vs_torch(got, ref, 2, L)


def test_tiled_vs_resident_at_292(dev, monkeypatch):
    """L = 292 through the tiled kernels (MMT_ATTN_RES = MMT_ATTN_RES_BWD = 0) against torch, and
    against the resident kernels at the existing resident-vs-tiled bar."""
    B, L, H = 2, 292, 3
    res = run_case(dev, L, H, 64, "octo", True)
    monkeypatch.setenv("MMT_ATTN_RES", "0")
    monkeypatch.setenv("MMT_ATTN_RES_BWD", "0")
    til = run_case(dev, L, H, 64, "octo", True)
    check_vs_torch(*til, B, L)
    (o1, l1, d1, b1), (o0, l0, d0, b0) = res[0], til[0]
    assert rel(o1, o0) < 1e-2 and (l1 - l0).abs().max().item() < 1e-3
    for i in range(3):
        a, b = d1.view(B, L, 3, -1)[:, :, i], d0.view(B, L, 3, -1)[:, :, i]
        assert rel(a, b) < 2e-2, ("qkv"[i], rel(a, b))


@pytest.mark.parametrize("L,mode", [(101, "causal"), (330, "octo")])
def test_generic_bias(dev, L, mode):
    """A bias on every key, uniform in [-4, 4] (not only log-sizes of one set)."""
    got, ref = run_case(dev, L, 3, 64, mode, True, kind="generic")
    check_vs_torch(got, ref, 2, L)


@pytest.mark.parametrize("L", [101, 330])
def test_shift_invariance(dev, L):
    """Adding a constant to every key's bias leaves the output unchanged and moves every finite
    lse by the constant (needs no reference)."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    B, H, Dh = 2, 3, 64
    g = torch.Generator().manual_seed(L)
    qkv = torch.randn((B, L, 3 * H * Dh), generator=g).bfloat16().to(dev)
    table, _, rng_set = make_table(K, "octo", L, dev)
    kb = make_bias(K, B, L, rng_set, dev, g)
    kb2 = kb.clone()
    kb2[:, :L] += 2.5
    o, lse = K.attn_fwd(qkv, H, Dh ** -0.5, table, key_bias=kb)
    o2, lse2 = K.attn_fwd(qkv, H, Dh ** -0.5, table, key_bias=kb2)
    torch.cuda.synchronize()
    assert rel(o2, o) < 1e-2
    fin = torch.isfinite(lse)
    assert fin.any() and torch.equal(fin, torch.isfinite(lse2))
    assert (lse2[fin] - lse[fin] - 2.5).abs().max().item() < 1e-3


def test_duplication_identity(dev):
    """Proportional attention is attention over the unmerged copies: a bias of log 2 on keys
    0..31 equals repeating those keys' k and v rows (the kernel against itself without a bias)."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    B, H, Dh, L, n = 2, 3, 64, 96, 32
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn((B, L, 3, H * Dh), generator=g).bfloat16()
    big = torch.cat([qkv, qkv[:, :n]], dim=1)                       # rows 96..127 repeat rows 0..31
    kb = torch.zeros((B, K.attn_lp(L)))
    kb[:, :n] = math.log(2.0)
    kb[:, L:] = PAD
    assert K.attn_fwd_resident(L, Dh) and K.attn_fwd_resident(L + n, Dh)
    o, _ = K.attn_fwd(qkv.view(B, L, -1).to(dev), H, Dh ** -0.5, key_bias=kb.to(dev))
    o2, _ = K.attn_fwd(big.view(B, L + n, -1).contiguous().to(dev), H, Dh ** -0.5)
    torch.cuda.synchronize()
    assert rel(o, o2[:, :L]) < 1e-2, rel(o, o2[:, :L])


@pytest.mark.parametrize("L", [292, 330])
def test_rerun_bit_identical(dev, L):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    B, H, Dh = 2, 3, 64
    g = torch.Generator().manual_seed(L + 1)
    qkv = torch.randn((B, L, 3 * H * Dh), generator=g).bfloat16().to(dev)
    dout = torch.randn((B, L, H * Dh), generator=g).bfloat16().to(dev)
    table, _, rng_set = make_table(K, "octo", L, dev)
    kb = make_bias(K, B, L, rng_set, dev, g)
    rng = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    bits = K.dropout_bits(rng, 1, 2, L, L, 0.9)
    runs = []
    for _ in range(2):
        o, lse = K.attn_fwd(qkv, H, Dh ** -0.5, table, bits, 0.9, key_bias=kb)
        dq = K.attn_bwd(qkv, o, dout, lse, H, Dh ** -0.5, table, bits, 0.9, key_bias=kb)
        torch.cuda.synchronize()
        runs.append((o, lse, dq))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_argument_checks(dev):
    """key_bias with wsum, with the T5 bias, or with a short / misaligned row stride: MMTError and
    nothing launched (the outputs keep their sentinel)."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd._C import MMTError
    B, L, H, Dh = 2, 100, 2, 64
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn((B, L, 3 * H * Dh), generator=g).bfloat16().to(dev)
    kb = torch.zeros((B, K.attn_lp(L)), device=dev)
    out = torch.full((B, L, H * Dh), 7.0, dtype=torch.bfloat16, device=dev)
    wsum = torch.zeros((B, H, L), device=dev)
    t5 = torch.zeros((H, L, L), device=dev)
    short = torch.zeros((B, L), device=dev)                         # stride 100 < roundup(L, 64)
    odd = torch.zeros((B, K.attn_lp(L) + 2), device=dev)            # stride 130: not a multiple of 4
    bad = [dict(key_bias=kb, wsum=wsum), dict(key_bias=kb, bias=t5), dict(key_bias=short),
           dict(key_bias=odd)]
    for kw in bad:
        with pytest.raises(MMTError):
            K.attn_fwd(qkv, H, Dh ** -0.5, out=out, **kw)
    o, lse = K.attn_fwd(qkv, H, Dh ** -0.5)
    dq = torch.full_like(qkv, 7.0)
    dout = torch.ones_like(o)
    for kbad in (short, odd):
        with pytest.raises(MMTError):
            K.attn_bwd(qkv, o, dout, lse, H, Dh ** -0.5, dqkv=dq, key_bias=kbad)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (dq == 7.0).all()
    with pytest.raises(ValueError):                                 # the wrapper's own checks
        K.attn_fwd(qkv, H, Dh ** -0.5, key_bias=kb.double())
    with pytest.raises(ValueError):
        K.attn_fwd(qkv, H, Dh ** -0.5, key_bias=kb[:1])


def test_tome_size_bias(dev):
    """log(size) on each merged set's range, exact 0 elsewhere and on the padding."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    B, L = 3, 50
    g = torch.Generator().manual_seed(8)

    def sizes(t):
        s = torch.randint(1, 9, (B, t), generator=g).float()
        s[:, ::3] = 1.0
        return s

    def check(sets):
        kb = K.tome_size_bias(B, L, [(s0, t, sz.to(dev)) for s0, t, sz in sets])
        torch.cuda.synchronize()
        assert kb.shape == (B, K.attn_lp(L)) and kb.dtype == torch.float32
        want = torch.zeros((B, K.attn_lp(L)))
        ones = torch.zeros((B, K.attn_lp(L)), dtype=torch.bool)
        for s0, t, sz in sets:
            want[:, s0:s0 + t] = torch.log(sz)
            ones[:, s0:s0 + t] = sz == 1.0
        got = kb.cpu()
        inside = want != 0
        assert torch.equal(got[~inside], want[~inside])             # exact zeros, size == 1 included
        assert (got[ones] == 0).all()
        torch.testing.assert_close(got[inside], want[inside], rtol=1e-6, atol=0)

    check([(5, 36, sizes(36))])                                     # one set: [5, 41)
    check([(2, 20, sizes(20)), (30, 17, sizes(17))])                # two sets
