"""GPU: QK-norm through one Encoder1DBlock (self_attention.normalize_qk), laid out as
tests/test_prop_attn_block_gpu.py: D 128, 2 heads (Dh 64), MLP 256; text 8 | image 40 | readout 4,
ToMe r = 4 on the image set with incoming sizes 1..6, train=False, against a float64 torch
restatement built from oracle.octo_ref's helpers plus tests/qknorm_ref.py and differentiated with
autograd. The block's two discrete choices come from its own saved state (the ToMe match indices
and the relu gate), since no tolerance compares them.

* The bar is measured against the block's own path without the flag: e0 = relative L2 of every
  quantity (output, input gradient, each parameter gradient) with the flag off against the
  restatement without the norm; with the flag on every quantity present in both must satisfy
  e1 <= 1.5 e0 + 1e-4, and the two scale gradients, which have no e0,
  e1 <= 1.5 max(e0 over the parameter gradients) + 1e-4. The table is printed.
* The flag does something: the outputs differ by more than 10 e0.
* ToMe reads the normalised keys: the saved match equals K.tome_match on the K slice of the saved
  (normalised) qkv and differs from the match on the pre-norm keys.
* The QKV bias gradient's q and k parts are the column sums of dqkv AFTER qk_norm_bwd, not of the
  attention backward's output.
"""
import pytest
import torch

from oracle.octo_ref import dense, seq_layernorm, tome_merge_wavg
from tests import qknorm_ref as R

pytestmark = pytest.mark.gpu

D, H, MLP, B = 128, 2, 256, 2
DH = D // H
STARTS, LENS, VIS = [0, 8, 48], [8, 40, 4], [0b001, 0b011, 0b111]
IMG, RM = 1, 4  # the merged set and its r
BLK = "S/Block_0"
QLN, KLN = f"{BLK}/SelfAttention_0/query_ln/scale", f"{BLK}/SelfAttention_0/key_ln/scale"


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def attention(qkv, scale, mask):
    Bq, L, _ = qkv.shape
    q, k, v = qkv.view(Bq, L, 3, H, DH).unbind(2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    s = torch.where(mask[None, None], s, torch.finfo(s.dtype).min)
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(Bq, L, D)


def block_ref(x, p, size, tome, qkn, gate):
    """The block in float64 (train=False: no dropout), Encoder1DBlock.forward's order: LN0, QKV,
    (QK-norm), attention, out-projection + residual, ToMe merge_wavg of the image set with the
    incoming sizes, LN1, MLP + residual. gate (B, L - r, MLP) bool: the relu's active units."""
    sid = torch.repeat_interleave(torch.arange(3), torch.tensor(LENS))
    mask = ((torch.tensor(VIS)[sid][:, None] >> sid[None, :]) & 1).bool()
    y0 = seq_layernorm(x, p[f"{BLK}/LayerNorm_0/scale"], p[f"{BLK}/LayerNorm_0/bias"], 1e-6)
    qkv = dense(p, f"{BLK}/SelfAttention_0/qkv", y0)
    if qkn:
        qkv = R.qk_norm(qkv, H, p[QLN], p[KLN], 1e-6)
    o = attention(qkv, DH ** -0.5, mask)
    x1 = x + dense(p, f"{BLK}/SelfAttention_0/out", o)
    s0, t = STARTS[IMG], LENS[IMG]
    unm, src, dst = tome
    xs, _ = tome_merge_wavg(x1[:, s0:s0 + t], size.unsqueeze(-1), unm, src, dst, RM)
    x1 = torch.cat([x1[:, :s0], xs, x1[:, s0 + t:]], dim=1)
    y1 = seq_layernorm(x1, p[f"{BLK}/LayerNorm_1/scale"], p[f"{BLK}/LayerNorm_1/bias"], 1e-6)
    z = dense(p, f"{BLK}/MLPBlock_0/Dense_0", y1)
    return x1 + dense(p, f"{BLK}/MLPBlock_0/Dense_1", z * gate)


SEED = 17


def run_block(dev, seed=SEED):
    """The block with the flag off and on and the restatement of each: {flag: (got, ref, extra)},
    got / ref = {quantity: tensor} (out, dx and every parameter gradient)."""
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import (
        LayerCtx, StackedEncoder1DBlock)
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_sequencer import LayerSets
    g = torch.Generator().manual_seed(seed)
    L = sum(LENS)
    x = torch.randn((B, L, D), generator=g)
    dy = torch.randn((B, L - RM, D), generator=g)
    size = torch.randint(1, 7, (B, LENS[IMG]), generator=g).float()
    scales = torch.rand((2, DH), generator=g) + 0.5
    runs = {}
    for qkn in (False, True):
        store = ParamStore()
        stack = StackedEncoder1DBlock.create(store, "S", 1, D, H, MLP, normalize_qk=qkn)
        store.materialize(dev, 5)       # the scales draw nothing: the other parameters are equal
        blk = stack.blocks[0]
        if qkn:
            blk.q_ln.data.copy_(scales[0])
            blk.k_ln.data.copy_(scales[1])
        ctx = LayerCtx(layer=0, sets=LayerSets(STARTS, LENS, VIS), table=K.SetTable(STARTS, LENS, VIS),
                       tome_set=IMG, r=RM, train=False)
        store.zero_grad()
        seen = {}
        real = K.qk_norm_bwd

        def spy(dqkv, *a, **kw):
            seen["dqkv_attn"] = dqkv.clone()
            out = real(dqkv, *a, **kw)
            seen["dqkv_pre"] = dqkv.clone()
            return out
        K.qk_norm_bwd = spy
        try:
            out, sv, _ = blk.forward(x.to(dev), ctx, size.to(dev))
            dx, _ = blk.backward(dy.to(dev), sv, ctx)
            torch.cuda.synchronize()
        finally:
            K.qk_norm_bwd = real
        K.device_status()
        assert (sv["qk_pre"] is not None) == qkn and bool(seen) == qkn
        got = {"out": out.cpu(), "dx": dx.cpu(), **{p.name: p.grad.cpu().clone() for p in store.params}}
        tome = tuple(a.cpu() for a in sv["tome"][6:9])      # the block's own match indices
        p64 = {p.name: (p.bf16 if p.name.endswith("kernel") else p.data).detach().double().cpu()
               .clone().requires_grad_() for p in store.params}
        x64 = x.double().requires_grad_()
        gate = (sv["h"].view(B, L - RM, MLP) > 0).cpu()
        ref_out = block_ref(x64, p64, size.double(), tome, qkn, gate)
        ref_out.backward(dy.double())
        ref = {"out": ref_out.detach(), "dx": x64.grad, **{n: v.grad for n, v in p64.items()}}
        extra = dict(sv=sv, seen=seen, tome=tuple(sv["tome"][6:9]), L=L)
        runs[qkn] = (got, ref, extra)
    return runs


@pytest.fixture(scope="module")
def block_runs(dev):
    return run_block(dev)


def test_block_matches_restatement_at_the_flag_off_floor(block_runs):
    (g0, r0, _), (g1, r1, _) = block_runs[False], block_runs[True]
    assert set(g0) == set(r0) and len(g0) == 14           # out, dx, 12 parameters
    assert set(g1) == set(r1) == set(g0) | {QLN, KLN}
    print(f"\n{'quantity':46s} {'e0 (flag off)':>14s} {'e1 (flag on)':>14s}")
    bad, e0_params = [], []
    for name in g0:
        e0, e1 = rel(g0[name], r0[name]), rel(g1[name], r1[name])
        if name not in ("out", "dx"):
            e0_params.append(e0)
        print(f"{name:46s} {e0:14.3e} {e1:14.3e}")
        if not e1 <= 1.5 * e0 + 1e-4:
            bad.append((name, e0, e1))
    for name in (QLN, KLN):
        e1 = rel(g1[name], r1[name])
        print(f"{name:46s} {'max ' + format(max(e0_params), '.3e'):>14s} {e1:14.3e}")
        if not e1 <= 1.5 * max(e0_params) + 1e-4:
            bad.append((name, max(e0_params), e1))
        assert g1[name].abs().max() > 0
    assert not bad, bad


def test_flag_changes_the_block_output(block_runs):
    (g0, r0, _), (g1, _, _) = block_runs[False], block_runs[True]
    e0 = rel(g0["out"], r0["out"])
    diff = rel(g1["out"], g0["out"])
    print(f"\nflag on vs off: rel {diff:.3e}; floor e0 {e0:.3e}")
    assert diff > 10 * e0, (diff, e0)


def test_tome_matches_on_the_normalised_keys(block_runs):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    _, _, ex = block_runs[True]
    sv, L = ex["sv"], ex["L"]
    s0, t = STARTS[IMG], LENS[IMG]
    k_norm = sv["qkv"].view(B, L, 3, H, DH)[:, s0:s0 + t, 1]
    k_pre = sv["qk_pre"].view(B, L, 2, H, DH)[:, s0:s0 + t, 1]
    assert not torch.equal(k_norm, k_pre)
    on_norm = K.tome_match(k_norm, RM)
    on_pre = K.tome_match(k_pre, RM)
    torch.cuda.synchronize()
    for a, b in zip(ex["tome"], on_norm):
        assert torch.equal(a, b)
    # SEED is chosen so that the two matches differ: the check above cannot pass vacuously
    assert any(not torch.equal(a, b) for a, b in zip(on_norm, on_pre))


def test_qkv_bias_gradient_is_the_pre_norm_column_sum(block_runs):
    (g0, r0, _), (g1, r1, ex) = block_runs[False], block_runs[True]
    name = f"{BLK}/SelfAttention_0/qkv/bias"
    floor = max(rel(g0[n], r0[n]) for n in g0 if n not in ("out", "dx"))
    allowed = 1.5 * floor + 1e-4
    bias = g1[name][:2 * D]
    pre = ex["seen"]["dqkv_pre"].double().view(-1, 3 * D).sum(0)[:2 * D]
    attn = ex["seen"]["dqkv_attn"].double().view(-1, 3 * D).sum(0)[:2 * D]
    e_pre, e_attn = rel(bias, pre), rel(bias, attn)
    print(f"\nqkv bias (q, k) vs colsum after qk_norm_bwd {e_pre:.3e}, vs the attention "
          f"backward's {e_attn:.3e}; allowed {allowed:.3e}")
    assert e_pre <= allowed
    assert e_attn > 10 * allowed
    # the V third of dqkv is not touched by qk_norm_bwd
    assert torch.equal(ex["seen"]["dqkv_pre"].view(-1, 3 * D)[:, 2 * D:],
                       ex["seen"]["dqkv_attn"].view(-1, 3 * D)[:, 2 * D:])
