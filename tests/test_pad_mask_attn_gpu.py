"""GPU: attention with the pad-mask key bias (K.pad_mask_bias -> mmt_attn_fwd_keybias /
mmt_attn_bwd_keybias), one case per kernel family, with and without attention dropout, against
the float64 restatement tests/pad_mask_ref.py masked_attention.

B = 3, H = 2, randn bf16 qkv, three sets (text | image | readout; text sees itself, image sees
text and image, readout sees all). Sample 0 has set 0 absent — at L = 100 and 330 the leading
32-key tiles are wholly masked: the running-max start and the alpha = 0 rescale of the one-pass
forward — sample 1 has set 1 absent, sample 2 nothing.

Asserted:
 (a) the k and v thirds of dqkv of every masked key row of its sample are exactly 0. This holds
     for the gradient that arrives from queries with a present key in sight: P of a masked key
     underflows to 0.0 there. The queries of sample 0's absent set 0 see that set alone, so their
     softmax over it is the ordinary one (shift invariance, include/mmt_api.h) and dk, dv of those
     rows get their ordinary, non-zero contribution from them. (a) is therefore taken from a second
     backward whose dout is zero on exactly those all-masked query rows — the rows no present
     token reads; everything else about it is the same call.
 (b) every output and lse is finite;
 (c) relative L2 of o, dq, dk, dv against the restatement: e1 <= 1.5 e0 + 1e-4, e0 the same
     quantity with an all-zero key_bias against the unmasked restatement (full random dout);
 (d) the mask does something: sample 0's output differs from the unmasked run by more than 10 e0.
"""
import numpy as np
import pytest
import torch

from tests import pad_mask_ref as R
from tests.test_prop_attn_gpu import bits_to_keep, expected_routes

pytestmark = pytest.mark.gpu

B, H = 3, 2
VIS = [0b001, 0b011, 0b111]
SET_MASK = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 1]], bool)
#        L   Dh  lens
CASES = [(20, 64, [8, 8, 4]),        # one-wave tiled
         (100, 64, [70, 26, 4]),     # resident forward, two-phase resident backward
         (100, 128, [70, 26, 4]),    # tiled, Dh 128
         (330, 64, [200, 126, 4])]   # tiled, past the resident limit


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def thirds(dqkv):
    return dqkv.view(dqkv.shape[0], dqkv.shape[1], 3, -1).unbind(2)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("L,Dh,lens", CASES, ids=[f"L{c[0]}-Dh{c[1]}" for c in CASES])
def test_attention_with_the_mask_bias(dev, L, Dh, lens, drop):
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    starts = [0, lens[0], lens[0] + lens[1]]
    assert sum(lens) == L
    table = K.SetTable(starts, lens, VIS)
    mask = R.dense_mask(starts, lens, VIS)
    masked = R.masked_rows(starts, lens, B, SET_MASK)
    g = torch.Generator().manual_seed(L + Dh)
    qkv = torch.randn((B, L, 3 * H * Dh), generator=g).bfloat16()
    dout = torch.randn((B, L, H * Dh), generator=g).bfloat16()
    # the queries whose visible keys are all masked: sample 0's set 0 (it sees itself alone)
    all_masked_q = torch.from_numpy(~(mask.numpy()[None] & ~masked[:, None, :]).any(-1))
    assert all_masked_q[0, :lens[0]].all() and int(all_masked_q.sum()) == lens[0]
    dout_a = dout.clone()
    dout_a[all_masked_q] = 0
    scale = Dh ** -0.5
    kp = 0.9 if drop else 1.0
    rng = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    bits = K.dropout_bits(rng, 1, 2, L, L, kp) if drop else None
    keep = bits_to_keep(bits, L) if drop else None
    words = K.pad_mask_pack(torch.from_numpy(SET_MASK).to(dev), 0b100)
    kb1 = K.pad_mask_bias(B, L, table, words)
    kb0 = torch.zeros_like(kb1)
    want_fwd, want_bwd = expected_routes(L, Dh)
    if (L, Dh) == (100, 64):
        assert want_fwd & 0xff in (_C.ATTN_ROUTE_FWD_RES_ONEPASS, _C.ATTN_ROUTE_FWD_RES_TWOPASS)
        assert want_bwd & 0xff == _C.ATTN_ROUTE_BWD_RES
    qd, dd = qkv.to(dev), dout.to(dev)
    got = {}
    for name, kb in (("zero", kb0), ("mask", kb1)):
        o, lse = K.attn_fwd(qd, H, scale, table, bits, kp, key_bias=kb)
        assert _C.attn_last_route() == want_fwd, hex(_C.attn_last_route())
        dq = K.attn_bwd(qd, o, dd, lse, H, scale, table, bits, kp, key_bias=kb)
        assert _C.attn_last_route() == want_bwd, hex(_C.attn_last_route())
        got[name] = (o, lse, dq)
    o1, lse1, _ = got["mask"]
    dq_a = K.attn_bwd(qd, o1, dout_a.to(dev), lse1, H, scale, table, bits, kp, key_bias=kb1)
    torch.cuda.synchronize()
    K.device_status()
    # (a)
    _, dk_a, dv_a = thirds(dq_a.cpu())
    mk = torch.from_numpy(masked)
    assert mk.any() and (dk_a[mk] == 0).all() and (dv_a[mk] == 0).all()
    assert (dk_a[~mk] != 0).any() and (dv_a[~mk] != 0).any()
    # the unmodified backward (full dout): exact zeros on the masked key rows of every sample
    # that has no all-masked query (sample 1's set 1); sample 0's set 0 gets its own queries'
    _, dk_f, dv_f = thirds(got["mask"][2].cpu())
    no_amq = ~all_masked_q.any(1)
    assert no_amq.tolist() == [False, True, True]
    mk_f = mk & no_amq[:, None]
    assert mk_f.any() and (dk_f[mk_f] == 0).all() and (dv_f[mk_f] == 0).all()
    assert (dk_f[0, :lens[0]] != 0).any() and (dv_f[0, :lens[0]] != 0).any()
    # (b)
    for o, lse, dq in got.values():
        assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(dq).all()
    assert torch.isfinite(dq_a).all()
    # (c) against the float64 restatement
    errs, ref_o = {}, {}
    for name, kb in (("zero", None), ("mask", kb1.cpu().double())):
        q64 = qkv.double().requires_grad_()
        ro, _ = R.masked_attention(q64, H, scale, mask, kb, keep, kp)
        ro.backward(dout.double())
        ref_o[name] = ro.detach()
        o, _, dq = got[name]
        pairs = zip(("o", "dq", "dk", "dv"), (o.cpu(), *thirds(dq.cpu())),
                    (ro.detach(), *thirds(q64.grad)))
        errs[name] = {k: rel(a, b) for k, a, b in pairs}
    print(f"\nL={L} Dh={Dh} drop={drop}")
    bad = []
    for k in ("o", "dq", "dk", "dv"):
        e0, e1 = errs["zero"][k], errs["mask"][k]
        print(f"  {k:3s} e0 {e0:.3e}  e1 {e1:.3e}  e1 / (1.5 e0 + 1e-4) = {e1 / (1.5 * e0 + 1e-4):.3f}")
        if not e1 <= 1.5 * e0 + 1e-4:
            bad.append((k, e0, e1))
    # (d)
    diff = rel(got["mask"][0][0], got["zero"][0][0])
    print(f"  sample 0, masked vs unmasked output: rel {diff:.3e}")
    assert not bad, bad
    assert diff > 10 * errs["zero"]["o"], (diff, errs["zero"]["o"])
    # the all-masked queries get the ordinary softmax over their keys: on those rows the masked
    # run is as close to the UNMASKED restatement as the unmasked run is (the same bar)
    am = all_masked_q
    e0 = rel(got["zero"][0].cpu()[am], ref_o["zero"][am])
    e1 = rel(got["mask"][0].cpu()[am], ref_o["zero"][am])
    print(f"  all-masked query rows vs the unmasked restatement: e0 {e0:.3e}  e1 {e1:.3e}")
    assert e1 <= 1.5 * e0 + 1e-4, (e0, e1)
