"""GPU: MultiHeadAttentionPooling as a module and inside the OCTO diffusion step
(OctoConfig.readout_pooling = "attention") against the torch restatement of the reference module
(tests/attn_pool_ref.py, float64, the module's own weights as the GEMMs read them).

Bars (SURVEY §8c, bf16 path): the output within 2e-2 relative L2; every parameter gradient and dx
at cosine >= 0.999 with the norm within 5e-2.

The output is held to its bar against the plain float64 restatement. The gradients are held to
theirs against the restatement with its activations rounded to bf16 at the storage points of a
bf16 compute policy (attn_pool_ref.bf16_storage, straight-through; the practice of
oracle/octo_ref.py): the MLP's relu gates a unit by the sign of a pre-activation that carries one
bf16 rounding of its input, so in plain float64 a few of the B x hidden units (5 x 192) gate the
other way, and that alone, with no kernel involved, moves the gradients by about 3e-2 relative:
the restatement against itself, float64 vs bf16 storage on the CPU, gives per-parameter cosines
of 0.9977 .. 0.99999 over 8 seeds at these shapes. Measured on the MI355X against plain float64:
the worst parameter of a case lies between 0.9985 (MLPBlock_0/Dense_0/kernel at D = 384;
0.99876 for LayerNorm_0/scale at D = 192 in another run) and 0.99999, depending on whether a
unit flips in that case; against the bf16 storage points every gradient is at 0.99999 or better.
Each test prints both sets of figures."""
import pytest
import torch

from attn_pool_ref import MHA, attention_pool, bf16_storage, grads_as_module, module_params
from oracle.parity import _inputs

pytestmark = pytest.mark.gpu

EPS = 1e-6


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()))


def _close_grad(got, want, what):
    got, want = got.double().cpu(), want.double().cpu()
    if float(want.norm()) == 0.0:
        assert float(got.norm()) == 0.0, what
        return
    c, ratio = _cos(got, want), float(got.norm() / want.norm())
    print(f"{what}: cosine {c:.6f}, norm ratio {ratio:.4f}")
    assert c >= 0.999, (what, c)
    assert abs(ratio - 1.0) <= 5e-2, (what, ratio)


def _module(dev, D, H, axes, seed):
    from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import (
        MultiHeadAttentionPooling)
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    store = ParamStore()
    m = MultiHeadAttentionPooling.create(store, "pool", D, H, reduction_axes=axes)
    store.materialize(dev, seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():   # LayerNorm scale / bias and the attention biases away from 1 / 0
        m.ln.scale.data.add_((0.1 * torch.randn(D, generator=g)).to(dev))
        m.ln.bias.data.add_((0.1 * torch.randn(D, generator=g)).to(dev))
        for b in (m.query.b, m.kv.b, m.out.b):
            b.data.add_((0.1 * torch.randn(b.shape, generator=g)).to(dev))
        if axes == (1,):
            # Every sample's LayerNorm output is the bias here, so every sample has the same MLP
            # pre-activations bias . W0 + b0. The sequence-axis kernel forms y as x * mul + (bias -
            # mean * mul) with mul = 1e3 gamma: y = bias + O(2^-24 * 1e3 |a|), which moves about
            # one y element in seven to the neighbouring bf16 value, per sample. A hidden unit
            # whose pre-activation lies within that noise (~3e-4) of zero would be gated per sample
            # by the noise, and a single unit of the 5 x 192 is 3e-2 of a gradient. The Dense_0 bias
            # is therefore moved so that no unit sits within 0.05 of zero: the comparison measures
            # the kernels, not the sign of a rounding error.
            w0 = m.mlp.dense.w.data.to(torch.bfloat16).double()
            pre = m.ln.bias.data.to(torch.bfloat16).double() @ w0.t() + m.mlp.dense.b.data.double()
            m.mlp.dense.b.data.add_((0.05 * torch.sign(pre)).float())
    store.sync_shadow()
    return m, store


@pytest.mark.parametrize("axes", [(-1,), (1,)], ids=["feature-norm", "sequence-norm"])
@pytest.mark.parametrize("D,H,n,B", [(192, 3, 4, 5), (384, 6, 8, 3)], ids=["D192", "D384"])
def test_module_parity(dev, D, H, n, B, axes):
    m, store = _module(dev, D, H, axes, seed=D + len(axes))
    g = torch.Generator().manual_seed(B)
    L = n + 3
    rows = list(range(1, 1 + n // 2)) + list(range(L - (n - n // 2), L))   # two runs of rows
    x = torch.randn((B, L, D), generator=g).to(dev)
    de = torch.randn((B, D), generator=g).to(torch.bfloat16).to(dev)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    flag = torch.full((L,), -1, dtype=torch.int32)
    flag[rows] = torch.arange(n, dtype=torch.int32)
    # the destination and the upstream gradient as column ranges of wider buffers (the head's cat)
    cat = torch.zeros((B, D + 24), dtype=torch.bfloat16, device=dev)
    dcat = torch.zeros((B, D + 24), dtype=torch.bfloat16, device=dev)
    dcat[:, 16:16 + D] = de
    store.zero_grad()
    out, sv = m.forward(x, rows_d, out=cat[:, 8:8 + D])
    dx = m.backward(dcat[:, 16:16 + D], sv, flag.to(dev))
    torch.cuda.synchronize()
    assert not cat[:, :8].any() and not cat[:, 8 + D:].any()
    # the restatement on the bf16 readout rows the GEMMs read
    P64 = module_params(m)
    xr = x[:, rows].to(torch.bfloat16).double()
    ref64, _ = attention_pool(xr, P64, EPS, axes)
    (ref64[:, 0] * de.double()).sum().backward()
    rel = float((out.double() - ref64[:, 0].detach()).norm() / ref64.detach().norm())
    print(f"output relative L2 error vs plain float64 {rel:.3e}")
    assert rel <= 2e-2
    plain = grads_as_module(P64, m)
    worst = min((_cos(p.grad, plain[p.name]), p.name) for p in store.params
                if float(plain[p.name].norm()) > 0)
    print(f"vs plain float64: worst parameter-gradient cosine {worst[0]:.6f} ({worst[1]})")
    # ... and with the bf16 storage points
    P = module_params(m)
    xr = xr.clone().requires_grad_(True)
    ref, aux = attention_pool(xr, P, EPS, axes, storage=bf16_storage)
    (ref[:, 0] * de.double()).sum().backward()
    rel = float((out.double() - ref[:, 0].detach()).norm() / ref.detach().norm())
    print(f"output relative L2 error vs bf16 storage {rel:.3e}")
    assert rel <= 2e-2
    want = grads_as_module(P, m)
    for p in store.params:
        _close_grad(p.grad, want[p.name], p.name)
    dx_ref = torch.zeros((B, L, D), dtype=torch.float64, device=dev)
    dx_ref[:, rows] = xr.grad
    _close_grad(dx, dx_ref, "dx")
    keep = torch.ones(L, dtype=torch.bool)
    keep[rows] = False
    assert not dx[:, keep].any()                       # exactly 0 outside the pooled rows
    if axes == (1,):
        # the norm over the length-1 pooled sequence outputs its bias: fp32 x * mul + (bias - mean
        # * mul) with mul = gamma / sqrt(eps) = 1e3 gamma leaves two roundings of |a| * mul, then
        # one bf16 rounding of the result; so out = a + MLP(bias), and nothing but the residual
        # reaches a (the reference's y == bias exactly)
        a = sv["a"].float()
        mul = 1e3 * float(m.ln.scale.data.abs().max())
        bias = m.ln.bias.data
        tol = 2 * 2.0 ** -23 * float(a.abs().max()) * mul + 2.0 ** -8 * float(bias.abs().max())
        assert float((sv["y"].float() - bias).abs().max()) <= tol
        torch.testing.assert_close(aux["y"][:, 0], bf16_storage(P["LayerNorm_0/bias"]).expand(B, D),
                                   rtol=0, atol=0)
        assert float(m.ln.scale.grad.abs().max()) == 0.0


def test_module_call_signature(dev):
    """``module(x)`` on readout tokens (B, n, D) returns (B, 1, D) like the reference; a fresh
    module creates and initialises its own parameters on the first call."""
    from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import (
        MLPBlock, MultiHeadAttentionPooling)
    from multi_modal_transformers_tokenmerge_amd.config_loader import LayerSpec
    m = MultiHeadAttentionPooling(
        None, LayerSpec("flax.linen.MultiHeadDotProductAttention", {"num_heads": 3}),
        LayerSpec("flax.linen.LayerNorm", {"epsilon": EPS, "reduction_axes": [-1]}),
        MLPBlock(LayerSpec("flax.linen.Dense", {"features": 96}), None, None,
                 LayerSpec("flax.linen.Dense", {"features": 192})))
    x = torch.randn((2, 4, 192), device=dev)
    y = m(x)
    assert y.shape == (2, 1, 192) and y.dtype == torch.float32
    ref, _ = attention_pool(x.to(torch.bfloat16).double(), module_params(m), EPS, (-1,))
    ref = ref.detach()
    assert float((y.double() - ref).norm() / ref.norm()) <= 2e-2


# ------------------------------------------------------------------ inside the training step
def _model(dev, **kw):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import Octo, create_octo_train_state
    cfg = get_config("octo-tiny", num_blocks=2, readout_pooling="attention", **kw)
    model = Octo(cfg, dev, seed=0)
    return model, create_octo_train_state(model, seed=11)


def _batch(model, B, dev):
    images, text, actions = _inputs(model, B, seed=3)
    return (None if text is None else torch.from_numpy(text).to(dev),
            torch.from_numpy(images).to(dev), torch.from_numpy(actions).to(dev))


@pytest.mark.parametrize("tcs", [None, "[Image{2};Readout{0}]"], ids=["plain", "tome2"])
def test_training_step(dev, tcs, monkeypatch):
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import diffusion_train_step
    model, state = _model(dev, token_compression_sequence=tcs)
    pool = model.pooling
    B = 4
    txt, img, act = _batch(model, B, dev)
    rows = model.readout_rows.cpu().tolist()
    if tcs:   # the readout rows sit behind the merged image set of the final layout
        assert model.L_final == model.L0 - 2 * 2 and rows == list(range(model.L_final - 4, model.L_final))
    rec = {}
    fwd, bwd = pool.forward, pool.backward

    def rec_fwd(x, rows_t, out=None):
        if "xL" not in rec:   # the first step's final sequence and the weights it ran with
            rec["xL"], rec["P"] = x.clone(), module_params(pool)
        return fwd(x, rows_t, out=out)

    def rec_bwd(de, sv, flag):
        rec.setdefault("de", de.clone())
        return bwd(de, sv, flag)
    monkeypatch.setattr(pool, "forward", rec_fwd)
    monkeypatch.setattr(pool, "backward", rec_bwd)
    pre = "diffusion_action_head/MultiHeadAttentionPooling_0/"
    for step in range(3):
        state, grads = diffusion_train_step(model, state, txt, img, act)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(state.last_loss).all()), step
        names = [k for k in grads if k.startswith(pre)]
        assert len(names) == 13
        for k in names:
            assert bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0.0, (step, k)
        assert float(model.stack.blocks[0].qkv.w.grad.abs().max()) > 0.0
        if step == 0:
            gq = grads[pre + "learnt_q_input"].clone()
    # d(loss of step 1) / d(learnt_q_input): the restatement on the saved final sequence with the
    # head's gradient of the pooled embedding as the upstream
    P = rec["P"]
    xr = rec["xL"][:, rows].to(torch.bfloat16).double()
    ref, _ = attention_pool(xr, P, model.cfg.layer_norm_eps, model.cfg.pooling_norm_axes,
                            storage=bf16_storage)
    (ref[:, 0] * rec["de"].double()).sum().backward()
    c = _cos(gq, P["learnt_q_input"].grad)
    print(f"learnt_q_input gradient cosine {c:.6f}")
    assert c >= 0.999
    a = model.predict_diffusion_action(txt, img, state.rng)
    torch.cuda.synchronize()
    assert a.shape == (B, 8) and bool(torch.isfinite(a).all()) and float(a.abs().max()) <= 5.0
    e = model.predict_diffusion_denoise_term(txt, img, torch.zeros(B, dtype=torch.int32, device=dev),
                                             torch.zeros((B, 8), device=dev), state.rng)
    assert e.shape == (B, 8) and bool(torch.isfinite(e).all())
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    K.device_status()


def test_head_reference_signature_pools_through_module(dev):
    """denoise_loss / predict_denoise_term / predict_action on readout tokens (B, n, D) pool
    through the module when it is on: the same numbers as the module's own forward feeding the
    *_mean entry points."""
    model, state = _model(dev)
    head, pool = model.head, model.pooling
    B, n, D = 3, 4, model.D
    g = torch.Generator().manual_seed(5)
    readouts = torch.randn((B, n, D), generator=g).to(dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    e, _ = pool.forward(readouts, rows)
    t = torch.tensor([0, 7, 31], dtype=torch.int32, device=dev)
    noisy = torch.randn((B, 8), generator=g).to(dev)
    got = head.predict_denoise_term(readouts, t, noisy)
    want = head.predict_denoise_term_mean(e, t, noisy)
    assert torch.equal(got, want)
    z = torch.randn((B, 8), generator=g).to(dev)
    assert torch.equal(head.predict_action(readouts, z=z), head.predict_action_mean(e, z=z))
    mean = readouts.mean(1).to(torch.bfloat16)
    assert not torch.equal(got, head.predict_denoise_term_mean(mean, t, noisy))
    loss = head.denoise_loss(readouts, torch.zeros((B, 8), device=dev), rng=state.rng)
    assert bool(torch.isfinite(loss).all())


def test_deterministic_reruns_bitwise(dev):
    """Deterministic mode (as tests/test_deterministic_gpu.py enables it): two identical steps
    give bitwise-equal gradients for every pooling parameter (and everything else). B = 40: the
    batch column sums run in more than one workgroup."""
    model, state = _model(dev)
    txt, img, act = _batch(model, 40, dev)

    def step():
        model.store.zero_grad()
        loss, st = model.compute_diffusion_denoise_loss(txt, img, act, True, state.rng, 0)
        model.backward(st)
        torch.cuda.synchronize()
        return float(loss.item()), model.store.flat_grad.clone()
    try:
        model.store.set_deterministic(True)
        l1, g1 = step()
        l2, g2 = step()
        assert int(model.store.det_fx.abs().sum().item()) == 0   # flushed and cleared
    finally:
        model.store.set_deterministic(False)
    assert l1 == l2
    pre = "diffusion_action_head/MultiHeadAttentionPooling_0/"
    pooled = [p for p in model.store.params if p.name.startswith(pre)]
    assert len(pooled) == 13
    for p in pooled:
        sl = slice(p.offset, p.offset + p.numel)
        assert torch.equal(g1[sl], g2[sl]), p.name
        assert float(g1[sl].abs().max()) > 0.0, p.name
    assert torch.equal(g1, g2)
    # and the mode's result is the plain one within the fixed-point resolution
    l3, g3 = step()
    assert l3 == l1
    for p in pooled:
        sl = slice(p.offset, p.offset + p.numel)
        assert float((g3[sl] - g1[sl]).norm()) <= 1e-5 * float(g1[sl].norm()) + 1e-9, p.name


def test_checkpoint_round_trip(dev):
    from multi_modal_transformers_tokenmerge_amd import checkpoint as C
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import Octo
    model, _ = _model(dev)
    other = Octo(model.cfg, dev, seed=7)
    tree = C.flax_msgpack_loads(C.flax_msgpack_dumps(C.to_flax_params(model)))
    leaves = set(C.flatten_tree(tree["diffusion_action_head"]["pooling"]))
    want = {"learnt_q_input", "LayerNorm_0/scale", "LayerNorm_0/bias"}
    want |= {f"{MHA}/{n}/{leaf}" for n in ("query", "key", "value", "out") for leaf in ("kernel", "bias")}
    want |= {f"MLPBlock_0/Dense_{i}/{leaf}" for i in (0, 1) for leaf in ("kernel", "bias")}
    assert leaves == want
    pre = "diffusion_action_head/MultiHeadAttentionPooling_0/"
    assert any(not torch.equal(p.data, q.data) for p, q in zip(model.store.params, other.store.params)
               if p.name.startswith(pre))
    assert C.load_flax_params(other, tree) == []
    for p, q in zip(model.store.params, other.store.params):
        if p.name.startswith(pre):
            assert torch.equal(p.data, q.data), p.name
            assert torch.equal(p.bf16, q.bf16), p.name
