"""CPU: attention pooling of the readout tokens (OctoConfig.readout_pooling = "attention";
MultiHeadAttentionPooling, reference attention.py:122-150) — the configuration surface, the
validation errors, the parameter layout, the argument checks of the new entry points (rejected
before any HIP call, so the fake pointers are never dereferenced) and hand cases of the torch
restatement the GPU tests compare against (tests/attn_pool_ref.py)."""
import pytest
import torch

from attn_pool_ref import MHA, attention_pool, random_params

PTR = 1 << 20          # non-null, 16-B aligned


def _cfg(*a, **k):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    return get_config(*a, **k)


# ------------------------------------------------------------------ configuration surface
def test_preset_and_yaml_load():
    p = _cfg("octo-small-tome16-map")
    assert p.readout_pooling == "attention" and p.pooling_heads == 6
    assert tuple(p.pooling_norm_axes) == (-1,)
    assert p.token_compression_sequence == _cfg("octo-small-tome16").token_compression_sequence
    y = _cfg("octo_small_tome16_map")
    assert y.readout_pooling == "attention" and y.pooling_heads == 6
    assert y.pooling_mlp_dim == y.token_embedding_dim == 384
    assert tuple(y.pooling_norm_axes) == (-1,)
    # every other key of the YAML is the plain ToMe config's
    base = _cfg("octo_small_tome16")
    for f in ("token_embedding_dim", "num_heads", "mlp_dim", "num_blocks", "input_sequence",
              "token_compression_sequence", "compression"):
        assert getattr(y, f) == getattr(base, f), f


def test_default_is_mean_everywhere():
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import PRESETS
    for name, c in PRESETS.items():
        assert c.readout_pooling == ("attention" if name.endswith("-map") else "mean"), name
    assert _cfg("octo_small_tome16").readout_pooling == "mean"
    assert _cfg("ref_octo_base").readout_pooling == "mean"


def test_yaml_reads_reference_pooling_node():
    """The reference schema's attention_pooling node (diffusion.yaml:6-51) supplies the heads, the
    MLP width and the LayerNorm axes when the root keys do not."""
    from multi_modal_transformers_tokenmerge_amd.config_loader import compose, octo_config_from_yaml
    cfg = compose("octo_small_tome16_map")
    node = cfg["action_heads"]["diffusion_action_head"]["attention_pooling"]
    node["dot_product_attention"]["num_heads"] = 3
    node["layer_norm"]["reduction_axes"] = [1]
    c = octo_config_from_yaml(cfg)
    assert c.pooling_heads == 3 and tuple(c.pooling_norm_axes) == (1,)
    cfg["pooling_heads"] = 12
    assert octo_config_from_yaml(cfg).pooling_heads == 12


def test_validation_errors():
    with pytest.raises(ValueError, match="readout_pooling"):
        _cfg("octo-tiny", readout_pooling="max")
    with pytest.raises(ValueError, match="pooling_heads"):
        _cfg("octo-tiny", readout_pooling="attention", pooling_heads=5)   # 192 % 5
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
    dm = {"_target_": "multi_modal_transformers.action_heads.diffusion.OctoDenoise",
          "time_encoder": {"_target_": "multi_modal_transformers.action_heads.diffusion.FourierFeatures",
                           "output_dim": 64},
          "mlp_block": {"_target_": "multi_modal_transformers.attention_blocks.attention.MLPBlock",
                        "dense": {"_target_": "flax.linen.Dense", "features": 64},
                        "dense_out": {"_target_": "flax.linen.Dense", "features": 8}}}
    with pytest.raises(ValueError, match="attention_pooling"):
        DiffusionActionHead(32, None, dm, readout_pooling="attention")
    with pytest.raises(ValueError, match="readout_pooling"):
        DiffusionActionHead(32, None, dm, readout_pooling="sum")
    # "mean" keeps accepting and ignoring the node
    h = DiffusionActionHead(32, {"anything": 1}, dm)
    assert h.pooling is None and h.readout_pooling == "mean"


def test_head_builds_module_from_reference_node():
    """readout_pooling="attention" on the head builds the module from the reference's
    attention_pooling node (reduction_axes [1] there) and declares it after the denoiser."""
    from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
    from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import (
        MultiHeadAttentionPooling)
    from multi_modal_transformers_tokenmerge_amd.config_loader import compose
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    cfg = compose("octo_small_tome16_map")
    node = cfg["action_heads"]["diffusion_action_head"]
    node["attention_pooling"]["layer_norm"]["reduction_axes"] = [1]
    head = DiffusionActionHead(node["diffusion_steps"], node["attention_pooling"],
                               node["denoising_model"], readout_pooling="attention")
    assert isinstance(head.pooling, MultiHeadAttentionPooling)
    assert head.pooling.H == 6 and head.pooling.norm_axis == 1
    mean = DiffusionActionHead(node["diffusion_steps"], node["attention_pooling"],
                               node["denoising_model"])
    s1, s2 = ParamStore(), ParamStore()
    head.bind(s1, "diffusion_action_head", 384)
    mean.bind(s2, "diffusion_action_head", 384)
    n1 = [(p.name, p.offset) for p in s1.params]
    n2 = [(p.name, p.offset) for p in s2.params]
    assert n1[:len(n2)] == n2
    pre = "diffusion_action_head/MultiHeadAttentionPooling_0/"
    assert [n for n, _ in n1[len(n2):]] == [pre + s for s in POOL_NAMES]
    with pytest.raises(NotImplementedError, match="reduction_axes"):
        MultiHeadAttentionPooling(None, {"_target_": "flax.linen.MultiHeadDotProductAttention",
                                         "num_heads": 3},
                                  {"_target_": "flax.linen.LayerNorm", "reduction_axes": [0]},
                                  node["attention_pooling"]["mlp_block"])


POOL_NAMES = ["learnt_q_input", f"{MHA}/query/kernel", f"{MHA}/query/bias", f"{MHA}/kv/kernel",
              f"{MHA}/kv/bias", f"{MHA}/out/kernel", f"{MHA}/out/bias", "LayerNorm_0/scale",
              "LayerNorm_0/bias", "MLPBlock_0/Dense_0/kernel", "MLPBlock_0/Dense_0/bias",
              "MLPBlock_0/Dense_1/kernel", "MLPBlock_0/Dense_1/bias"]


def test_default_store_layout_unchanged():
    """Pooling off: the explicit "mean" is the default config, name for name and offset for offset;
    pooling on: the same list first, the pooling parameters after every head."""
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import Octo
    layout = lambda m: [(p.name, p.offset, p.shape) for p in m.store.params]   # noqa: E731
    a = Octo(_cfg("octo-tiny", num_blocks=2), device="cpu")
    b = Octo(_cfg("octo-tiny", num_blocks=2, readout_pooling="mean"), device="cpu")
    assert layout(a) == layout(b) and a.store.n == b.store.n
    assert a.pooling is None and a.head.pooling is None
    assert torch.equal(a.store.flat, b.store.flat)
    heads = ("diffusion", "continuous", "categorical")
    c = Octo(_cfg("octo-tiny", num_blocks=2, action_heads=heads), device="cpu")
    d = Octo(_cfg("octo-tiny", num_blocks=2, action_heads=heads, readout_pooling="attention"),
             device="cpu")
    lc, ld = layout(c), layout(d)
    assert ld[:len(lc)] == lc
    assert torch.equal(d.store.flat[:c.store.n], c.store.flat)   # same seeded initial values
    pre = "diffusion_action_head/MultiHeadAttentionPooling_0/"
    assert [n for n, _, _ in ld[len(lc):]] == [pre + s for s in POOL_NAMES]
    assert d.head.pooling is d.pooling and d.pooling.H == 3 and d.pooling.norm_axis == -1
    # the last backward stage region still ends at the store's end: the pooling gradients are
    # all-reduced with the heads'
    assert d.grad_regions(2)[0][1] == d.store.n


def test_checkpoint_tree_names_cpu():
    """The Flax tree holds the module under the head's setup attribute `pooling` with split
    key / value leaves in the DenseGeneral layouts, and loads back bitwise (host stores)."""
    from multi_modal_transformers_tokenmerge_amd import checkpoint as C
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import Octo
    cfg = _cfg("octo-tiny", num_blocks=1, readout_pooling="attention")
    a, b = Octo(cfg, device="cpu", seed=0), Octo(cfg, device="cpu", seed=9)
    tree = C.flax_msgpack_loads(C.flax_msgpack_dumps(C.to_flax_params(a)))
    leaves = C.flatten_tree(tree["diffusion_action_head"]["pooling"])
    D, H, Dh = 192, 3, 64
    want = {"learnt_q_input": (1, 1, D), "LayerNorm_0/scale": (D,), "LayerNorm_0/bias": (D,),
            f"{MHA}/out/kernel": (H, Dh, D), f"{MHA}/out/bias": (D,),
            "MLPBlock_0/Dense_0/kernel": (D, D), "MLPBlock_0/Dense_0/bias": (D,),
            "MLPBlock_0/Dense_1/kernel": (D, D), "MLPBlock_0/Dense_1/bias": (D,)}
    for n in ("query", "key", "value"):
        want[f"{MHA}/{n}/kernel"] = (D, H, Dh)
        want[f"{MHA}/{n}/bias"] = (H, Dh)
    assert {k: tuple(v.shape) for k, v in leaves.items()} == want
    assert C.load_flax_params(b, tree) == []
    for p, q in zip(a.store.params, b.store.params):
        assert torch.equal(p.data, q.data), p.name
    # the class auto-name is accepted on import too
    tree["diffusion_action_head"]["MultiHeadAttentionPooling_0"] = \
        tree["diffusion_action_head"].pop("pooling")
    c = Octo(cfg, device="cpu", seed=4)
    assert C.load_flax_params(c, tree) == []
    assert torch.equal(a.store.flat, c.store.flat)


# ------------------------------------------------------------------ the torch restatement
def test_ref_equal_keys_pool_to_the_mean():
    """All keys equal (x rows identical up to the value path): softmax is uniform, so the pooled
    context is the mean of the projected values."""
    B, n, D, H = 2, 5, 24, 3
    P = random_params(D, H, seed=1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn((B, n, D), generator=g, dtype=torch.float64)
    P[f"{MHA}/key/kernel"] = torch.zeros_like(P[f"{MHA}/key/kernel"])   # k_j = bias for every j
    out, aux = attention_pool(x, P)
    assert out.shape == (B, 1, D)
    torch.testing.assert_close(aux["p"], torch.full((B, H, n), 1.0 / n, dtype=torch.float64))
    v = torch.einsum("bjd,dhk->bjhk", x, P[f"{MHA}/value/kernel"]) + P[f"{MHA}/value/bias"]
    torch.testing.assert_close(aux["ctx"], v.mean(1).reshape(B, D), rtol=1e-12, atol=1e-12)
    # and the module's output is a + MLP(LN(a)) of that context
    a = aux["ctx"] @ P[f"{MHA}/out/kernel"].reshape(D, D) + P[f"{MHA}/out/bias"]
    torch.testing.assert_close(aux["a"][:, 0], a, rtol=1e-12, atol=1e-12)


def test_ref_sequence_axis_norm_outputs_bias():
    """reduction_axes [1] on the length-1 pooled sequence: a - mean = 0, so y == bias exactly, the
    output is a + MLP(bias) and no gradient reaches a through the norm."""
    B, n, D, H = 3, 4, 16, 2
    P = {k: v.requires_grad_(True) for k, v in random_params(D, H, seed=3).items()}
    x = torch.randn((B, n, D), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    out, aux = attention_pool(x, P, axes=(1,))
    assert torch.equal(aux["y"], P["LayerNorm_0/bias"].expand(B, 1, D))
    b = P["LayerNorm_0/bias"]
    m = torch.relu(b @ P["MLPBlock_0/Dense_0/kernel"] + P["MLPBlock_0/Dense_0/bias"]) \
        @ P["MLPBlock_0/Dense_1/kernel"] + P["MLPBlock_0/Dense_1/bias"]
    torch.testing.assert_close(out, aux["a"] + m, rtol=1e-12, atol=1e-12)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (g_a,) = torch.autograd.grad((out * w).sum(), aux["a"], retain_graph=True)
    # only the residual branch: the norm's two paths to a (through a and through its mean) cancel,
    # up to the rounding of adding and subtracting rstd * scale * (upstream) ~ 1e3 |w|
    torch.testing.assert_close(g_a, w, rtol=0, atol=1e-10)
    (g_s,) = torch.autograd.grad((out * w).sum(), P["LayerNorm_0/scale"], allow_unused=True)
    assert g_s is None or not g_s.any()
    # the feature-axis norm does send gradient through
    out2, aux2 = attention_pool(x, P, axes=(-1,))
    (g2,) = torch.autograd.grad((out2 * w).sum(), aux2["a"])
    assert float((g2 - w).abs().max()) > 1e-3


# ------------------------------------------------------------------ argument checks (no launch)
def _lib():
    from multi_modal_transformers_tokenmerge_amd import _C
    return _C.lib()


def _pool_fwd(lib, q=PTR, k=PTR, v=PTR, ld=384, B=2, n=4, H=6, Dh=64, ctx=PTR, ld_ctx=384, p=PTR):
    return lib.mmt_attn_pool_fwd(q, k, v, ld, B, n, H, Dh, ctx, ld_ctx, p, None)


def _pool_bwd(lib, n=4, Dh=64, ld=384, dk=PTR, dqb=PTR):
    return lib.mmt_attn_pool_bwd(PTR, 384, PTR, PTR, PTR, PTR, ld, 2, n, 6, Dh, dk, PTR, ld, dqb, None)


REJECTED = [
    ("pool_fwd-n-65", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, n=65)),
    ("pool_fwd-n-0", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, n=0)),
    ("pool_fwd-Dh-60", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, Dh=60, ld=360, ld_ctx=360)),
    ("pool_fwd-Dh-520", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, H=1, Dh=520, ld=520, ld_ctx=520)),
    ("pool_fwd-null-ctx", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, ctx=None)),
    ("pool_fwd-null-p", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, p=None)),
    ("pool_fwd-ld-small", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, ld=376)),
    ("pool_fwd-misaligned", "mmt_attn_pool_fwd", lambda l: _pool_fwd(l, k=PTR + 2)),
    ("pool_bwd-n-65", "mmt_attn_pool_bwd", lambda l: _pool_bwd(l, n=65)),
    ("pool_bwd-Dh-60", "mmt_attn_pool_bwd", lambda l: _pool_bwd(l, Dh=60)),
    ("pool_bwd-null-dk", "mmt_attn_pool_bwd", lambda l: _pool_bwd(l, dk=None)),
    ("pool_bwd-null-dqb", "mmt_attn_pool_bwd", lambda l: _pool_bwd(l, dqb=None)),
    ("gather-D-12", "mmt_rows_gather_bf16",
     lambda l: l.mmt_rows_gather_bf16(PTR, 4096, 16, 2, 11, 12, PTR, 3, PTR, None)),
    ("gather-n-0", "mmt_rows_gather_bf16",
     lambda l: l.mmt_rows_gather_bf16(PTR, 4096, 16, 2, 11, 8, PTR, 0, PTR, None)),
    ("gather-null-r", "mmt_rows_gather_bf16",
     lambda l: l.mmt_rows_gather_bf16(PTR, 4096, 16, 2, 11, 8, PTR, 3, None, None)),
    ("gather-stride", "mmt_rows_gather_bf16",
     lambda l: l.mmt_rows_gather_bf16(PTR, 4096, 10, 2, 11, 8, PTR, 3, PTR, None)),
    ("scatter-L-0", "mmt_rows_scatter_bwd",
     lambda l: l.mmt_rows_scatter_bwd(PTR, 2, 0, 8, PTR, 3, PTR, None)),
    ("scatter-null-dx", "mmt_rows_scatter_bwd",
     lambda l: l.mmt_rows_scatter_bwd(PTR, 2, 11, 8, PTR, 3, None, None)),
    ("ln_fwd-D-12", "mmt_layernorm_fwd",
     lambda l: l.mmt_layernorm_fwd(PTR, 0, 16, 4, 12, PTR, PTR, 1e-6, PTR, 16, PTR, PTR, None)),
    ("ln_fwd-dtype", "mmt_layernorm_fwd",
     lambda l: l.mmt_layernorm_fwd(PTR, 2, 64, 4, 64, PTR, PTR, 1e-6, PTR, 64, PTR, PTR, None)),
    ("ln_fwd-null-mean", "mmt_layernorm_fwd",
     lambda l: l.mmt_layernorm_fwd(PTR, 0, 64, 4, 64, PTR, PTR, 1e-6, PTR, 64, None, PTR, None)),
    ("ln_fwd-ldx-small", "mmt_layernorm_fwd",
     lambda l: l.mmt_layernorm_fwd(PTR, 0, 56, 4, 64, PTR, PTR, 1e-6, PTR, 64, PTR, PTR, None)),
    ("ln_bwd-null-dyxhat", "mmt_layernorm_bwd",
     lambda l: l.mmt_layernorm_bwd(PTR, 1, 64, PTR, 1, 64, 4, 64, PTR, PTR, PTR, None, 0, PTR, 64,
                                   None, None)),
    ("ln_bwd-B-0", "mmt_layernorm_bwd",
     lambda l: l.mmt_layernorm_bwd(PTR, 1, 64, PTR, 1, 64, 0, 64, PTR, PTR, PTR, None, 0, PTR, 64,
                                   PTR, None)),
    ("ln_bwd-addend-stride", "mmt_layernorm_bwd",
     lambda l: l.mmt_layernorm_bwd(PTR, 1, 64, PTR, 1, 64, 4, 64, PTR, PTR, PTR, PTR, 60, PTR, 64,
                                   PTR, None)),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_bad_arguments_are_errors(case):
    _, entry, call = case
    lib = _lib()
    assert call(lib) == -1
    assert entry.encode() in lib.mmt_last_error()


def test_signatures_match_header():
    """The binding table's argument counts are the header's (a drifted count would shift every
    later argument of a ctypes call)."""
    import re
    from pathlib import Path
    from multi_modal_transformers_tokenmerge_amd import _C
    txt = (Path(__file__).resolve().parents[1] / "include" / "mmt_api.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mmt_rows_gather_bf16", "mmt_rows_scatter_bwd", "mmt_attn_pool_fwd",
                 "mmt_attn_pool_bwd", "mmt_layernorm_fwd", "mmt_layernorm_bwd"):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", txt)
        assert m, name
        assert len(_C.SIGNATURES[name]) == len(m.group(1).split(",")), name
        assert _C.SIGNATURES[name][-1] == _C.P
