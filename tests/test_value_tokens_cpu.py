"""CPU: value tokens (tokenizers/numeric_values, the Value token set, include/mmt_api.h "value
tokens") without a GPU: the numpy reference's own checks, the grammar and attention rules of
Value, the compression and configuration errors, the YAML schema, and the argument checks of both
entry points on the CPU-loaded library (rejected before any HIP call; pointers are never
dereferenced there, so any aligned non-null value serves)."""
import numpy as np
import pytest
import torch

from tests import value_tokens_ref as R

SEQ = "[TaskDescriptionPrefix{2}] [Image{4};Value{3};Readout{2}]*2"
#        P  I1 V1 R1 I2 V2 R2   (row = query set, 1 = sees)
TABLE = [[1, 0, 0, 0, 0, 0, 0],
         [1, 1, 1, 0, 0, 0, 0],
         [1, 1, 1, 0, 0, 0, 0],
         [1, 1, 1, 1, 0, 0, 0],
         [1, 1, 1, 0, 1, 1, 0],
         [1, 1, 1, 0, 1, 1, 0],
         [1, 1, 1, 0, 1, 1, 1]]


# ---------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("N", [2, 16, 256, 1024, 4096])
@pytest.mark.parametrize("encoding", R.ENCODINGS)
def test_reference_fixed_points(N, encoding):
    np.testing.assert_array_equal(R.tokens(R.FIXED_POINTS, N, 255.0, encoding),
                                  R.fixed_point_tokens(N))


@pytest.mark.parametrize("encoding", R.ENCODINGS)
@pytest.mark.parametrize("mu", [100.0, 255.0])
def test_reference_tokens_are_monotone_and_cover_every_bin(encoding, mu):
    v = np.linspace(-1.25, 1.25, 20001).astype(np.float32)
    t = R.tokens(v, 256, mu, encoding)
    assert (np.diff(t) >= 0).all() and t[0] == 0 and t[-1] == 255
    assert len(np.unique(t)) == 256


@pytest.mark.parametrize("N", [16, 256, 1024])
@pytest.mark.parametrize("mu", [100.0, 255.0])
@pytest.mark.parametrize("encoding", R.ENCODINGS)
def test_bin_centre_values_reproduce_their_token(N, mu, encoding):
    """The GPU tests' inputs: every token exactly, for every element, with log1p and with
    log(1 + x) in fp32."""
    rng = np.random.default_rng(0)
    k = np.tile(np.arange(N), 8)
    v = R.bin_centre_values(k, N, mu, encoding, rng)
    np.testing.assert_array_equal(R.tokens(v, N, mu, encoding), k)
    if encoding == "mu_law":
        f = np.float32
        y = np.copysign(np.log(f(1) + f(mu) * np.abs(v)) / np.log(f(1) + f(mu)), v).astype(f)
        np.testing.assert_array_equal(np.floor((y + f(1)) * f(0.5) * f(N)).astype(np.int64), k)


def test_mu_law_encoder_matches_the_formula():
    from multi_modal_transformers_tokenmerge_amd.tokenizers.numeric_values.value_tokenizer import \
        mu_law_encoder
    x = torch.linspace(-1, 1, 257, dtype=torch.float64)
    for mu in (255, 100.0):
        np.testing.assert_allclose(mu_law_encoder(x, mu).numpy(), R.mu_law(x.numpy(), mu),
                                   rtol=1e-12, atol=1e-15)
    got = mu_law_encoder(torch.tensor([-1.0, 0.0, 1.0]))
    assert got.tolist() == [-1.0, 0.0, 1.0]


def test_reference_table_grad_is_the_ordered_sum():
    rng = np.random.default_rng(1)
    dx0 = rng.standard_normal((3, 6, 8)).astype(np.float32)
    tok = np.array([[0, 1], [1, 1], [0, 3]], np.int32)
    rows = [2, 5]
    g = R.table_grad(dx0, tok, rows, 4)
    f = np.float32
    np.testing.assert_array_equal(g[1], (f(0) + dx0[0, 5] + dx0[1, 2]) + dx0[1, 5])
    np.testing.assert_array_equal(g[0], f(0) + dx0[0, 2] + dx0[2, 2])
    assert not g[2].any()


# ---------------------------------------------------------------------------- grammar and rules
def test_value_parses_and_has_a_modality():
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_sequencer import (
        TokenEmbeddings, TokenSequence, Value)
    seq = TokenSequence(SEQ)
    kinds = [type(ts).__name__ for ts in seq.token_sequence]
    assert kinds == ["TaskDescriptionPrefix", "Image", "Value", "Readout", "Image", "Value",
                     "Readout"]
    vs = [ts for ts in seq.token_sequence if isinstance(ts, Value)]
    assert [(v.num_tokens, v.timestep, v.modality) for v in vs] == [(3, 1, "values"),
                                                                    (3, 2, "values")]
    np.testing.assert_array_equal(seq.get_modality_idx("values"), [6, 7, 8, 15, 16, 17])
    assert [seq.slice_idx[i] for i in (2, 5)] == [(0, 3), (3, 3)]
    assert TokenEmbeddings().values is None


def test_set_table_and_dense_mask_follow_the_rules():
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_sequencer import (
        TokenSequence, dense_mask_of, sets_from_mask)
    seq = TokenSequence(SEQ)
    sets = seq.set_table(0)
    got = [[(v >> k) & 1 for k in range(7)] for v in sets.vis]
    assert got == TABLE
    assert sets.lens == [2, 4, 3, 2, 4, 3, 2] and sets.modalities[2] == "values"
    assert not any(sets.causal)
    dense = seq.generate_attention_mask(square=True)[0]
    want = np.kron(np.array(TABLE, bool), np.ones((1, 1), bool))
    sid = np.repeat(np.arange(7), sets.lens)
    np.testing.assert_array_equal(dense, want[sid][:, sid])
    np.testing.assert_array_equal(dense_mask_of(sets), dense)
    # round trip: a dense mask segments into sets that stand for the same mask (adjacent sets
    # with equal rules, I1 | V1, may come back as one)
    back = sets_from_mask(dense)
    np.testing.assert_array_equal(dense_mask_of(back), dense)
    assert back.L == sets.L


def _tiny(**kw):
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    return get_config("octo-tiny", num_blocks=2, **kw)


@pytest.mark.parametrize("method", ["tome", "prune"])
def test_compressing_a_value_set_raises(method):
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    cfg = _tiny(input_sequence="[Image{16};Value{5};Readout{4}]",
                token_compression_sequence="[Image{2};Value{1};Readout{0}]", compression=method)
    with pytest.raises(ValueError, match="Value sets are never compressed"):
        O.Octo(cfg, torch.device("cpu"))


def test_host_built_model_declares_the_embedding_last():
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    base = O.Octo(_tiny(), torch.device("cpu"))
    m = O.Octo(_tiny(input_sequence="[Image{16};Value{5};Readout{4}]",
                     token_compression_sequence="[Image{2};Value{0};Readout{0}]",
                     value_tokenizer=dict(num_bins=64)), torch.device("cpu"))
    names = [p.name for p in m.store.params]
    assert names[-1] == "ValueTokenizer_0/embedding"
    assert "ValueTokenizer_0/embedding" not in base.store.by_name
    emb = m.store.by_name["ValueTokenizer_0/embedding"]
    assert emb.shape == (64, m.D)
    assert abs(float(emb.data.std()) - m.D ** -0.5) < 0.1 * m.D ** -0.5   # nn.Embed's default
    # every parameter both models share sits at the same offset, except the position embedding
    # (one row per sequence position: 5 more) and what follows it
    for p in base.store.params:
        if p.name == "StackedEncoder1DBlock_0/posembed_input/pos_embedding":
            break
        assert m.store.by_name[p.name].offset == p.offset
    assert m.value_rows.tolist() == [16, 17, 18, 19, 20] and m.n_values == 5
    assert [v >> 24 for v in m.row_src.tolist()] == [1] * 16 + [3] * 5 + [2] * 4
    # Value keeps its length while the image set shrinks; the readouts follow it
    assert [m.layer_sets[i][0].lens for i in range(2)] == [[16, 5, 4], [14, 5, 4]]
    assert m.L_final == 12 + 5 + 4 and m.readout_rows.tolist() == [17, 18, 19, 20]
    # parameter groups: the Octo recipe leaves the embedding undecayed; head_only freezes it
    st = O.create_octo_train_state(m, O.AdamW(weight_decay_mask="kernels"))
    assert st.param_groups["ValueTokenizer_0/embedding"] == {"decay": False, "frozen": False}
    O.create_octo_train_state(m, O.AdamW(frozen_keys="head_only"))
    assert m._cut == (2, True) and emb.frozen
    O.create_octo_train_state(m, O.AdamW(frozen_keys=[n for n in names if n != emb.name]))
    assert m._cut == (0, False)        # the embedding alone is trained: the whole backward
    O.create_octo_train_state(m, O.AdamW())
    # the staged backward: the embedding's gradient is a region of its own, final last
    assert m.tail_region() == (emb.offset, m.store.n) and base.tail_region() is None
    assert m.grad_regions(2)[0][1] == emb.offset and m.grad_regions(1) == [(0, m.store.n)]
    assert base.grad_regions(2)[0][1] == base.store.n
    # values are checked before anything is launched
    with pytest.raises(ValueError, match="pass values"):
        m._check_values(None, 3)
    with pytest.raises(ValueError, match="no Value set"):
        base._check_values(torch.zeros(3, 5), 3)


def test_ddp_step_reduces_the_embedding_gradient_after_the_last_stage():
    """distributed.DDPStep's plan over a 2-stage backward, built on the host (nothing is
    launched): the embedding's gradient lies past the heads but is written by the token backward,
    so it is all-reduced after the last stage and counts as exposed."""
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep, GradAllReducer
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    m = O.Octo(_tiny(input_sequence="[Image{16};Value{5};Readout{4}]"), torch.device("cpu"))
    emb = m.store.by_name["ValueTokenizer_0/embedding"]
    red = GradAllReducer(2)
    img = torch.zeros((3, 1, 64, 64, 3), dtype=torch.uint8)
    vals = torch.zeros((3, 5))

    def plan(tx, **kw):
        state = O.create_octo_train_state(m, tx, allreduce=red)
        return DDPStep(m, state, None, img, None, red, stages=2, use_graph=False, **kw)
    d = plan(O.AdamW(), values=vals)
    regions = m.grad_regions(2)
    assert d.tail == (emb.offset, m.store.n) and regions[0][1] == emb.offset
    assert d.exposed_bytes == 4 * (regions[1][1] - regions[1][0]) + 4 * (m.store.n - emb.offset)
    assert plan(O.AdamW(frozen_keys=[emb.name]), values=vals).tail is None
    with pytest.raises(ValueError, match="pass values"):
        plan(O.AdamW())
    with pytest.raises(ValueError):
        plan(O.AdamW(), values=vals[:2])
    O.create_octo_train_state(m, O.AdamW())


# ---------------------------------------------------------------------------- configuration
def test_yaml_loads_to_the_preset():
    from dataclasses import asdict
    from multi_modal_transformers_tokenmerge_amd import config_loader as C
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import PRESETS
    a = asdict(C.load_octo_config("octo_small_tome16_proprio8"))
    b = asdict(PRESETS["octo-small-tome16-proprio8"])
    diff = {k: (a[k], b[k]) for k in a if k not in ("name", "stem") and a[k] != b[k]}
    assert not diff
    assert a["value_tokenizer"] == dict(num_bins=256, mu=255.0, encoding="mu_law")
    node = C.compose("octo_small_tome16_proprio8")["tokenizers"]["values"]["encoder"]
    tok = C.instantiate(node)
    assert (type(tok).__name__, tok.num_bins, tok.mu, tok.encoding) == ("ValueTokenizer", 256,
                                                                        255.0, "mu_law")
    assert C.load_octo_config("octo_small_tome16").value_tokenizer is None


@pytest.mark.parametrize("bad", [dict(num_bins=1), dict(num_bins=4097), dict(num_bins=16.0),
                                 dict(num_bins=True), dict(mu=0.0), dict(mu=-1.0),
                                 dict(mu=float("inf")), dict(mu=float("nan")), dict(mu="255"),
                                 dict(encoding="a_law"), dict(bins=16), [256]])
def test_bad_value_tokenizer_configs_raise(bad):
    from multi_modal_transformers_tokenmerge_amd.tokenizers.numeric_values.value_tokenizer import \
        ValueTokenizer
    with pytest.raises(ValueError):
        _tiny(value_tokenizer=bad)
    if isinstance(bad, dict) and "bins" not in bad:
        with pytest.raises(ValueError):
            ValueTokenizer(**bad)


def test_value_tokenizer_config_without_value_sets_raises():
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    with pytest.raises(ValueError, match="no Value set"):
        O.Octo(_tiny(value_tokenizer=dict(num_bins=16)), torch.device("cpu"))


# ---------------------------------------------------------------------------- argument checks
PTR = 1 << 20          # non-null, 16-B aligned
NAN, INF = float("nan"), float("inf")


def _fwd(lib, values=PTR, ld_v=5, B=2, n=5, encoding=1, mu=255.0, N=256, table=PTR, pe=PTR,
         rows=PTR, D=8, x0=PTR, xs_b=200, xs_t=8, tok=PTR):
    return lib.mmt_value_tokens_fwd(values, ld_v, B, n, encoding, mu, N, table, pe, rows, D, x0,
                                    xs_b, xs_t, tok, None)


def _bwd(lib, dx0=PTR, xs_b=200, xs_t=8, B=2, n=5, tok=PTR, rows=PTR, D=8, N=256, dtable=PTR):
    return lib.mmt_value_tokens_bwd(dx0, xs_b, xs_t, B, n, tok, rows, D, N, dtable, None)


REJECTED = [
    ("fwd-null-values", "fwd", lambda l: _fwd(l, values=None)),
    ("fwd-null-table", "fwd", lambda l: _fwd(l, table=None)),
    ("fwd-null-pe", "fwd", lambda l: _fwd(l, pe=None)),
    ("fwd-null-rows", "fwd", lambda l: _fwd(l, rows=None)),
    ("fwd-null-x0", "fwd", lambda l: _fwd(l, x0=None)),
    ("fwd-null-tok", "fwd", lambda l: _fwd(l, tok=None)),
    ("fwd-B-0", "fwd", lambda l: _fwd(l, B=0)),
    ("fwd-B-neg", "fwd", lambda l: _fwd(l, B=-2)),
    ("fwd-n-0", "fwd", lambda l: _fwd(l, n=0, ld_v=0)),
    ("fwd-n-neg", "fwd", lambda l: _fwd(l, n=-1)),
    ("fwd-D-0", "fwd", lambda l: _fwd(l, D=0)),
    ("fwd-D-neg", "fwd", lambda l: _fwd(l, D=-8)),
    ("fwd-D-12", "fwd", lambda l: _fwd(l, D=12, xs_t=12)),
    ("fwd-bins-1", "fwd", lambda l: _fwd(l, N=1)),
    ("fwd-bins-4097", "fwd", lambda l: _fwd(l, N=4097)),
    ("fwd-mu-0", "fwd", lambda l: _fwd(l, mu=0.0)),
    ("fwd-mu-neg", "fwd", lambda l: _fwd(l, mu=-255.0)),
    ("fwd-mu-inf", "fwd", lambda l: _fwd(l, mu=INF)),
    ("fwd-mu-nan", "fwd", lambda l: _fwd(l, mu=NAN)),
    ("fwd-encoding-2", "fwd", lambda l: _fwd(l, encoding=2)),
    ("fwd-encoding-neg", "fwd", lambda l: _fwd(l, encoding=-1)),
    ("fwd-x0-unaligned", "fwd", lambda l: _fwd(l, x0=PTR + 4)),
    ("fwd-table-unaligned", "fwd", lambda l: _fwd(l, table=PTR + 8)),
    ("fwd-xs_t-lt-D", "fwd", lambda l: _fwd(l, D=16, xs_t=8)),
    ("fwd-xs_t-not-4", "fwd", lambda l: _fwd(l, xs_t=10)),
    ("fwd-xs_b-not-4", "fwd", lambda l: _fwd(l, xs_b=202)),
    ("bwd-null-dx0", "bwd", lambda l: _bwd(l, dx0=None)),
    ("bwd-null-tok", "bwd", lambda l: _bwd(l, tok=None)),
    ("bwd-null-rows", "bwd", lambda l: _bwd(l, rows=None)),
    ("bwd-null-dtable", "bwd", lambda l: _bwd(l, dtable=None)),
    ("bwd-B-0", "bwd", lambda l: _bwd(l, B=0)),
    ("bwd-n-0", "bwd", lambda l: _bwd(l, n=0)),
    ("bwd-n-neg", "bwd", lambda l: _bwd(l, n=-3)),
    ("bwd-D-0", "bwd", lambda l: _bwd(l, D=0)),
    ("bwd-D-12", "bwd", lambda l: _bwd(l, D=12, xs_t=12)),
    ("bwd-bins-1", "bwd", lambda l: _bwd(l, N=1)),
    ("bwd-bins-4097", "bwd", lambda l: _bwd(l, N=4097)),
    ("bwd-dx0-unaligned", "bwd", lambda l: _bwd(l, dx0=PTR + 4)),
    ("bwd-dtable-unaligned", "bwd", lambda l: _bwd(l, dtable=PTR + 8)),
    ("bwd-xs_t-lt-D", "bwd", lambda l: _bwd(l, D=16, xs_t=8)),
    ("bwd-xs_t-not-4", "bwd", lambda l: _bwd(l, xs_t=10)),
    ("bwd-xs_b-not-4", "bwd", lambda l: _bwd(l, xs_b=202)),
]


@pytest.mark.parametrize("which,call", [c[1:] for c in REJECTED], ids=[c[0] for c in REJECTED])
def test_entry_points_reject_bad_arguments_without_gpu(which, call):
    """Every rejection the header lists: MMT_ERR_INVALID, a message naming the entry point,
    nothing launched."""
    from multi_modal_transformers_tokenmerge_amd import _C
    lib = _C.lib()
    # leave another entry point's message behind first, so a stale one cannot satisfy the check
    assert lib.mmt_step_advance(None, None) == -1 and b"mmt_step_advance" in lib.mmt_last_error()
    assert call(lib) == -1                       # MMT_ERR_INVALID
    msg = lib.mmt_last_error()
    assert msg and f"mmt_value_tokens_{which}".encode() in msg, msg


def test_assemble_rows_have_a_kind_of_their_own():
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    assert (O.KIND_TEXT, O.KIND_IMAGE, O.KIND_READOUT, O.KIND_VALUE) == (0, 1, 2, 3)
