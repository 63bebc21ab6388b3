"""CPU: the observation pad masks (include/mmt_api.h "observation pad masks") without a GPU: the
TokenSequence helper, every ValueError of the Python surface raised before libmmt_hip is called,
the restatement's own sanity (tests/pad_mask_ref.py), the binding table, and the argument checks
of the five entry points on the CPU-loaded library (rejected before any HIP call; device pointers
are never dereferenced there, so any aligned non-null value serves; the set tables are host
arrays and real)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import pad_mask_ref as R

ROOT = Path(__file__).resolve().parents[1]
SEQ = "[TaskDescriptionPrefix{8}] [Image{16};Image{16};Readout{4}]*2"


# ------------------------------------------------------------------------------ the helper
def test_token_sequence_layout():
    from multi_modal_transformers_tokenmerge_amd.tokenizers.token_sequencer import TokenSequence
    assert TokenSequence(SEQ).pad_mask_layout() == (7, 0b1001000, 0)
    assert TokenSequence("[Image{16};Readout{4}]").pad_mask_layout() == (2, 0b10, -1)
    # the first text-class set, whichever class it is
    assert TokenSequence("[Image{16};Readout{4}] [Text{8}]").pad_mask_layout() == (3, 0b010, 2)
    assert TokenSequence("[Text{32}] [Image{256};Image{256};Readout{4}]*2").pad_mask_layout()[0] == 7


def test_constant_is_exported_and_matches_the_header():
    from multi_modal_transformers_tokenmerge_amd import _C, _kernels as K
    text = (ROOT / "include" / "mmt_api.h").read_text()
    m = re.search(r"#define\s+MMT_PAD_MASK_LOGIT\s+\((-[0-9.]+)f\)", text)
    assert m and float(m.group(1)) == _C.PAD_MASK_LOGIT == K.PAD_MASK_LOGIT == R.M == -1024.0
    assert re.search(r"MMT_FAULT_PAD_MASK\s*=\s*16\b", text) and _C.FAULT_PAD_MASK == 16
    assert re.search(r"#define\s+MMT_PAD_MASK_MAX_SETS\s+16\b", text)
    # exact in fp32, and so is the quotient by the power-of-two scales (Dh 64: 1/8, 256: 1/16)
    for scale in (0.125, 0.0625):
        q = np.float32(R.M) / np.float32(scale)
        assert float(q) == R.M / scale and float(q * np.float32(scale)) == R.M


def _header_arg_count(name):
    text = (ROOT / "include" / "mmt_api.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mmt_api.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ["mmt_pad_mask_pack", "mmt_pad_mask_bias", "mmt_pad_mask_rows_fwd",
                                  "mmt_pad_mask_rows_bwd", "mmt_pad_mask_images"])
def test_binding_lists_the_entry_points(name):
    from multi_modal_transformers_tokenmerge_amd import _C
    assert name in _C.SIGNATURES and len(_C.SIGNATURES[name]) == _header_arg_count(name)
    assert hasattr(_C.lib(), name)


# ------------------------------------------------------------------------ the restatement
def test_restatement_masked_rows_and_words():
    starts, lens = [0, 5, 12, 15], [5, 7, 3, 4]
    sm = np.array([[1, 0, 1, 1], [1, 1, 1, 0], [0, 0, 0, 0]], bool)
    assert R.pack(sm).tolist() == [0b1101, 0b0111, 0]
    assert R.pack(sm, 0b1000).tolist() == [0b1101, 0b1111, 0b1000]   # a Readout set stays present
    tm = np.array([[1, 1, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]], bool)
    m = R.masked_rows(starts, lens, 3, sm, tm, 0, 0b1000)
    assert m.shape == (3, 19)
    assert m[0].tolist() == [0, 0, 1, 1, 1] + [1] * 7 + [0] * 3 + [0] * 4
    assert m[1].tolist() == [0] * 19
    assert m[2].tolist() == [1] * 15 + [0] * 4
    kb = R.bias_rows(m, 64)
    assert kb.shape == (3, 64) and (kb[:, 19:] == 0).all() and kb.dtype == np.float32
    assert ((kb[:, :19] == R.M) == m).all() and ((kb[:, :19] == 0) == ~m).all()
    base = np.full((3, 64), 0.5, np.float32)
    base[:, 19:] = np.nan
    acc = R.bias_rows(m, 64, base)
    assert (acc[:, :19][m] == np.float32(0.5) + np.float32(R.M)).all()
    assert (acc[:, :19][~m] == 0.5).all() and np.isnan(acc[:, 19:]).all()


def test_restatement_masked_key_has_weight_exactly_zero():
    """float64: exp(M + s - max) underflows to exactly 0 (e^-1024 is below the smallest float64
    denormal, e^-745), so the masked attention equals the attention with those keys removed; a
    row whose visible keys are all masked is the unmasked softmax (shift invariance)."""
    g = torch.Generator().manual_seed(0)
    B, L, H, Dh = 2, 12, 2, 8
    qkv = torch.randn((B, L, 3 * H * Dh), generator=g, dtype=torch.float64)
    starts, lens, vis = [0, 4, 10], [4, 6, 2], [0b001, 0b011, 0b111]
    mask = R.dense_mask(starts, lens, vis)
    sm = np.array([[0, 1, 1], [1, 0, 1]], bool)
    masked = R.masked_rows(starts, lens, B, sm)
    kb = torch.from_numpy(R.bias_rows(masked, 64)).double()
    o1, lse1 = R.masked_attention(qkv, H, Dh ** -0.5, mask, kb)
    o0, _ = R.masked_attention(qkv, H, Dh ** -0.5, mask)
    assert torch.isfinite(o1).all() and torch.isfinite(lse1).all()
    q, k, v = qkv.view(B, L, 3, H, Dh).unbind(2)
    for b in range(B):
        s = torch.einsum("qhd,khd->hqk", q[b], k[b]) * Dh ** -0.5 + kb[b, None, None, :L]
        s = torch.where(mask[None], s, torch.finfo(torch.float64).min)
        p = torch.softmax(s, -1)
        for qi in range(L):
            seen = mask[qi].numpy()
            if (seen & ~masked[b]).any():   # a present key in sight: the masked ones weigh 0.0
                assert (p[:, qi, torch.from_numpy(seen & masked[b])] == 0).all()
        # the same attention with the masked keys taken out of the visible set
        keep = mask & torch.from_numpy(~masked[b])[None, :]
        rows = keep.any(1)
        s2 = torch.einsum("qhd,khd->hqk", q[b], k[b]) * Dh ** -0.5
        p2 = torch.softmax(torch.where(keep[None], s2, -torch.inf), -1)
        o2 = torch.einsum("hqk,khd->qhd", p2[:, rows], v[b]).reshape(-1, H * Dh)
        assert torch.allclose(o1[b, rows], o2, rtol=0, atol=1e-14)
    # sample 0, set 0 absent: its queries see set 0 alone, all masked -> the unmasked softmax
    assert torch.allclose(o1[0, :4], o0[0, :4], rtol=0, atol=1e-13)
    assert not torch.allclose(o1[0, 4:], o0[0, 4:], atol=1e-3)


def test_restatement_rows():
    rng = np.random.default_rng(0)
    x0, pe = rng.normal(size=(2, 5, 4)).astype(np.float32), rng.normal(size=(5, 4)).astype(np.float32)
    m = np.array([[0, 1, 0, 0, 1], [0, 0, 0, 0, 0]], bool)
    y, z = R.rows_fwd(x0, pe, m), R.rows_bwd(x0, m)
    assert (y[0, 1] == pe[1]).all() and (y[0, 4] == pe[4]).all() and (y[~m] == x0[~m]).all()
    assert (z[m] == 0).all() and (z[~m] == x0[~m]).all()


# -------------------------------------------------------------------- the Python surface
def _model(**kw):
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    from multi_modal_transformers_tokenmerge_amd.tokenizers.text.t5_base import T5Config
    base = dict(num_blocks=2, text_tokens=8, t5=T5Config(num_layers=1, vocab_size=64),
                input_sequence="[TaskDescriptionPrefix{8}] [Image{16};Image{16};Readout{4}]",
                token_compression_sequence="[TaskDescriptionPrefix{0}] [Image{2};Image{2};Readout{0}]")
    base.update(kw)
    return O.Octo(get_config("octo-tiny", **base), torch.device("cpu")), O


@pytest.fixture(scope="module")
def model():
    return _model()[0]


@pytest.fixture()
def no_library(monkeypatch):
    """Any call into libmmt_hip fails the test: the errors below come before every launch."""
    from multi_modal_transformers_tokenmerge_amd import _C

    def boom(name, *a):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_C, "call", boom)


B = 4


def _bad_masks():
    ok_s, ok_t = torch.ones((B, 4), dtype=torch.bool), torch.ones((B, 8), dtype=torch.bool)
    return [
        ("set-dtype", dict(set_pad_mask=ok_s.to(torch.uint8))),
        ("set-float", dict(set_pad_mask=ok_s.float())),
        ("set-not-a-tensor", dict(set_pad_mask=[[True] * 4] * B)),
        ("set-count", dict(set_pad_mask=torch.ones((B, 3), dtype=torch.bool))),
        ("set-count-more", dict(set_pad_mask=torch.ones((B, 7), dtype=torch.bool))),
        ("set-batch", dict(set_pad_mask=ok_s[:2])),
        ("set-rank", dict(set_pad_mask=ok_s.view(-1))),
        ("text-dtype", dict(text_pad_mask=ok_t.long())),
        ("text-length", dict(text_pad_mask=torch.ones((B, 32), dtype=torch.bool))),
        ("text-batch", dict(text_pad_mask=ok_t[:3])),
        ("text-rank", dict(text_pad_mask=ok_t.view(B, 8, 1))),
        ("both-one-bad", dict(set_pad_mask=ok_s, text_pad_mask=ok_t[:, :5])),
    ]


@pytest.mark.parametrize("kw", [c[1] for c in _bad_masks()], ids=[c[0] for c in _bad_masks()])
def test_bad_masks_raise_before_any_launch(model, no_library, kw):
    images = torch.zeros((B, 2, 64, 64, 3), dtype=torch.uint8)
    txt = torch.zeros((B, 8), dtype=torch.int64)
    act = torch.zeros((B, model.cfg.action_space_dim))
    with pytest.raises(ValueError, match="pad_mask"):
        model._check_pad_masks(kw.get("set_pad_mask"), kw.get("text_pad_mask"), B)
    # and through the public functions, which check before they launch anything
    for fn, args in ((model.generate_readouts, (txt, images)),
                     (model.compute_diffusion_denoise_loss, (txt, images, act)),
                     (model.predict_diffusion_action, (txt, images, None))):
        with pytest.raises(ValueError, match="pad_mask"):
            fn(*args, **kw)


def test_masks_on_the_wrong_device_raise(no_library):
    from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import check_pad_masks
    ok = torch.ones((B, 4), dtype=torch.bool)
    check_pad_masks(ok, None, B, 4, 8, "cpu")
    with pytest.raises(ValueError, match="device"):
        check_pad_masks(ok, None, B, 4, 8, "cuda")
    with pytest.raises(ValueError, match="contiguous"):
        check_pad_masks(torch.ones((4, B), dtype=torch.bool).t(), None, B, 4, 8)


def test_none_masks_pass_and_good_masks_pass(model, no_library):
    assert model._check_pad_masks(None, None, B) is False
    assert model._check_pad_masks(torch.ones((B, 4), dtype=torch.bool), None, B) is True
    assert model._check_pad_masks(None, torch.ones((B, 8), dtype=torch.bool), B) is True
    assert (model.n_sets, model.readout_set_bits, model.text_set) == (4, 0b1000, 0)


def test_image_copy_limits_are_checked_on_the_host(model, no_library):
    """mmt_pad_mask_images' limits (B * I <= 65535 images, image bytes a multiple of 16) as
    ValueError before any launch, under a set mask only."""
    sm = torch.ones((B, 4), dtype=torch.bool)
    tm = torch.ones((B, 8), dtype=torch.bool)
    odd = torch.zeros((B, 2, 5, 5, 3), dtype=torch.uint8)          # 75 bytes an image
    with pytest.raises(ValueError, match="multiple of 16"):
        model._check_pad_masks(sm, None, B, odd)
    assert model._check_pad_masks(None, tm, B, odd) is True       # no copy without a set mask
    big = torch.zeros((1, 2, 16, 16, 3), dtype=torch.uint8).expand(40000, 2, 16, 16, 3)
    with pytest.raises(ValueError, match="65535"):
        model._check_pad_masks(torch.ones((40000, 4), dtype=torch.bool), None, 40000, big)
    ok = torch.zeros((B, 2, 64, 64, 3), dtype=torch.uint8)
    assert model._check_pad_masks(sm, tm, B, ok) is True
    assert model._check_pad_masks(sm, None, B, ok.float()) is True


def test_masks_with_pruning_raise(no_library):
    m, _ = _model(compression="prune",
                  token_compression_sequence="[TaskDescriptionPrefix{0}] [Image{2};Image{2};Readout{0}]")
    with pytest.raises(ValueError, match="prune"):
        m._check_pad_masks(torch.ones((B, 4), dtype=torch.bool), None, B)
    with pytest.raises(ValueError, match="prune"):
        m._check_pad_masks(None, torch.ones((B, 8), dtype=torch.bool), B)
    assert m._check_pad_masks(None, None, B) is False


def test_text_mask_needs_an_uncompressed_text_set(no_library):
    from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O
    from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config
    plain = O.Octo(get_config("octo-tiny", num_blocks=2), torch.device("cpu"))
    assert plain.text_set == -1 and plain.n_sets == 2
    with pytest.raises(ValueError, match="no text set"):
        plain._check_pad_masks(None, torch.ones((B, 8), dtype=torch.bool), B)
    assert plain._check_pad_masks(torch.ones((B, 2), dtype=torch.bool), None, B) is True
    m, _ = _model(token_compression_sequence="[TaskDescriptionPrefix{1}] [Image{2};Image{2};Readout{0}]")
    with pytest.raises(ValueError, match="compressed"):
        m._check_pad_masks(None, torch.ones((B, 8), dtype=torch.bool), B)
    assert m._check_pad_masks(torch.ones((B, 4), dtype=torch.bool), None, B) is True


def test_ddp_step_checks_at_construction(model, no_library):
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    img = torch.zeros((B, 2, 64, 64, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="set_pad_mask"):
        DDPStep(model, None, None, img, None, set_pad_mask=torch.ones((B, 5), dtype=torch.bool))
    with pytest.raises(ValueError, match="text_pad_mask"):
        DDPStep(model, None, None, img, None, text_pad_mask=torch.ones((B, 8)))


def test_block_call_checks_its_masks(no_library):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import Encoder1DBlock
    from multi_modal_transformers_tokenmerge_amd.params import ParamStore
    blk = Encoder1DBlock.create(ParamStore(), "B", 128, 2, 256)
    table = K.SetTable([0, 8, 48], [8, 40, 4], [0b001, 0b011, 0b111])
    x = torch.zeros((2, 52, 128))
    for kw in (dict(set_pad_mask=torch.ones((2, 4), dtype=torch.bool)),
               dict(set_pad_mask=torch.ones((2, 3))),
               dict(text_pad_mask=torch.ones((2, 40), dtype=torch.bool)),
               dict(text_pad_mask=torch.ones((2, 8), dtype=torch.bool), text_set=3),
               dict(set_pad_mask=torch.ones((2, 3), dtype=torch.bool), readout_bits=0b1000)):
        with pytest.raises(ValueError, match="pad_mask"):
            blk(x, mask=table, train=False, **kw)


def test_wrappers_check_on_the_host(no_library):
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    with pytest.raises(ValueError):
        K.pad_mask_pack(torch.ones((B, 4), dtype=torch.bool))   # a host tensor
    with pytest.raises(ValueError):
        K.pad_mask_bias(B, 19, ([0, 5], [5, 14]), None, None)    # neither mask


# ---------------------------------------------------------------------- argument checks
PTR = 1 << 20          # non-null, 16-B aligned


def _arr(v):
    return (ctypes.c_int32 * len(v))(*v)


STARTS, LENS = [0, 5, 12, 15], [5, 7, 3, 4]


def _bias(lib, words=PTR, B=3, L=19, n=4, starts=STARTS, lens=LENS, text=None, text_set=0, T=0,
          kb=PTR, kb_s_b=64, acc=0):
    return lib.mmt_pad_mask_bias(words, B, L, n, starts and _arr(starts), lens and _arr(lens), text,
                                 text_set, T, kb, kb_s_b, acc, None)


def _rows(lib, which="fwd", words=PTR, B=3, L=19, D=8, n=4, starts=STARTS, lens=LENS, text=None,
          text_set=0, T=0, pe=PTR, x=PTR, xs_b=19 * 8, xs_t=8):
    s, ln = starts and _arr(starts), lens and _arr(lens)
    if which == "fwd":
        return lib.mmt_pad_mask_rows_fwd(words, B, L, D, n, s, ln, text, text_set, T, pe, x, xs_b,
                                         xs_t, None)
    return lib.mmt_pad_mask_rows_bwd(words, B, L, D, n, s, ln, text, text_set, T, x, xs_b, xs_t, None)


def _pack(lib, mask=PTR, B=3, n=4, readout=0b1000, words=PTR):
    return lib.mmt_pad_mask_pack(mask, B, n, readout, words, None)


def _images(lib, words=PTR, sets=(1, 2), n=4, B=3, I=2, nbytes=12288, src=PTR, dst=2 * PTR):
    return lib.mmt_pad_mask_images(words, sets and _arr(sets), n, B, I, nbytes, src, dst, None)


REJECTED = [
    ("images-null-words", "images", lambda l: _images(l, words=None)),
    ("images-null-sets", "images", lambda l: _images(l, sets=None)),
    ("images-null-src", "images", lambda l: _images(l, src=None)),
    ("images-null-dst", "images", lambda l: _images(l, dst=None)),
    ("images-in-place", "images", lambda l: _images(l, dst=PTR)),
    ("images-n-0", "images", lambda l: _images(l, n=0)),
    ("images-n-17", "images", lambda l: _images(l, n=17)),
    ("images-B-0", "images", lambda l: _images(l, B=0)),
    ("images-I-0", "images", lambda l: _images(l, I=0)),
    ("images-I-17", "images", lambda l: _images(l, I=17, sets=[1] * 17)),
    ("images-BI-large", "images", lambda l: _images(l, B=40000)),
    ("images-bytes-0", "images", lambda l: _images(l, nbytes=0)),
    ("images-bytes-not-16", "images", lambda l: _images(l, nbytes=12296)),
    ("images-src-unaligned", "images", lambda l: _images(l, src=PTR + 8)),
    ("images-dst-unaligned", "images", lambda l: _images(l, dst=2 * PTR + 4)),
    ("images-set-past", "images", lambda l: _images(l, sets=(1, 4))),
    ("images-set-neg", "images", lambda l: _images(l, sets=(-1, 2))),
    ("pack-null-mask", "pack", lambda l: _pack(l, mask=None)),
    ("pack-null-words", "pack", lambda l: _pack(l, words=None)),
    ("pack-B-0", "pack", lambda l: _pack(l, B=0)),
    ("pack-n-0", "pack", lambda l: _pack(l, n=0, readout=0)),
    ("pack-n-17", "pack", lambda l: _pack(l, n=17)),
    ("pack-readout-past-n", "pack", lambda l: _pack(l, readout=0b10000)),
    ("bias-null-kb", "bias", lambda l: _bias(l, kb=None)),
    ("bias-null-starts", "bias", lambda l: _bias(l, starts=None)),
    ("bias-null-lens", "bias", lambda l: _bias(l, lens=None)),
    ("bias-no-mask", "bias", lambda l: _bias(l, words=None)),
    ("bias-B-0", "bias", lambda l: _bias(l, B=0)),
    ("bias-L-0", "bias", lambda l: _bias(l, L=0)),
    ("bias-n-0", "bias", lambda l: _bias(l, n=0)),
    ("bias-n-17", "bias", lambda l: _bias(l, n=17, starts=list(range(17)), lens=[1] * 17, L=17)),
    ("bias-gap", "bias", lambda l: _bias(l, starts=[0, 6, 12, 15])),
    ("bias-overlap", "bias", lambda l: _bias(l, lens=[6, 7, 3, 4])),
    ("bias-short", "bias", lambda l: _bias(l, lens=[5, 7, 3, 3])),
    ("bias-long", "bias", lambda l: _bias(l, lens=[5, 7, 3, 5])),
    ("bias-neg-len", "bias", lambda l: _bias(l, lens=[5, 7, -3, 4])),
    ("bias-first-start", "bias", lambda l: _bias(l, starts=[1, 5, 12, 15])),
    ("bias-stride-short", "bias", lambda l: _bias(l, kb_s_b=60)),
    ("bias-stride-L", "bias", lambda l: _bias(l, kb_s_b=20)),
    ("bias-stride-not-4", "bias", lambda l: _bias(l, kb_s_b=66)),
    ("bias-kb-unaligned", "bias", lambda l: _bias(l, kb=PTR + 4)),
    ("bias-text-T", "bias", lambda l: _bias(l, text=PTR, T=7)),
    ("bias-text-T-of-other-set", "bias", lambda l: _bias(l, text=PTR, T=5, text_set=1)),
    ("bias-text-set-neg", "bias", lambda l: _bias(l, text=PTR, T=5, text_set=-1)),
    ("bias-text-set-past", "bias", lambda l: _bias(l, text=PTR, T=5, text_set=4)),
    ("rows_fwd-null-x0", "rows_fwd", lambda l: _rows(l, x=None)),
    ("rows_fwd-null-pe", "rows_fwd", lambda l: _rows(l, pe=None)),
    ("rows_fwd-no-mask", "rows_fwd", lambda l: _rows(l, words=None)),
    ("rows_fwd-D-6", "rows_fwd", lambda l: _rows(l, D=6, xs_t=8)),
    ("rows_fwd-D-0", "rows_fwd", lambda l: _rows(l, D=0)),
    ("rows_fwd-x0-unaligned", "rows_fwd", lambda l: _rows(l, x=PTR + 8)),
    ("rows_fwd-pe-unaligned", "rows_fwd", lambda l: _rows(l, pe=PTR + 4)),
    ("rows_fwd-xs_t-lt-D", "rows_fwd", lambda l: _rows(l, D=16, xs_t=8, xs_b=19 * 16)),
    ("rows_fwd-xs_t-not-4", "rows_fwd", lambda l: _rows(l, xs_t=10, xs_b=19 * 10 + 2)),
    ("rows_fwd-xs_b-not-4", "rows_fwd", lambda l: _rows(l, xs_b=19 * 8 + 2)),
    ("rows_fwd-xs_b-short", "rows_fwd", lambda l: _rows(l, xs_b=18 * 8)),
    ("rows_fwd-gap", "rows_fwd", lambda l: _rows(l, starts=[0, 6, 12, 15])),
    ("rows_fwd-n-17", "rows_fwd", lambda l: _rows(l, n=17)),
    ("rows_fwd-text-T", "rows_fwd", lambda l: _rows(l, text=PTR, T=8)),
    ("rows_bwd-null-dx0", "rows_bwd", lambda l: _rows(l, "bwd", x=None)),
    ("rows_bwd-no-mask", "rows_bwd", lambda l: _rows(l, "bwd", words=None)),
    ("rows_bwd-D-6", "rows_bwd", lambda l: _rows(l, "bwd", D=6)),
    ("rows_bwd-dx0-unaligned", "rows_bwd", lambda l: _rows(l, "bwd", x=PTR + 4)),
    ("rows_bwd-xs_t-lt-D", "rows_bwd", lambda l: _rows(l, "bwd", D=16, xs_t=8, xs_b=19 * 16)),
    ("rows_bwd-xs_b-not-4", "rows_bwd", lambda l: _rows(l, "bwd", xs_b=19 * 8 + 2)),
    ("rows_bwd-short-table", "rows_bwd", lambda l: _rows(l, "bwd", lens=[5, 7, 3, 3])),
    ("rows_bwd-text-set-past", "rows_bwd", lambda l: _rows(l, "bwd", text=PTR, T=5, text_set=9)),
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
    assert msg and f"mmt_pad_mask_{which}".encode() in msg, msg
