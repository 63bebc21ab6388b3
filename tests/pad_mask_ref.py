"""Restatement of the observation pad masks (include/mmt_api.h, "observation pad masks") in numpy
and float64 torch: which rows are masked, the packed words, the key-bias rows, the row overwrite
and zeroing, and attention with the mask bias. Shared by tests/test_pad_mask_*.py."""
import numpy as np
import torch

M = -1024.0  # MMT_PAD_MASK_LOGIT


def set_ids(starts, lens):
    """(L,) the set of every row of a sequence tiled by (starts, lens)."""
    sid = np.zeros(int(sum(lens)), np.int64)
    for k, (s, n) in enumerate(zip(starts, lens)):
        sid[s:s + n] = k
    return sid


def pack(set_mask, readout_bits=0):
    """(B,) uint32 present-bits of a bool (B, n_sets) mask; Readout sets are always present."""
    set_mask = np.asarray(set_mask, bool)
    w = (set_mask.astype(np.uint32) << np.arange(set_mask.shape[1], dtype=np.uint32)).sum(1)
    return (w | np.uint32(readout_bits)).astype(np.uint32)


def masked_rows(starts, lens, B, set_mask=None, text_mask=None, text_set=0, readout_bits=0):
    """(B, L) bool, True = masked: a row of a set flagged absent (set_mask (B, n_sets), True =
    present; Readout sets cannot be absent) or a padded token of set text_set (text_mask (B, T),
    True = real)."""
    sid = set_ids(starts, lens)
    out = np.zeros((B, sid.size), bool)
    if set_mask is not None:
        words = pack(set_mask, readout_bits)
        out |= ((words[:, None] >> sid[None, :].astype(np.uint32)) & 1) == 0
    if text_mask is not None:
        s0, T = starts[text_set], lens[text_set]
        assert np.asarray(text_mask).shape == (B, T)
        out[:, s0:s0 + T] |= ~np.asarray(text_mask, bool)
    return out


def bias_rows(masked, lp, base=None):
    """The key-bias rows (B, lp) fp32. base None (accumulate = 0): M on the masked entries, 0 on
    the others and on the padding. base given (accumulate = 1): base with one fp32 add of M on the
    masked entries, everything else as it was."""
    B, L = masked.shape
    if base is None:
        kb = np.zeros((B, lp), np.float32)
        kb[:, :L][masked] = np.float32(M)
        return kb
    kb = np.array(base, np.float32, copy=True)
    view = kb[:, :L]
    view[masked] = view[masked] + np.float32(M)
    return kb


def rows_fwd(x0, pe, masked):
    """x0 (B, L, D) with pe[l] written over the masked rows."""
    out = np.array(x0, copy=True)
    b, l = np.nonzero(masked)
    out[b, l] = pe[l]
    return out


def rows_bwd(dx0, masked):
    out = np.array(dx0, copy=True)
    out[masked] = 0
    return out


def dense_mask(starts, lens, vis):
    """(L, L) bool torch mask of a token-set table (query set s sees the key sets of vis[s])."""
    sid = torch.from_numpy(set_ids(starts, lens))
    v = torch.tensor(vis, dtype=torch.long)
    return ((v[sid][:, None] >> sid[None, :]) & 1).bool()


def masked_attention(qkv, H, scale, mask, key_bias=None, keep=None, keep_prob=1.0):
    """softmax(scale q.k + key_bias[b, k]) v in the dtype of qkv (float64 in the tests), the bias
    added in that dtype, then the set mask (finfo.min), as tests/test_prop_attn_block_gpu.py's
    biased_attention; keep (L, L) bool: attention dropout, kept weights / keep_prob.
    Returns (o (B, L, H Dh), lse (B, H, L))."""
    B, L, three = qkv.shape
    Dh = three // (3 * H)
    q, k, v = qkv.view(B, L, 3, H, Dh).unbind(2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    if key_bias is not None:
        s = s + key_bias[:, None, None, :L].to(s.dtype)
    s = torch.where(mask[None, None], s, torch.finfo(s.dtype).min)
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    if keep is not None:
        p = torch.where(keep[None, None], p / keep_prob, torch.zeros_like(p))
    return torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(B, L, H * Dh), lse
