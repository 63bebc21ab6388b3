"""CPU reference of the chunked continuous / categorical heads (include/mmt_api.h
mmt_head_continuous, mmt_head_categorical, mmt_head_categorical_decode) in float64 numpy:

    continuous:  p = tanh(z / M) M;  e = (p - y)^2 | |p - y|
                 loss = A / max(sum m, 1) sum m e;  dz = A / max(sum m, 1) m e'(p - y) (1 - tanh^2)
    categorical: bin = #edges <= y;  label = one_hot(bin, N) (zero for bin >= N)
                 loss = sum m ce / max(sum m, 1);  dz = m (has softmax - label) / max(sum m, 1)
    decode:      argmax (first index on ties), or the smallest c with CDF(c) > u of softmax(z / T)

For h = 1, no mask and the squared error the general forms equal oracle/heads_ref.py's, which the
CPU test asserts; the labels are its digitize_bins. The decode's uniform draws are restated bit
for bit from oracle/rng.py. Also the synthetic inputs of the GPU tests."""
from __future__ import annotations

import numpy as np

from oracle import heads_ref as HR
from oracle import rng as R

DECODE_LAYER, DECODE_SITE = 0xFFF8, 1


# ------------------------------------------------------------------------------- losses
def _mask(mask, shape):
    return np.ones(shape) if mask is None else (np.asarray(mask) != 0).astype(np.float64).reshape(shape)


def continuous(z, y, mask, h: int, A: int, loss: str = "mse", max_action: float = 5.0):
    """z, y (B, h A); mask (B, h A) of 0 / 1 or None. Returns (pred (B, h, A), loss, dz (B, h A))."""
    z = np.asarray(z, np.float64)
    B = z.shape[0]
    assert z.shape == (B, h * A)
    m = _mask(mask, z.shape)
    t = np.tanh(z / max_action)
    p = t * max_action
    d = p - np.asarray(y, np.float64)
    if loss == "mse":
        e, de = d * d, 2.0 * d
    elif loss == "l1":
        e, de = np.abs(d), np.sign(d)
    else:
        raise ValueError(loss)
    norm = A / max(m.sum(), 1.0)
    return p.reshape(B, h, A), norm * (m * e).sum(), norm * m * de * (1.0 - t * t)


def labels(y, max_action: float, N: int):
    """bin = #edges <= y against assign_bins' float32 edges (oracle/heads_ref.digitize_bins)."""
    return HR.digitize_bins(y, max_action, N)


def categorical(z, y, mask, h: int, A: int, max_action: float = 5.0):
    """z (B, h A, N) logits; y (B, h A); mask (B, h A) of 0 / 1 or None. Returns (loss,
    dz (B, h A, N), cls (B, h A) int: the first argmax)."""
    z = np.asarray(z, np.float64)
    B, G, N = z.shape
    assert G == h * A
    cls = z.argmax(axis=-1)       # numpy: the first index on ties, as jnp.argmax
    m = _mask(mask, (B, G))
    bins = labels(y, max_action, N).reshape(B, G)
    lab = np.zeros_like(z)
    bi, gi = np.nonzero(bins < N)
    lab[bi, gi, bins[bi, gi]] = 1.0
    mx = z.max(axis=-1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(axis=-1, keepdims=True))
    ce = -(lab * (z - lse)).sum(-1)
    norm = 1.0 / max(m.sum(), 1.0)
    dz = m[..., None] * (lab.sum(-1, keepdims=True) * np.exp(z - lse) - lab) * norm
    return norm * (m * ce).sum(), dz, cls


# ------------------------------------------------------------------------------- decode
def decode_u(seed: int, step: int, rows: int, G: int, sample_offset: int = 0) -> np.ndarray:
    """The uniform of every row r = b G + g, float32, bit for bit the kernel's: key
    stream_key(seed, step, 0xFFF8, 1), counter (sample_offset + b) G + g,
    u = ((draw >> 8) + 0.5) / 2^24 evaluated in fp32 (the sum rounds to even from 2^23 on)."""
    ctr = (np.uint64(sample_offset) * np.uint64(G) + np.arange(rows, dtype=np.uint64)) & R.M32
    d = R.draw_u32(R.stream_key(seed, step, DECODE_LAYER, DECODE_SITE), ctr) >> np.uint64(8)
    return (d.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def cdf(z, T: float) -> np.ndarray:
    """Float64 CDF of softmax(z / T) along the last axis."""
    z = np.asarray(z, np.float64) / T
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return np.cumsum(e, axis=-1) / e.sum(axis=-1, keepdims=True)


def decode(z, values, u=None, T: float = 1.0):
    """z (R, N); values (N,); u (R,) or None (argmax). Returns (cls (R,), actions (R,)): the
    smallest c with CDF(c) > u, N - 1 if there is none."""
    z = np.asarray(z, np.float64)
    if u is None:
        cls = z.argmax(axis=-1)
    else:
        c = cdf(z, T)
        cls = np.minimum((c <= np.asarray(u, np.float64)[:, None]).sum(axis=-1), z.shape[1] - 1)
    return cls, np.asarray(values)[cls]


# ------------------------------------------------------------------------------- test inputs
# (B, h, A) / (B, h, A, N): the smallest shapes at which each loop and tail of the kernels can
# fail: W = 7 (lanes past the row), 24, 72 (a second trip of the lane loop), B no multiple of the
# 4 rows of a workgroup; N = 32 (lanes without a class), 256, 100 (a ragged last run of the
# decode's ceil(N / 64) = 2 classes per lane), 1024 (the limit, 16 classes per lane)
CONT_CASES = [(1, 1, 7), (5, 3, 8), (6, 9, 8)]
CAT_CASES = [(3, 2, 3, 32), (2, 1, 8, 256), (3, 2, 2, 100), (1, 1, 2, 1024)]
MASKS = ("none", "random", "zero-row", "all-zero")
MAX_ACTION = 5.0
L1_MARGIN = 1e-3


def masks(mask: np.ndarray) -> dict:
    """The mask variants of tests/diffusion_multi_ref.masks: none, ~70 % ones, the same with one
    sample all zero (the last: B = 1 has no row 1), all zero."""
    row0 = mask.copy()
    row0[-1] = 0
    return {"none": None, "random": mask, "zero-row": row0, "all-zero": np.zeros_like(mask)}


def cont_inputs(B: int, h: int, A: int) -> dict:
    """z (fp32 pre-activations up to the tanh's flat part), y with the targets -5, 5, 4.99 of
    tests/test_heads_gpu.py in row 0, moved where needed so that |p - y| >= L1_MARGIN in float64
    everywhere (the sign of the L1 gradient is then no rounding question), mask ~70 % ones."""
    g = np.random.default_rng(1000 * B + 10 * h + A)
    W = h * A
    z = (g.standard_normal((B, W)) * 6).astype(np.float32)
    y = (g.standard_normal((B, W)) * 2).astype(np.float32)
    y[0, :3] = [-5.0, 5.0, 4.99]
    p = np.tanh(z.astype(np.float64) / MAX_ACTION) * MAX_ACTION
    near = np.abs(p - y) < 2 * L1_MARGIN
    y = np.where(near, (p + 0.5).astype(np.float32), y)
    return dict(z=z, y=y, mask=(g.random((B, W)) < 0.7).astype(np.uint8))


def cat_inputs(B: int, h: int, A: int, N: int) -> dict:
    """Logits with deliberate exact ties of the maximum (row 0: classes 3 and N - 2; row 1: the
    last two classes; row 2: all classes equal), targets over [-6, 6) with -5, 5, 4.99 first."""
    g = np.random.default_rng(100000 * B + 10000 * h + 1000 * A + N)
    G = h * A
    z = (g.standard_normal((B, G, N)) * 3).astype(np.float32)
    zf = z.reshape(B * G, N)
    top = np.float32(np.abs(zf).max() + 1)
    zf[0, [3, N - 2]] = top
    zf[1, [N - 2, N - 1]] = top
    if B * G > 2:
        zf[2, :] = np.float32(0.25)
    y = (g.random((B, G)) * 12 - 6).astype(np.float32)
    yf = y.reshape(-1)
    n = min(3, yf.size)
    yf[:n] = [-5.0, 5.0, 4.99][:n]
    return dict(z=z, y=y, mask=(g.random((B, G)) < 0.7).astype(np.uint8))
