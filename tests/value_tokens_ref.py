"""numpy restatement of the value tokens (include/mmt_api.h "value tokens"; the one formula cited
from the reference is mu_law_encoder, tokenizers/numeric_values/value_tokenizer.py:33-34:
``sign(x) * log(1 + mu |x|) / log(1 + mu)``). Everything is fp32 unless it says float64.

    s = min(max(v, -1), 1)                          # NaN -> -1 (IEEE fmax / fmin)
    y = s | copysign(log1p(mu |s|) / log1p(mu), s)  # "uniform" | "mu_law"
    token = min(N - 1, floor((y + 1) * 0.5 * N))
    x0[b, rows[j]] = table[token[b, j]] + pe[rows[j]]
    dtable[k] += sum over (b, j) ascending with token == k of dx0[b, rows[j]]   (one accumulator)
"""
import numpy as np

F = np.float32
ENCODINGS = ("mu_law", "uniform")
FIXED_POINTS = np.array([-1.0, 0.0, 1.0, np.inf, -np.inf, np.nan, 1.5, -7.0], F)


def fixed_point_tokens(N):
    """The tokens of FIXED_POINTS for N bins, either encoding."""
    return np.array([0, N // 2, N - 1, N - 1, 0, 0, N - 1, 0], np.int32)


def mu_law(x, mu):
    """The reference's mu_law_encoder in float64 (the formula itself, for the helper's test)."""
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.log(1 + mu * np.abs(x)) / np.log(1 + mu)


def tokens(values, num_bins, mu=255.0, encoding="mu_law"):
    v = np.asarray(values, F)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(v), F(-1), np.minimum(np.maximum(v, F(-1)), F(1))).astype(F)
    y = s
    if encoding == "mu_law":
        mag = np.log1p(F(mu) * np.abs(s), dtype=F) / np.log1p(F(mu), dtype=F)
        y = np.copysign(mag.astype(F), s)
    elif encoding != "uniform":
        raise ValueError(encoding)
    t = np.floor((y + F(1)) * F(0.5) * F(num_bins)).astype(np.int64)
    return np.minimum(num_bins - 1, t).astype(np.int32)


def bin_centre_values(tok, num_bins, mu, encoding, rng):
    """fp32 values whose token is tok, away from every bin edge: y = (2k+1)/N - 1 + d 2/N with d
    uniform in [-0.25, 0.25], the encoding inverted in float64, cast to fp32."""
    tok = np.asarray(tok)
    d = rng.uniform(-0.25, 0.25, tok.shape)
    y = (2.0 * tok + 1.0) / num_bins - 1.0 + d * 2.0 / num_bins
    if encoding == "mu_law":
        s = np.sign(y) * ((1.0 + mu) ** np.abs(y) - 1.0) / mu
    else:
        s = y
    return s.astype(F)


def forward_rows(tok, table, pe, rows):
    """(B, n, D) fp32: table[tok] + pe[rows], one fp32 add."""
    return (table[tok].astype(F) + pe[np.asarray(rows)][None].astype(F)).astype(F)


def table_grad(dx0, tok, rows, num_bins, init=None):
    """The sequential fp32 sum in ascending (b, j) order, one accumulator per entry, added once
    to the buffer (init, zeros by default). Tokens outside [0, num_bins) are skipped."""
    B, n = tok.shape
    D = dx0.shape[-1]
    acc = np.zeros((num_bins, D), F)
    for b in range(B):
        for j in range(n):
            k = int(tok[b, j])
            if 0 <= k < num_bins:
                acc[k] = acc[k] + dx0[b, rows[j]].astype(F)
    base = np.zeros((num_bins, D), F) if init is None else np.asarray(init, F)
    return (base + acc).astype(F)
