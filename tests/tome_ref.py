"""Shared reference helpers of the ToMe match contract tests (tests/test_tome_ties_cpu.py,
tests/test_tome_contract_gpu.py): the dispatch of mmt_tome_match restated in Python, metrics that
tie, and the conditions such a metric has to meet.

expected_route is written from the description of the forms in include/mmt_api.h
(MMT_TOME_ROUTE_*), not from the dispatcher's code: the LDS budgets are spelled out here as byte
counts of the arrays each kernel keeps (all within 160 KB).

tie_metric draws token rows from a codebook of K small-integer vectors. Equal rows give exactly
equal normalised rows, so equal scores: many a rows share their best score (ties in the rank, on
both sides of the r cut) and the first b row holding a code collects every a row of that code (a
fan-in far above 8). Integers in [-3, 3] are exact in bf16, so fp32 and bf16 runs share one
expected result. No two code vectors are parallel, so the best score of a row is well separated
from its second best distinct score and the first-index argmax does not hang on rounding."""
import numpy as np

LDS = 160 * 1024
FUSED, BIG_AG1, BIG_AG2, TILED_MFMA, TILED_VALU = 1, 2, 3, 4, 5   # MMT_TOME_ROUTE_* forms
NORM_SCALAR, IN_BF16 = 0x10000, 0x20000


def _pow2_at_least(v):
    p = 1
    while p < v:
        p *= 2
    return p


def _pad32(v):
    return (v + 31) // 32 * 32


def fused_lds(t, c):
    """Bytes of the one-launch kernel: both normalised halves, rows padded to 32 and c + 1 floats
    wide; a (max, idx) pair per (b tile, padded a row); max, idx and rank slot per a row."""
    ta, tb = (t + 1) // 2, t // 2
    pa, pb = _pad32(ta), _pad32(tb)
    return 4 * (pa + pb) * (c + 1) + (pb // 32) * pa * 8 + ta * 12


def score_big_lds(t, c, ag):
    """Bytes of the b-resident score kernel: the padded b half and ag 32-row a tiles, c + 1 floats
    wide, and a (max, idx) pair per (wave of 16, a row of 32)."""
    return 4 * ((_pad32(t // 2) + 32 * ag) * (c + 1) + 2 * 16 * 32)


def tiled_nbt(c):
    """b tiles per LDS group of the tiled score kernel: what fits beside one a tile and the
    (max, idx) partials of 8 slices x 32 rows, at most 4."""
    tile = 4 * 32 * (c + 1)
    return min(4, (LDS - tile - 4 * 8 * 32 * 2) // tile)


def expected_route(n, t, c, dtype, strides=None, base_align=0, use_mfma=True):
    """The MMT_TOME_ROUTE_* value mmt_tome_match must report for an (n, t, heads, c) metric of
    `dtype` (a torch dtype or its name) with element strides (s_n, s_t, s_h) (None: contiguous,
    one head), a base address of `base_align` modulo 16 bytes and the MFMA or VALU score path."""
    bf16 = "bfloat16" in str(dtype)
    per16 = 8 if bf16 else 4
    strides = (t * c, c, 0) if strides is None else strides
    vec = c % 8 == 0 and base_align % 16 == 0 and all(s % per16 == 0 for s in strides)
    lpr = _pow2_at_least(c // 8) if vec else 0
    flags = (0 if vec else NORM_SCALAR) | (IN_BF16 if bf16 else 0)
    if vec and use_mfma and fused_lds(t, c) <= LDS and c // 8 <= 64:
        return FUSED | lpr << 8 | flags
    if use_mfma and c % 4 == 0 and score_big_lds(t, c, 1) <= LDS:
        n_at = ((t + 1) // 2 + 31) // 32
        two = n * n_at > 256 and score_big_lds(t, c, 2) <= LDS
        return (BIG_AG2 if two else BIG_AG1) | lpr << 8 | flags
    form = TILED_MFMA if use_mfma and c % 2 == 0 else TILED_VALU
    return form | lpr << 8 | tiled_nbt(c) << 20 | flags


def form_boundaries(c, n_big2=512):
    """(last t on the fused form, last t on a b-resident form, last t on its two-tile form) for a
    contiguous fp32 metric of width c on the MFMA path, found by scanning expected_route."""
    form = lambda n, t: expected_route(n, t, c, "float32") & 0xff
    ts = range(2, 2049)
    return (max(t for t in ts if form(1, t) == FUSED),
            max(t for t in ts if form(1, t) in (BIG_AG1, BIG_AG2)),
            max(t for t in ts if form(n_big2, t) == BIG_AG2))


# ------------------------------------------------------------------ metrics that tie
def tie_params(t):
    """(K, seed) at which check_tie_properties holds for the shapes of the tests: 6 codes, but a
    fan-in of 9 among the r <= t / 2 src tokens of a small set needs fewer (found by running the
    oracle on seeds 0, 1, ...; the conditions themselves are never relaxed)."""
    return (2, 1) if t < 48 else (3, 0) if t < 128 else (6, 0)


def tie_metric(n, t, heads, c, K=None, seed=None):
    """(n, t, heads, c) fp32; K, seed default to tie_params(t).
    Every token's head sum is one of K integer code vectors (entries in
    [-3, 3], none all zero, no two parallel); head h holds the code's entries k with
    k % heads == h, so the sum over the heads is the code. Sample s with s % 3 == 1 has one zero a
    row (an even token, not token 0): exactly one NaN node_max. Sample s with s % 3 == 2 has one
    zero b row (an odd token, not token 1): every score against it is NaN, so every node_max of
    the sample is (a class-token flag turns a row 0 into -inf)."""
    K = tie_params(t)[0] if K is None else K
    seed = tie_params(t)[1] if seed is None else seed
    assert t >= 6 and c >= 2 and K >= 2
    rng = np.random.default_rng([seed, n, t, heads, c, K])
    while True:
        code = rng.integers(-3, 4, (K, c)).astype(np.float64)
        nrm = np.sqrt((code * code).sum(1))
        if (nrm == 0).any():
            continue
        cos = (code @ code.T) / np.outer(nrm, nrm)
        np.fill_diagonal(cos, 0.0)
        if np.abs(cos).max() < 0.95:    # no two codes (anti)parallel or nearly so
            break
    pick = rng.integers(0, K, (n, t))
    tok = code[pick].astype(np.float32)                      # (n, t, c)
    mask = (np.arange(c)[None, :] % heads) == np.arange(heads)[:, None]   # (heads, c)
    m = tok[:, :, None, :] * mask[None, None].astype(np.float32)
    ta, tb = (t + 1) // 2, t // 2
    for s in range(n):
        if s % 3 == 1:
            m[s, 2 * int(rng.integers(1, ta))] = 0.0
        elif s % 3 == 2:
            m[s, 2 * int(rng.integers(1, tb)) + 1] = 0.0
    return np.ascontiguousarray(m)


def sort_key(v):
    """The total order of the rank (lax.sort on floats) as uint32 keys: NaN largest, -0 < +0."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    b = v.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where(np.isnan(v), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def check_tie_properties(nmax, dst, r):
    """The oracle's node_max (n, ta) and dst (n, r) of a tie_metric input do what the input is
    for: in sample 0 the keys on both sides of the r cut are equal and some dst has a fan-in of at
    least 9; sample 1 has exactly one NaN; sample 2 is NaN in every row past row 0."""
    n, ta = nmax.shape
    if r < ta:
        keys = np.sort(sort_key(nmax[0]))[::-1]
        assert keys[r - 1] == keys[r], "no tie across the r cut in sample 0"
    else:
        assert len(np.unique(sort_key(nmax[0]))) < ta, "no tie in sample 0"
    fan = np.bincount(dst[0]).max()
    assert fan >= 9, f"largest fan-in of sample 0 is {fan}"
    if n > 1:
        assert np.isnan(nmax[1]).sum() == 1, "sample 1 must hold exactly one NaN node_max"
    if n > 2:
        assert np.isnan(nmax[2][1:]).all(), "sample 2 must be NaN throughout"


def f64_first_argmax(metric):
    """(n, t, heads, c) -> (n, ta) first-index argmax over the b half of the cosine scores, NaN
    counting as the maximum (the first NaN wins), in float64. Equal token rows give exactly equal
    scores: each score is looked up in a table over the sample's distinct rows."""
    m = np.asarray(metric, dtype=np.float64).sum(2)
    out = []
    for s in range(m.shape[0]):
        rows, inv = np.unique(m[s], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            unit = rows / np.sqrt((rows * rows).sum(1))[:, None]
            table = np.array([[float(np.dot(unit[i], unit[j])) for j in range(len(rows))]
                              for i in range(len(rows))])
        scores = table[inv[0::2]][:, inv[1::2]]
        out.append(np.argmax(scores, axis=1))     # numpy: the first NaN, else the first maximum
    return np.stack(out).astype(np.int32)
