"""CPU reference of the multi-draw diffusion loss (include/mmt_api.h mmt_diffusion_loss_multi and
mmt_diffusion_loss_dq), per sample b and draw k:

    noisy = sqrt(abar_t) a_b + sqrt(1 - abar_t) eps;   pre = W1x noisy + Q[t] + P[b]
    h = relu(pre);  pred = W2 h + b2;  d = pred - eps
    loss  = A / (K max(sum m, 1)) sum m 0.5 d^2
    dpred = grad_scale A / (K max(sum m, 1)) m d;  dh = (W2^T dpred) [pre > 0]
    dP[b] = sum_k dh[k, b];  dQ[t] = sum of the dh rows drawn at t

in float64 numpy, forward and every backward output, with an fp32 emulation (``dtype=np.float32``:
every operand, product and sum in fp32). ``head_grads`` continues the backward through the split
first Dense and the time encoder to every parameter of a DiffusionActionHead. The draws come from
``oracle.rng``. Also the synthetic inputs of the kernel-level tests, so the CPU and GPU tests see
the same arrays."""
from __future__ import annotations

import numpy as np

from oracle import rng as R
from oracle.sampler_ref import bf16


def loss_multi(actions, mask, alpha_hats, P, Q, w1x, w2, b2, t, eps, grad_scale: float = 1.0,
               dtype=np.float64) -> dict:
    """actions (B, A); mask (B, A) of 0 / 1 or None; alpha_hats (steps,); P (B, H); Q (steps, H);
    w1x (H, A) and w2 (A, H) bf16 values; b2 (A,); t (K, B) int; eps (K, B, A). Returns a dict of
    `dtype` arrays: loss (), noisy / dpred (K, B, A), pre / h / dh (K, B, H), dP (B, H),
    dQ (steps, H)."""
    f = lambda v: np.asarray(v, dtype=np.float64).astype(dtype)
    actions, P, Q, w1x, w2, b2, eps = f(actions), f(P), f(Q), f(bf16(w1x)), f(bf16(w2)), f(b2), f(eps)
    abar = f(alpha_hats)
    t = np.asarray(t).astype(np.int64)
    K, B = t.shape
    A = actions.shape[1]
    m = np.ones((B, A), dtype=dtype) if mask is None else f(np.asarray(mask) != 0)
    c1, c2 = np.sqrt(abar[t]), np.sqrt(dtype(1) - abar[t])               # (K, B)
    noisy = (c1[..., None] * actions[None] + c2[..., None] * eps).astype(dtype)
    pre = (noisy @ w1x.T + Q[t] + P[None]).astype(dtype)
    h = np.maximum(pre, dtype(0))
    d = (h @ w2.T + b2 - eps).astype(dtype)
    norm = dtype(A) / (dtype(K) * dtype(max(float(m.sum()), 1.0)))
    per_sample = (m[None] * dtype(0.5) * d * d).sum(axis=2).sum(axis=0)   # over a, then k: (B,)
    loss = dtype(0)
    for v in per_sample:                                                  # ascending b
        loss = dtype(loss + v)
    loss = dtype(loss * norm)
    dpred = (dtype(grad_scale) * norm * m[None] * d).astype(dtype)
    dh = ((dpred @ w2) * (pre > 0)).astype(dtype)
    return dict(loss=loss, noisy=noisy, pre=pre, h=h, dpred=dpred, dh=dh, dP=dh.sum(axis=0),
                dQ=segment_sum(t.reshape(-1), dh.reshape(K * B, -1), Q.shape[0]))


def segment_sum(t_rows, rows, steps: int) -> np.ndarray:
    """out[t] = sum of rows[r] with t_rows[r] == t, in ascending r."""
    rows = np.asarray(rows)
    out = np.zeros((steps, rows.shape[1]), dtype=rows.dtype)
    for r, t in enumerate(np.asarray(t_rows)):
        out[int(t)] += rows[r]
    return out


# ------------------------------------------------------------------------------- draws
def t_key(seed: int, step: int, k: int) -> int:
    """Key of draw k's diffusion step (include/mmt_api.h): k = 0 mmt_diffusion_prep's stream
    (layer 0xFFFE, site 1), k >= 1 site 2 k of layer 0xFFF9."""
    return R.stream_key(seed, step, 0xFFFE, 1) if k == 0 else R.stream_key(seed, step, 0xFFF9, 2 * k)


def eps_key(seed: int, step: int, k: int) -> int:
    return (R.stream_key(seed, step, 0xFFFE, 2) if k == 0
            else R.stream_key(seed, step, 0xFFF9, 2 * k + 1))


def draws(seed: int, step: int, B: int, A: int, steps: int, K: int, sample_offset: int = 0):
    """(t (K, B) int32: bit-exact; eps (K, B, A) float64 Box-Muller: the device's fp32 logf / cosf
    agree to a few ulp) at the global sample index g = sample_offset + b: t = (u32(g) * steps) >> 32,
    eps from counters 2 c, 2 c + 1 of c = g A + j."""
    g = np.arange(B, dtype=np.uint64) + np.uint64(sample_offset)
    c = (g[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]) & R.M32
    t = np.empty((K, B), dtype=np.int32)
    eps = np.empty((K, B, A), dtype=np.float64)
    for k in range(K):
        u = R.draw_u32(t_key(seed, step, k), g).astype(np.uint64)
        t[k] = ((u * np.uint64(steps)) >> np.uint64(32)).astype(np.int32)
        ke = eps_key(seed, step, k)
        u1 = ((R.draw_u32(ke, (np.uint64(2) * c) & R.M32) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (R.draw_u32(ke, (np.uint64(2) * c + np.uint64(1)) & R.M32) >> np.uint64(8)).astype(np.float64) / 16777216.0
        eps[k] = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return t, eps


# ------------------------------------------------------------------------------- the head
def head_grads(p: dict, e, actions, mask, alpha_hats, t, eps, A: int) -> dict:
    """Loss and every gradient of DiffusionActionHead.loss_forward_multi in float64 from the
    head's parameters p (the values its GEMMs read): fourier (F,), t1w / t2w (T, T), t1b / t2b
    (T,), w1 (H, A+T+D), b1 (H,), w2 (A, H), b2 (A,), all stored [out][in]; e (B, D) the pooled
    readout. Nothing in between is rounded. Returns loss, de and the gradients by the same names."""
    g = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    e = np.asarray(e, dtype=np.float64)
    S = len(alpha_hats)
    T = g["t1w"].shape[0]
    tt = 2.0 * np.pi * np.arange(S, dtype=np.float64)[:, None]
    ang = tt * g["fourier"].reshape(1, -1)
    feats = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)
    zt = feats @ g["t1w"].T + g["t1b"]
    ht = np.maximum(zt, 0.0)
    temb = ht @ g["t2w"].T + g["t2b"]
    w1x, w1t, w1r = g["w1"][:, :A], g["w1"][:, A:A + T], g["w1"][:, A + T:]
    Q = temb @ w1t.T + g["b1"]
    P = e @ w1r.T
    r = loss_multi(actions, mask, alpha_hats, P, Q, w1x, g["w2"], g["b2"], t, eps)
    KB = r["dh"].shape[0] * r["dh"].shape[1]
    dh, dpred = r["dh"].reshape(KB, -1), r["dpred"].reshape(KB, -1)
    dQ = r["dQ"]
    dtemb = dQ @ w1t
    dzt = (dtemb @ g["t2w"]) * (zt > 0)
    dfeats = dzt @ g["t1w"]
    F = ang.shape[1]
    dfour = (tt * (np.cos(ang) * dfeats[:, F:] - np.sin(ang) * dfeats[:, :F])).sum(axis=0)
    dw1 = np.concatenate([dh.T @ r["noisy"].reshape(KB, -1), dQ.T @ temb, r["dP"].T @ e], axis=1)
    return dict(loss=r["loss"], de=r["dP"] @ w1r, pre=r["pre"], w2=dpred.T @ r["h"].reshape(KB, -1),
                b2=dpred.sum(axis=0), w1=dw1, b1=dQ.sum(axis=0), t2w=dtemb.T @ ht,
                t2b=dtemb.sum(axis=0), t1w=dzt.T @ feats, t1b=dzt.sum(axis=0), fourier=dfour)


# ------------------------------------------------------------------------------- test inputs
# the kernel-level cases (H, A, B, steps, K) -> numpy seed. Each seed is the first for which no
# float64 pre-activation of the case (any mask) lies within PRE_MARGIN of zero, so the ReLU gate
# of the fp32 kernel cannot differ from the reference's (tests/test_diffusion_multi_cpu.py asserts
# the condition)
KERNEL_CASES = [(192, 8, 5, 7, 3), (200, 24, 33, 12, 2), (384, 40, 18, 12, 4), (1024, 64, 9, 5, 2),
                (64, 16, 4, 32, 1)]
PRE_MARGIN = 1e-4
KERNEL_SEEDS = {}   # filled below


def schedule(steps: int) -> np.ndarray:
    """A decreasing abar in (0, 1), fp32 (any schedule serves the kernel)."""
    return np.cos(np.linspace(0.05, 1.5, steps)).astype(np.float32) ** 2


def kernel_inputs(H: int, A: int, B: int, steps: int, K: int, seed: int | None = None) -> dict:
    """fp32 / bf16-valued arrays. W1 carries 8 columns past the A it is read at (a padded row
    stride, as the head's (H, A+T+D) kernel). mask: about 70 % ones."""
    seed = KERNEL_SEEDS[(H, A, B, steps, K)] if seed is None else seed
    g = np.random.default_rng(seed)
    r = lambda *s: g.standard_normal(s).astype(np.float32)
    return dict(P=0.5 * r(B, H), Q=0.5 * r(steps, H),
                w1=bf16(r(H, A + 8) / np.sqrt(A)).astype(np.float32),
                w2=bf16(0.5 * r(A, H) / np.sqrt(H)).astype(np.float32), b2=0.1 * r(A),
                actions=r(B, A), eps=r(K, B, A),
                t=g.integers(0, steps, size=(K, B)).astype(np.int32),
                mask=(g.random((B, A)) < 0.7).astype(np.uint8), alpha_hats=schedule(steps))


def masks(inp: dict) -> dict:
    """The mask variants of a case: none, ~70 % ones, the same with row 1 all zero, all zero."""
    row0 = inp["mask"].copy()
    row0[1] = 0
    return {"none": None, "random": inp["mask"], "zero-row": row0,
            "all-zero": np.zeros_like(inp["mask"])}


def min_abs_pre(inp: dict, A: int) -> float:
    r = loss_multi(inp["actions"], None, inp["alpha_hats"], inp["P"], inp["Q"], inp["w1"][:, :A],
                   inp["w2"], inp["b2"], inp["t"], inp["eps"])
    return float(np.abs(r["pre"]).min())


def find_seed(case, tries: int = 200) -> int:
    """The first numpy seed 1000 H + 10 A + B + 100000 i whose inputs keep every pre-activation
    PRE_MARGIN away from zero."""
    H, A, B, steps, K = case
    for i in range(tries):
        seed = 1000 * H + 10 * A + B + 100000 * i
        if min_abs_pre(kernel_inputs(H, A, B, steps, K, seed), A) >= PRE_MARGIN:
            return seed
    raise RuntimeError(f"no seed for {case}")


KERNEL_SEEDS.update({   # find_seed(case), recorded (1st, 1st, 2nd, 3rd and 1st candidate)
    (192, 8, 5, 7, 3): 192085, (200, 24, 33, 12, 2): 200273, (384, 40, 18, 12, 4): 484418,
    (1024, 64, 9, 5, 2): 1224649, (64, 16, 4, 32, 1): 64164})


def want(case, mask_name: str = "none", grad_scale: float = 1.0, dtype=np.float64) -> dict:
    H, A, B, steps, K = case
    inp = kernel_inputs(*case)
    return loss_multi(inp["actions"], masks(inp)[mask_name], inp["alpha_hats"], inp["P"], inp["Q"],
                      inp["w1"][:, :A], inp["w2"], inp["b2"], inp["t"], inp["eps"], grad_scale,
                      dtype)
