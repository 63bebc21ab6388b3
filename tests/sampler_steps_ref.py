"""CPU reference of the step-table sampler (include/mmt_api.h mmt_diffusion_sample_steps):

    x <- clip(a_k x + b_k eps_hat(x, t_k) + c_k n_k, -clip, +clip),      k = 0 .. K-1
    eps_hat = W2 relu(W1x x + Q[t_k] + P[b]) + b2,        x_0 = z,  n_k = z (frozen) or noise[k]

in float64 numpy, with the two rounding models of the device forms (``stored_bf16``: x and the
hidden layer rounded to bf16 where the per-step launch form stores them) and an fp32 emulation
(``dtype=np.float32``: every operand and product in fp32). The DDPM and DDIM tables are restated
here from the formulas, independently of DiffusionActionHead.sampler_table. Also the synthetic
inputs of the kernel-level tests, so the CPU and GPU tests see the same arrays."""
from __future__ import annotations

import numpy as np

from oracle.sampler_ref import bf16


# ------------------------------------------------------------------------------- tables
def ddpm_table(betas, alpha_hats, final_noise: bool = True):
    """Rows t = S-1 .. 0: a = 1/sqrt(alpha_t), b = -a (1 - alpha_t) / sqrt(1 - abar_t),
    c = sqrt(beta_t); c = 0 on the t = 0 row unless final_noise. -> (t int32 (S,), coef (S, 3))."""
    beta = np.asarray(betas, dtype=np.float64)
    abar = np.asarray(alpha_hats, dtype=np.float64)
    S = beta.shape[0]
    t = np.arange(S - 1, -1, -1)
    alpha = 1.0 - beta[t]
    a = 1.0 / np.sqrt(alpha)
    b = -a * (1.0 - alpha) / np.sqrt(1.0 - abar[t])
    c = np.sqrt(beta[t])
    if not final_noise:
        c = np.where(t == 0, 0.0, c)
    return t.astype(np.int32), np.stack([a, b, c], axis=1).astype(np.float32)


def ddim_times(S: int, K: int) -> np.ndarray:
    """K evenly spread steps from S-1 down to 0 (rounded to nearest)."""
    if not 1 <= K <= S:
        raise ValueError(f"DDIM needs 1 <= steps <= {S}, got {K}")
    if K == 1:
        return np.array([S - 1], dtype=np.int32)
    return np.array([((S - 1) * (K - 1 - k) + (K - 1) // 2) // (K - 1) for k in range(K)],
                    dtype=np.int32)


def ddim_abar_prev(alpha_hats, t: np.ndarray) -> np.ndarray:
    """abar of the step each row lands on: the next row's, 1 after the last."""
    abar = np.asarray(alpha_hats, dtype=np.float64)
    return np.concatenate([abar[t[1:]], [1.0]])


def ddim_table(alpha_hats, K: int):
    """eta = 0: x <- sqrt(abar_prev) x0_hat + sqrt(1 - abar_prev) eps_hat with
    x0_hat = (x - sqrt(1 - abar_t) eps_hat) / sqrt(abar_t), as a (a, b, 0) row."""
    abar = np.asarray(alpha_hats, dtype=np.float64)
    t = ddim_times(abar.shape[0], K)
    at, ap = abar[t], ddim_abar_prev(abar, t)
    a = np.sqrt(ap / at)
    b = np.sqrt(1.0 - ap) - np.sqrt(ap * (1.0 - at) / at)
    return t, np.stack([a, b, np.zeros_like(a)], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------- the update
def run_steps(P, Q, w1x, w2, b2, step_t, coef, clip, z, noise=None, stored_bf16: bool = False,
              dtype=np.float64) -> np.ndarray:
    """P (B, H); Q (q_rows, H); w1x (H, A) and w2 (A, H) bf16 values; b2 (A,); step_t (K,);
    coef (K, 3) = a, b, c; z (B, A) the initial sample; noise None (n_k = z) or (K, B, A).
    Returns x after the K steps (B, A) in `dtype`."""
    f = lambda v: np.asarray(v, dtype=np.float64).astype(dtype)
    P, Q, w1x, w2, b2, z = f(P), f(Q), f(bf16(w1x)), f(bf16(w2)), f(b2), f(z)
    coef = f(coef)
    clip = dtype(clip)
    x = z.copy()
    for k, t in enumerate(np.asarray(step_t)):
        n = z if noise is None else f(noise[k])
        xin = f(bf16(x)) if stored_bf16 else x
        h = np.maximum(xin @ w1x.T + Q[int(t)][None, :] + P, dtype(0))
        if stored_bf16:
            h = f(bf16(h))
        eps = h @ w2.T + b2
        x = np.clip(coef[k, 0] * x + coef[k, 1] * eps + coef[k, 2] * n, -clip, clip).astype(dtype)
    return x


def split_first_dense(readout_mean, temb, w1, b1, A: int):
    """The denoiser's first Dense on concatenate([noisy, time_emb, readout]) split along its input
    (oracle.sampler_ref.predict_action): -> P (B, H), Q (steps, H), W1x (H, A), all float64."""
    temb = np.asarray(temb, dtype=np.float64)
    T = temb.shape[1]
    w1 = bf16(w1)
    P = bf16(readout_mean) @ w1[:, A + T:].T
    Q = temb @ w1[:, A:A + T].T + np.asarray(b1, np.float64)
    return P, Q, w1[:, :A]


# ------------------------------------------------------------------------------- draws
def step_noise_key(seed: int, step: int, k: int) -> int:
    """Key of step k's noise stream (include/mmt_api.h): site 16 + k % 240 of layer
    0xFFFE - k // 240."""
    from oracle import rng as R
    return R.stream_key(seed, step, 0xFFFE - k // 240, 16 + k % 240)


def normal_draws(key: int, B: int, A: int, sample_offset: int = 0) -> np.ndarray:
    """Box-Muller on the counter stream `key` at counters g A + a, g = sample_offset + b, in
    float64 (B, A): the device's fp32 logf / cosf agree to a few ulp, not bitwise."""
    from oracle import rng as R
    ctr = ((sample_offset + np.arange(B))[:, None] * A + np.arange(A)[None, :]).astype(np.uint64)
    u1 = ((R.draw_u32(key, 2 * ctr) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (R.draw_u32(key, 2 * ctr + np.uint64(1)) >> np.uint64(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# ------------------------------------------------------------------------------- test inputs
# the kernel-level cases (H, A, B, q_rows) and their mild table
KERNEL_CASES = [(192, 8, 5, 7), (200, 24, 33, 12), (384, 40, 70, 12), (1024, 64, 9, 5)]
KERNEL_K = 12
# at clip = 5 / 0.75 at most this share of the reference outputs may sit at +-clip
SATURATION_CAP = {5.0: 0.02, 0.75: 0.65}


def kernel_table(q_rows: int, K: int = KERNEL_K):
    t = np.array([(5 * k + 3) % q_rows for k in range(K)], dtype=np.int32)
    coef = np.tile(np.array([0.95, -0.2, 0.1], dtype=np.float32), (K, 1))
    return t, coef


def kernel_inputs(H: int, A: int, B: int, q_rows: int, K: int = KERNEL_K) -> dict:
    """fp32 / bf16-valued arrays from a numpy seed that depends on the shape alone. W1 carries 8
    columns past the A it is read at (a padded row stride, as the head's (H, A+T+D) kernel). W2 is
    scaled so that the update's Jacobian 0.95 I - 0.2 W2 diag(h > 0) W1x stays near the unit disk
    (its random part has spectral radius ~ 0.07): x does not run into clip = 5 over the K steps."""
    g = np.random.default_rng(1000 * H + 10 * A + B)
    r = lambda *s: g.standard_normal(s).astype(np.float32)
    return dict(P=0.5 * r(B, H), Q=0.5 * r(q_rows, H),
                w1=bf16(r(H, A + 8) / np.sqrt(A)).astype(np.float32),
                w2=bf16(0.5 * r(A, H) / np.sqrt(H)).astype(np.float32), b2=0.1 * r(A),
                z=r(B, A), noise=r(K, B, A))


def saturated(want: np.ndarray, clip: float) -> np.ndarray:
    return np.abs(want) >= clip
