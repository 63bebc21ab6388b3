"""numpy restatement of the point-cloud tokenizer (csrc/pointcloud.hip, include/mmt_api.h
"point-cloud tokens"): the indices in float32 arithmetic that mirrors the kernel's individually
rounded operations bit for bit, the embedding forward and backward in float64. Test
infrastructure only.

Error bounds. An fp32 sum of N products in any order (FMA or not) differs from the exact sum by at
most gamma_{N+1} * sum|terms| with gamma_m ~ m * 2^-24. A term that is itself the result of such a
sum carries that sum's error, relative to ITS sum of magnitudes, so the magnitudes are propagated:
every function below returns next to a value v the magnitude A(v) >= |v| obtained by running the
same formula on absolute values (the max over neighbours takes the max of the magnitudes). With
magnitudes propagated, a chain of up to three inherited sums and the own one is covered by

    |got - ref64| <= 4 * (N + 2) * 2^-24 * A

when N is the largest number of products summed along the chain (own sum included). N is stated
per tensor in `bounds`.
"""
from __future__ import annotations

import numpy as np

from oracle import rng as R

f32 = np.float32
U = 2.0 ** -24
FPS_LAYER, FPS_SITE = 0xFFF7, 1


# --------------------------------------------------------------------------------- indices
def dist3(xyz: np.ndarray, c: np.ndarray) -> np.ndarray:
    """d(p, c) = (dx dx + dy dy) + dz dz, each operation rounded to float32."""
    xyz = np.asarray(xyz, f32)
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        dx, dy, dz = xyz[..., 0] - c[0], xyz[..., 1] - c[1], xyz[..., 2] - c[2]
        return ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)


def fps(points: np.ndarray, n: int, start: int = 0) -> np.ndarray:
    """Farthest-point sampling of one cloud (P, C): dist = +inf, ids[0] = start, then n - 1 times
    dist = min(dist, d(., last)), sampled points count as -inf, arg-max with the lowest index."""
    xyz = np.asarray(points, f32)[:, :3]
    P = xyz.shape[0]
    dist = np.full(P, np.inf, f32)
    taken = np.zeros(P, bool)
    ids = np.zeros(n, np.int32)
    ids[0] = start
    for i in range(1, n):
        last = ids[i - 1]
        taken[last] = True
        dist = np.minimum(dist, dist3(xyz, xyz[last]))
        ids[i] = int(np.argmax(np.where(taken, -np.inf, dist)))   # first maximum
    return ids


def knn(points: np.ndarray, centroid: int, k: int) -> np.ndarray:
    """The k points of smallest d to point `centroid`, ascending by (d, index)."""
    xyz = np.asarray(points, f32)[:, :3]
    d = dist3(xyz, xyz[centroid])
    return np.lexsort((np.arange(xyz.shape[0]), d))[:k].astype(np.int32)


def sample_group(points: np.ndarray, n: int, k: int, start=None):
    """points (B, S, P, C) -> centroid_idx (B, S, n), neighbour_idx (B, S, n, k); start (B, S) or
    None (0)."""
    B, S = points.shape[:2]
    cidx = np.zeros((B, S, n), np.int32)
    nidx = np.zeros((B, S, n, k), np.int32)
    for b in range(B):
        for s in range(S):
            st = 0 if start is None else int(start[b, s])
            cidx[b, s] = fps(points[b, s], n, st)
            for m in range(n):
                nidx[b, s, m] = knn(points[b, s], cidx[b, s, m], k)
    return cidx, nidx


def drawn_start(seed: int, step: int, B: int, S: int, P: int, sample_offset: int = 0) -> np.ndarray:
    """The train-mode first centroids: (draw_u32(stream_key(seed, step, 0xFFF7, 1), g) * P) >> 32
    with g = (sample_offset + b) * S + s."""
    key = R.stream_key(seed, step, FPS_LAYER, FPS_SITE)
    g = (np.arange(B, dtype=np.uint64)[:, None] + np.uint64(sample_offset)) * np.uint64(S) + \
        np.arange(S, dtype=np.uint64)[None, :]
    u = R.draw_u32(key, g & R.M32).astype(np.uint64)
    return ((u * np.uint64(P)) >> np.uint64(32)).astype(np.int32)


# --------------------------------------------------------------------------------- embedding
def features(points: np.ndarray, cidx: np.ndarray, nidx: np.ndarray) -> np.ndarray:
    """(B, S, n, k, 2C) float32: [points[j] - points[c], points[j]], the subtraction in float32."""
    pts = np.asarray(points, f32)
    B, S = pts.shape[:2]
    bi = np.arange(B)[:, None, None, None]
    si = np.arange(S)[None, :, None, None]
    nb = pts[bi, si, nidx]                                        # (B, S, n, k, C)
    ce = pts[bi[..., 0], si[..., 0], cidx][:, :, :, None, :]      # (B, S, n, 1, C)
    return np.concatenate([(nb - ce).astype(f32), nb], axis=-1)


def init_params(rng: np.random.Generator, C: int, F1: int, F2: int, D: int) -> dict:
    """Random float32 parameters with non-zero biases (a test's, not the module's initialiser)."""
    def w(i, o):
        return (rng.standard_normal((i, o)) / np.sqrt(i)).astype(f32)
    return dict(w1=w(2 * C, F1), b1=(0.1 * rng.standard_normal(F1)).astype(f32), w2=w(F1, F2),
                b2=(0.1 * rng.standard_normal(F2)).astype(f32), w_out=w(F2, D),
                b_out=(0.1 * rng.standard_normal(D)).astype(f32))


def embed_fwd(feat: np.ndarray, p: dict, argmax=None) -> dict:
    """float64 forward of feat (..., k, 2C). Returns z1, z2 (pre-activations), h1, h2, g, argmax
    (the first neighbour attaining the maximum, or the one given), out (..., D) and the
    magnitudes A1, A2, Ag, Aout."""
    f = feat.astype(np.float64)
    w1, b1, w2, b2, wo, bo = (p[k].astype(np.float64) for k in
                              ("w1", "b1", "w2", "b2", "w_out", "b_out"))
    z1 = f @ w1 + b1
    h1 = np.maximum(z1, 0)
    z2 = h1 @ w2 + b2
    h2 = np.maximum(z2, 0)
    am = np.argmax(h2, axis=-2) if argmax is None else np.asarray(argmax, np.int64)
    g = np.take_along_axis(h2, am[..., None, :], axis=-2)[..., 0, :]
    out = g @ wo + bo
    A1 = np.abs(f) @ np.abs(w1) + np.abs(b1)
    A2 = A1 @ np.abs(w2) + np.abs(b2)
    Ag = A2.max(axis=-2)
    Aout = Ag @ np.abs(wo) + np.abs(bo)
    return dict(z1=z1, z2=z2, h1=h1, h2=h2, g=g, argmax=am, out=out, A1=A1, A2=A2, Ag=Ag,
                Aout=Aout)


def embed_bwd(feat: np.ndarray, p: dict, dy: np.ndarray, argmax: np.ndarray):
    """float64 gradients of the six parameter tensors for dy (..., D), the max routed to `argmax`
    (..., F2), relu'(0) = 0. Returns (grads, mags): dicts keyed w1, b1, w2, b2, w_out, b_out."""
    fw = embed_fwd(feat, p, argmax)
    k = feat.shape[-2]
    f = feat.astype(np.float64).reshape(-1, k, feat.shape[-1])          # (T, k, 2C)
    T = f.shape[0]
    dy = dy.astype(np.float64).reshape(T, -1)
    w2, wo = p["w2"].astype(np.float64), p["w_out"].astype(np.float64)
    am = np.asarray(argmax, np.int64).reshape(T, -1)                     # (T, F2)
    h1 = fw["h1"].reshape(T, k, -1)
    A1 = fw["A1"].reshape(T, k, -1)
    g, Ag = fw["g"].reshape(T, -1), fw["Ag"].reshape(T, -1)
    ady = np.abs(dy)
    dg, Adg = dy @ wo.T, ady @ np.abs(wo).T
    live = g > 0
    dz2, Adz2 = np.where(live, dg, 0.0), np.where(live, Adg, 0.0)
    onehot = (am[:, None, :] == np.arange(k)[None, :, None])            # (T, k, F2)
    dh2, Adh2 = onehot * dz2[:, None, :], onehot * Adz2[:, None, :]
    dh1, Adh1 = dh2 @ w2.T, Adh2 @ np.abs(w2).T                          # (T, k, F1)
    m1 = h1 > 0
    dz1, Adz1 = np.where(m1, dh1, 0.0), np.where(m1, Adh1, 0.0)
    grads = dict(w_out=g.T @ dy, b_out=dy.sum(0),
                 w2=np.einsum("tki,tkf->if", h1, dh2), b2=dz2.sum(0),
                 w1=np.einsum("tkc,tki->ci", f, dz1), b1=dz1.sum((0, 1)))
    mags = dict(w_out=Ag.T @ ady, b_out=ady.sum(0),
                w2=np.einsum("tki,tkf->if", A1, Adh2), b2=Adz2.sum(0),
                w1=np.einsum("tkc,tki->ci", np.abs(f), Adz1), b1=Adz1.sum((0, 1)))
    return grads, mags


def bound(N: int, mag: np.ndarray) -> np.ndarray:
    return 4.0 * (N + 2) * U * mag


def chain_lengths(T: int, k: int, C: int, F1: int, F2: int, D: int) -> dict:
    """N per tensor: the largest number of products summed along the chain that ends in it."""
    return dict(out=max(2 * C, F1, F2), z2=max(2 * C, F1),
                w_out=max(T, 2 * C, F1), b_out=T, w2=max(T, D, 2 * C), b2=max(T, D),
                w1=max(T * k, F2, D), b1=max(T * k, F2, D))


def relu_margin(fw: dict) -> float:
    """min |z| / max |z| over both pre-activations: above 1e-5 no relu' can differ between the
    fp32 kernel and this restatement."""
    return min(float(np.abs(fw[z]).min() / np.abs(fw[z]).max()) for z in ("z1", "z2"))


# --------------------------------------------------------------------------------- known answers
def line_cloud() -> np.ndarray:
    pts = np.zeros((8, 3), f32)
    pts[:, 0] = np.arange(8)
    return pts


def lattice_cloud() -> np.ndarray:
    g = np.arange(5, dtype=f32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(125, 3)


# the backward cases of the GPU tests: (B, S, n, k, F1, F2, D), P, C and the seed whose relu margin
# test_pointcloud_cpu.py asserts
BWD_CASES = {
    "small": dict(shape=(2, 1, 4, 3, 32, 32, 16), P=24, C=3, seed=0),
    "wide": dict(shape=(1, 2, 5, 16, 64, 128, 48), P=40, C=6, seed=1),
    "largest": dict(shape=(1, 1, 6, 32, 128, 128, 64), P=48, C=8, seed=6),   # the widest layers
}


def bwd_case(name: str) -> dict:
    """points, start, parameters and dy of a backward case, and the restatement's own indices."""
    c = BWD_CASES[name]
    B, S, n, k, F1, F2, D = c["shape"]
    rng = np.random.default_rng([c["seed"], len(name)])
    points = rng.standard_normal((B, S, c["P"], c["C"])).astype(f32)
    p = init_params(rng, c["C"], F1, F2, D)
    dy = rng.standard_normal((B, S, n, D)).astype(f32)
    cidx, nidx = sample_group(points, n, k)
    return dict(points=points, params=p, dy=dy, cidx=cidx, nidx=nidx, **c)
