"""numpy restatement of the ragged point clouds (mmt_pc_sample_group_counts), of the thin-cloud
rule of mmt_pad_mask_pack_counts and of the depth back-projection (mmt_depth_unproject), on top of
the unchanged tests/pointcloud_ref.py. Test infrastructure only.

Ragged sampling and grouping: slice the cloud to its c rows, run the unragged restatement with
min(n, c) centroids and min(k, c) neighbours, then apply the repeat rules: centroids repeat
periodically (ids[i] = ids[i - c]), neighbour slots past the cloud repeat slot 0.

Back-projection: numpy float32 arrays, one rounded operation per numpy operation, as the kernel's
__f*_rn intrinsics.
"""
from __future__ import annotations

import numpy as np

from oracle import rng as RNG
from tests import pointcloud_ref as R

f32 = np.float32


# --------------------------------------------------------------------------------- ragged indices
def clamp_counts(counts: np.ndarray, P: int) -> np.ndarray:
    return np.clip(np.asarray(counts, np.int64), 0, P).astype(np.int32)


def sample_group_counts(points: np.ndarray, n: int, k: int, counts: np.ndarray, start=None):
    """points (B, S, P, C), counts (B, S) -> (centroid_idx (B, S, n), neighbour_idx (B, S, n, k),
    fault): fault is whether the device status word gets MMT_FAULT_ROW_INDEX (a count outside
    [0, P], an injected start not below the clamped count)."""
    B, S, P = points.shape[:3]
    cc = clamp_counts(counts, P)
    fault = bool((cc != np.asarray(counts)).any())
    cidx = np.zeros((B, S, n), np.int32)
    nidx = np.zeros((B, S, n, k), np.int32)
    for b in range(B):
        for s in range(S):
            c = int(cc[b, s])
            st = 0
            if start is not None:
                st = int(start[b, s])
                if not 0 <= st < c:
                    st, fault = 0, True
            if c == 0:
                continue
            ns, kk = min(n, c), min(k, c)
            ci, ni = R.sample_group(points[b:b + 1, s:s + 1, :c], ns, kk, np.array([[st]]))
            cidx[b, s, :ns] = ci[0, 0]
            nidx[b, s, :ns, :kk] = ni[0, 0]
            nidx[b, s, :ns, kk:] = nidx[b, s, :ns, :1]
            for i in range(ns, n):
                cidx[b, s, i] = cidx[b, s, i - c]
                nidx[b, s, i] = nidx[b, s, i - c]
    return cidx, nidx, fault


def drawn_start_counts(seed: int, step: int, counts: np.ndarray, P: int,
                       sample_offset: int = 0) -> np.ndarray:
    """The train-mode first centroids: (draw_u32(key, g) * c) >> 32 with the clamped count."""
    B, S = counts.shape
    key = RNG.stream_key(seed, step, R.FPS_LAYER, R.FPS_SITE)
    g = (np.arange(B, dtype=np.uint64)[:, None] + np.uint64(sample_offset)) * np.uint64(S) + \
        np.arange(S, dtype=np.uint64)[None, :]
    u = RNG.draw_u32(key, g & RNG.M32).astype(np.uint64)
    return ((u * clamp_counts(counts, P).astype(np.uint64)) >> np.uint64(32)).astype(np.int32)


# --------------------------------------------------------------------------------- thin clouds
def pack_counts(set_mask, n_sets: int, readout_bits: int, counts: np.ndarray, pc_sets, min_points):
    """(words (B,) uint32, fault): pad_mask_pack's words with bit pc_sets[s] cleared where
    counts[b, s] < min_points[s]; fault: a Readout set flagged absent in set_mask."""
    B = counts.shape[0]
    words = np.zeros(B, np.uint32)
    fault = False
    for b in range(B):
        w = (1 << n_sets) - 1
        if set_mask is not None:
            w = sum(1 << s for s in range(n_sets) if set_mask[b, s])
            if ~w & readout_bits:
                fault = True
                w |= readout_bits
        for s, (si, m) in enumerate(zip(pc_sets, min_points)):
            if counts[b, s] < m:
                w &= ~(1 << si)
        words[b] = w
    return words, fault


# --------------------------------------------------------------------------------- selection
def selected_ranks(V: int, P: int) -> list:
    """The ranks (raster order among the V valid pixels) of the slots 0 .. min(V, P) - 1."""
    if V <= P:
        return list(range(V))
    return [(q * V + P - 1) // P for q in range(P)]      # ceil(q V / P), exact integers


def slot_of_rank(j: int, V: int, P: int):
    """The kernel's form of the same rule, from the pixel's side: the slot rank j owns, or None.
    V <= P: slot j. Else slot floor(j P / V) iff (j P mod V) < P."""
    if V <= P:
        return j
    q, rem = divmod(j * P, V)
    return q if rem < P else None


# --------------------------------------------------------------------------------- back-projection
def valid_mask(depth: np.ndarray, scale, z_min, z_max) -> np.ndarray:
    d = depth.astype(f32)
    with np.errstate(all="ignore"):
        z = d * f32(scale)
        ok = (d > 0) & np.isfinite(d) & (z >= f32(z_min)) & (z <= f32(z_max))
    return ok


def unproject(depth: np.ndarray, intrinsics: np.ndarray, P: int, scale=0.001, z_min=0.1, z_max=3.0,
              pose=None, rgb=None):
    """depth (B, S, H, W) uint16 / float32 -> (points (B, S, P, C) float32, counts (B, S) int32)."""
    B, S, H, W = depth.shape
    C = 6 if rgb is not None else 3
    points = np.zeros((B, S, P, C), f32)
    counts = np.zeros((B, S), np.int32)
    for b in range(B):
        for s in range(S):
            ok = valid_mask(depth[b, s], scale, z_min, z_max).reshape(-1)
            pix = np.flatnonzero(ok)                         # raster order
            V = pix.size
            pix = pix[selected_ranks(V, P)] if V else pix
            m = pix.size
            counts[b, s] = m
            fx, fy, cx, cy = (f32(v) for v in intrinsics[b, s])
            v, u = pix // W, pix % W
            with np.errstate(all="ignore"):
                z = depth[b, s].reshape(-1)[pix].astype(f32) * f32(scale)
                x = ((u.astype(f32) - cx) * z) / fx
                y = ((v.astype(f32) - cy) * z) / fy
                p = np.stack([x, y, z], -1)
                if pose is not None:
                    Rt = pose[b, s].astype(f32)
                    p = np.stack([((Rt[i, 0] * x + Rt[i, 1] * y) + Rt[i, 2] * z) + Rt[i, 3]
                                  for i in range(3)], -1)
            assert p.dtype == f32
            points[b, s, :m, :3] = p
            if rgb is not None:
                points[b, s, :m, 3:] = rgb[b, s].reshape(-1, 3)[pix].astype(f32) / f32(255.0)
    return points, counts
