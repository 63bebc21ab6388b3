"""Point-cloud tokens: a cloud (P, C) becomes n sequence rows, one per sampled centroid with its
neighbourhood, mirroring the reference's
``multi_modal_transformers/tokenizers/pointclouds/point_cloud_tokenizer.py`` (euclidean distance
:30-36, farthest_point_sampling :42-92, knn :106-116, SampleAndGroupModule :119-198), restated
where the reference cannot be followed (DESIGN.md §3 "Point-cloud tokens"). All fp32.

    d(p, c)  = (dx dx + dy dy) + dz dz on xyz, every operation individually rounded (no FMA)
    sampling : dist = +inf, ids[0] = start; ids[i] = argmax of dist = min(dist, d(., ids[i-1]))
               over the points not yet sampled, the lowest index on ties
    grouping : per centroid the k points of smallest d, ascending by (d, index)
    features : neighbour j of centroid c: [points[j] - points[c], points[j]]   (2 C numbers)
    token    : max_k relu(relu(feat W1 + b1) W2 + b2) . W_out + b_out   (+ pos_embedding[row])

The three departures from the reference: no BatchNorm (its ``use_running_average=is_training`` is
inverted and batch statistics would couple samples), a max over the neighbour axis as in the PCT
paper (the reference never reduces it), and ``output_dense`` (F2 -> D), which the reference lacks.
The kernels are csrc/pointcloud.hip (mmt_pc_sample_group, mmt_pc_sample_group_counts for ragged
clouds, mmt_pc_embed_fwd / _bwd, include/mmt_api.h); no gradient reaches the points. depth.py turns
depth images into clouds with counts.
"""
from __future__ import annotations

import torch

from ... import _kernels as K
from ...module_api import Bindable
from ...params import ParamStore, const, he_normal, xavier_uniform

CONFIG_KEYS = ("num_points", "num_neighbours_knn", "point_features", "hidden")


def check_point_cloud_config(num_points, num_tokens, num_neighbours_knn=16, point_features=3,
                             hidden=(64, 64)):
    """ValueError unless max(n, k) <= P <= 4096, 1 <= n <= 256, 1 <= k <= 32, 3 <= C <= 8 and
    hidden is a pair of widths among 32, 64, 128 (the kernels' limits)."""
    if not isinstance(hidden, (tuple, list)) or len(hidden) != 2:
        raise ValueError(f"hidden must be a pair of widths (F1, F2), got {hidden!r}")
    K.check_pc_limits(num_points, point_features, num_tokens, num_neighbours_knn, hidden[0],
                      hidden[1])


class PointCloudTokenizer(Bindable):
    """``PointCloudTokenizer(num_neighbours_knn=16, point_features=3, hidden=(64, 64))`` owns
    ``<name>/LBR_1/kernel`` (2C, F1), ``LBR_1/bias``, ``LBR_2/kernel`` (F1, F2), ``LBR_2/bias``
    (xavier_uniform kernels as the reference, zero biases) and ``output_dense/kernel`` (F2, D),
    ``output_dense/bias`` (the project's Dense default kernel, zero bias), all fp32 in the Flax
    (in, out) layout. One parameter set serves every PointCloud set and timestep.
    ``bind(store, name, D)`` declares them in a caller's store (Octo); the first call of an
    unbound module creates a private store, and then needs ``embedding_dim``."""

    def __init__(self, num_neighbours_knn: int = 16, point_features: int = 3, hidden=(64, 64),
                 embedding_dim: int | None = None, num_points: int | None = None):
        if not isinstance(hidden, (tuple, list)) or len(hidden) != 2:
            raise ValueError(f"hidden must be a pair of widths (F1, F2), got {hidden!r}")
        k, C = num_neighbours_knn, point_features
        # num_points (the YAML node's field): checked when given, the clouds' own P rules
        P = num_points if num_points is not None else (max(k, 1) if isinstance(k, int) else k)
        K.check_pc_limits(P, C, 1, k, hidden[0], hidden[1])
        self.num_points = num_points
        self.k, self.C = int(k), int(C)
        self.F1, self.F2 = int(hidden[0]), int(hidden[1])
        self.D = None if embedding_dim is None else int(embedding_dim)
        self.w1 = self.b1 = self.w2 = self.b2 = self.w_out = self.b_out = None

    def _declare(self, store: ParamStore, name: str, embedding_dim: int):
        self.D = D = int(embedding_dim)
        C2, F1, F2 = 2 * self.C, self.F1, self.F2
        self.w1 = store.add(f"{name}/LBR_1/kernel", (C2, F1), xavier_uniform((C2, F1)))
        self.b1 = store.add(f"{name}/LBR_1/bias", (F1,), const(0.0))
        self.w2 = store.add(f"{name}/LBR_2/kernel", (F1, F2), xavier_uniform((F1, F2)))
        self.b2 = store.add(f"{name}/LBR_2/bias", (F2,), const(0.0))
        self.w_out = store.add(f"{name}/output_dense/kernel", (F2, D), he_normal((F2, D)))
        self.b_out = store.add(f"{name}/output_dense/bias", (D,), const(0.0))

    def _all(self):
        return (self.w1, self.b1, self.w2, self.b2, self.w_out, self.b_out)

    @property
    def first_offset(self) -> int:
        return self.w1.offset

    # ------------------------------------------------------------------ the hooks Octo uses
    def forward(self, points: torch.Tensor, n: int, rows: torch.Tensor, pe: torch.Tensor,
                x0: torch.Tensor, train: bool = False, rng=None, sample_offset: int = 0,
                fps_start=None, counts=None) -> dict:
        """points (B, S, P, C) fp32, rows (S n,) int32: samples and groups every cloud, writes
        x0[b, rows[s n + m]] = token(b, s, m) + pe[rows[s n + m]] (no other row of x0) and returns
        the backward's saved state. The first centroid: fps_start (B, S) int32 if given, the
        counter-RNG draw in train mode, point 0 in eval mode. counts (B, S) int32: ragged clouds,
        the leading counts[b, s] rows of a cloud are its points (K.pc_sample_group); the
        embedding kernels take the padded groups as they are."""
        if points.shape[-1] != self.C:
            raise ValueError(f"points have {points.shape[-1]} features, the tokenizer "
                             f"point_features = {self.C}")
        cidx, nidx = K.pc_sample_group(points, n, self.k, fps_start,
                                       rng if (train and fps_start is None) else None,
                                       sample_offset, counts)
        w = [p.data for p in self._all()]
        argmax = K.pc_embed_fwd(points, cidx, nidx, *w, pe, rows, x0)
        return dict(points=points, cidx=cidx, nidx=nidx, argmax=argmax)

    def backward(self, dx0: torch.Tensor, sv: dict, rows: torch.Tensor):
        """The six parameter gradients += their values from the rows dx0[b, rows[s n + m]]: fixed
        summation order, added once (bitwise reproducible)."""
        K.pc_embed_bwd(dx0, rows, sv["points"], sv["cidx"], sv["nidx"], sv["argmax"],
                       self.w1.data, self.b1.data, self.w2.data, self.b2.data, self.w_out.data,
                       tuple(p.grad for p in self._all()))

    # ------------------------------------------------------------------ standalone module form
    def _clouds(self, points: torch.Tensor) -> torch.Tensor:
        if not torch.is_tensor(points) or points.dtype != torch.float32 or not points.is_cuda \
                or points.dim() < 2:
            raise ValueError("points must be an fp32 device tensor (..., P, C)")
        return points.reshape(-1, 1, *points.shape[-2:]).contiguous()

    def _counts(self, counts, p4: torch.Tensor):
        """counts: None, an int, or an int32 tensor (...) -> None or int32 (clouds, 1)."""
        if counts is None:
            return None
        if not torch.is_tensor(counts):
            return torch.full((p4.shape[0], 1), int(counts), dtype=torch.int32, device=p4.device)
        if counts.dtype != torch.int32 or counts.numel() != p4.shape[0] or \
                counts.device != p4.device:
            raise ValueError("counts must be an int32 tensor on the points' device with one "
                             f"entry per cloud ({p4.shape[0]})")
        return counts.reshape(p4.shape[0], 1).contiguous()

    def sample_and_group(self, points: torch.Tensor, n: int, start=None, counts=None):
        """points (..., P, C) -> (centroid_idx (..., n), neighbour_idx (..., n, k)) int32.
        start: None (point 0), an int, or an int32 tensor (...) of first centroids. counts: None
        (every cloud has P points), an int, or an int32 tensor (...): the leading rows of each
        cloud that are points."""
        p4 = self._clouds(points)
        lead = points.shape[:-2]
        counts = self._counts(counts, p4)
        if start is not None:
            if not torch.is_tensor(start):
                start = torch.full((p4.shape[0], 1), int(start), dtype=torch.int32,
                                   device=points.device)
            start = start.to(torch.int32).reshape(p4.shape[0], 1).contiguous()
        cidx, nidx = K.pc_sample_group(p4, n, self.k, start, counts=counts)
        return cidx.view(*lead, n), nidx.view(*lead, n, self.k)

    def farthest_point_sampling(self, points: torch.Tensor, num_samples: int, start=None,
                                counts=None):
        """Reference :42-92 on the device: the (..., num_samples) int32 indices of the sampled
        points. counts: sample_and_group's."""
        return self.sample_and_group(points, num_samples, start, counts)[0]

    def knn(self, points: torch.Tensor, centroid: int, k: int | None = None):
        """Reference :106-116 on the device: the k nearest points of point ``centroid`` of one
        cloud (P, C), ascending by (d, index), as int32 (k,). One sampling run with the centroid
        as its start."""
        tok = self if k is None or k == self.k else PointCloudTokenizer(k, self.C, (self.F1, self.F2))
        return tok.sample_and_group(points, 1, int(centroid))[1].reshape(-1, tok.k)[0]

    def __call__(self, points: torch.Tensor, n: int, start=None, counts=None) -> torch.Tensor:
        """(..., P, C) fp32 -> (..., n, D) fp32: the tokens alone, no position term. counts:
        sample_and_group's (a cloud with fewer points than n repeats its tokens)."""
        p4 = self._clouds(points)
        counts = self._counts(counts, p4)
        if self.w1 is None and self.D is None:
            raise ValueError("an unbound PointCloudTokenizer needs embedding_dim")
        self._ensure(points.device, self.D)
        dev, B = points.device, p4.shape[0]
        if start is not None and not torch.is_tensor(start):
            start = torch.full((B, 1), int(start), dtype=torch.int32, device=dev)
        out = torch.empty((B, n, self.D), dtype=torch.float32, device=dev)
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        zero = torch.zeros((n, self.D), dtype=torch.float32, device=dev)  # no position term
        self.last_saved = self.forward(p4, n, rows, zero, out, fps_start=start, counts=counts)
        return out.view(*points.shape[:-2], n, self.D)
