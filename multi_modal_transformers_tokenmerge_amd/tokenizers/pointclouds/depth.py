"""Depth images to point clouds on the device (csrc/depth.hip, mmt_depth_unproject in
include/mmt_api.h): what a depth camera delivers, uint16 millimetres plus pinhole intrinsics,
becomes the ``point_clouds`` and ``point_cloud_counts`` arguments of Octo in one launch, inside
the step's captured graph.

    z = d * depth_scale; valid: d != 0 (uint16) or d > 0 and finite (fp32), z_min <= z <= z_max
    x = (u - cx) * z / fx, y = (v - cy) * z / fy   (every operation individually rounded)
    with pose (camera -> base, [R | t]): p' = R p + t; with rgb: three more features, channel / 255
    the V valid pixels in raster order; V > P: the P of ranks ceil(q V / P); counts = min(V, P)

A frame with fewer valid points than the PointCloud set has tokens becomes an absent set for its
sample (Octo ``point_cloud_counts``); a frame with none gives counts 0 and a cloud of zeros.
"""
from __future__ import annotations

import torch

from ... import _kernels as K


def depth_to_point_cloud(depth: torch.Tensor, intrinsics: torch.Tensor, num_points: int,
                         depth_scale: float = 0.001, z_range=(0.1, 3.0),
                         pose: torch.Tensor | None = None, rgb: torch.Tensor | None = None):
    """depth (..., H, W) uint16 or fp32 on the device, intrinsics (..., 4) fp32 = fx fy cx cy,
    pose (..., 3, 4) fp32 or None, rgb (..., H, W, 3) uint8 or None ->
    (points (..., num_points, C) fp32, counts (...) int32), C = 6 with rgb, else 3. With fewer
    than two leading dimensions the images count as (B, 1) or (1, 1) clouds. ValueError before
    any launch: K.depth_unproject's checks (dtypes, shapes, devices, 1 <= num_points <= 4096,
    H W <= 2^20 and a multiple of 8 / 4, depth_scale > 0, z_range ascending)."""
    if not torch.is_tensor(depth) or depth.dim() < 2:
        raise ValueError("depth must be a (..., H, W) tensor")
    if not isinstance(z_range, (tuple, list)) or len(z_range) != 2:
        raise ValueError(f"z_range must be a pair (z_min, z_max), got {z_range!r}")
    lead = tuple(depth.shape[:-2])
    H, W = depth.shape[-2:]
    n = 1
    for d in lead:
        n *= d
    B, S = (lead if len(lead) == 2 else (n, 1))

    def shaped(t, tail, what):
        if t is None:
            return None
        if not torch.is_tensor(t) or tuple(t.shape) != lead + tail:
            raise ValueError(f"{what} must be a tensor of shape {lead + tail}")
        return t.reshape(B, S, *tail)

    points, counts = K.depth_unproject(
        depth.reshape(B, S, H, W), shaped(intrinsics, (4,), "intrinsics"), num_points, depth_scale,
        z_range[0], z_range[1], shaped(pose, (3, 4), "pose"), shaped(rgb, (H, W, 3), "rgb"))
    return points.view(*lead, num_points, points.shape[-1]), counts.reshape(lead)
