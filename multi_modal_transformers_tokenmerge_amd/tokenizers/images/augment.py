"""Image augmentation on the device (csrc/augment.hip, mmt_image_augment in include/mmt_api.h):
the Octo training recipe for uint8 camera frames, one launch pair inside the step's captured graph.

    primary camera: random resized crop (scale, aspect ratio) resampled bilinearly to the frame's
                    size, then brightness, contrast and saturation jitter
    wrist camera:   the colour jitter alone

One draw per (global sample, camera), keyed by (seed, step, sample_offset + b) like every other
random stream here: a 1-GPU run and an N-GPU run see the same crops, a replayed graph a new one
every step, and the image slots of a sample that share a camera (a history window) are cropped
and tinted alike. The arithmetic is pinned operation by operation (tests/image_augment_ref.py
restates it in numpy float32, bit for bit). Against dlimp / TF: the aspect ratio is drawn
uniformly (not log-uniformly), the contrast mean is taken over the integer source box of the crop
(not the resampled frame), and the pixel is clamped once, at the end; hue is not built.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Sequence

import torch

from ... import _kernels as K


def _pair(v, what: str):
    try:
        lo, hi = v
        return float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a pair (lo, hi), got {v!r}") from None


@dataclass(frozen=True)
class CameraAugmentation:
    """One camera's ranges. scale: the crop's area as a fraction of the frame, 0 < lo <= hi <= 1;
    ratio: its aspect ratio w / h, drawn uniformly, 0 < lo <= hi; brightness: the largest shift
    as a fraction of 255, in [0, 1]; contrast, saturation: the factor ranges, 0 <= lo <= hi. The
    defaults change nothing."""
    scale: tuple = (1.0, 1.0)
    ratio: tuple = (1.0, 1.0)
    brightness: float = 0.0
    contrast: tuple = (1.0, 1.0)
    saturation: tuple = (1.0, 1.0)

    def __post_init__(self):
        for f in ("scale", "ratio", "contrast", "saturation"):
            object.__setattr__(self, f, _pair(getattr(self, f), f))
        try:
            object.__setattr__(self, "brightness", float(self.brightness))
        except (TypeError, ValueError):
            raise ValueError(f"brightness must be a number, got {self.brightness!r}") from None
        K.check_augment_tables([0], [self.row()])

    def row(self) -> tuple:
        """The camera's row of mmt_image_augment's cam_params (K.AUGMENT_FIELDS)."""
        return (*self.scale, *self.ratio, self.brightness, *self.contrast, *self.saturation)

    @classmethod
    def of(cls, spec) -> "CameraAugmentation":
        """A CameraAugmentation, or a mapping of its fields (a YAML node)."""
        if isinstance(spec, cls):
            return spec
        names = {f.name for f in fields(cls)}
        if not isinstance(spec, dict) or set(spec) - names:
            raise ValueError(f"a camera's augmentation must be a mapping with keys among "
                             f"{sorted(names)}, got {spec!r}")
        return cls(**spec)


OCTO_PRIMARY = CameraAugmentation((0.8, 1.0), (0.9, 1.1), 0.1, (0.9, 1.1), (0.9, 1.1))
OCTO_WRIST = CameraAugmentation(brightness=0.1, contrast=(0.9, 1.1), saturation=(0.9, 1.1))


class ImageAugmentation:
    """``ImageAugmentation(cameras, image_camera)``: cameras, a sequence of CameraAugmentation (or
    mappings of its fields); image_camera, the camera index of every image slot of a sample.
    ``aug(images, rng)`` returns the augmented copy of uint8 (B, I, H, W, 3) frames. The device
    tables and the workspace are made on the first call for a (device, B) and kept: that upload
    is a host-to-device copy, which a graph capture cannot hold, so the first call for a shape
    must run outside a capture (DDPStep.build's warm-up steps do), or ``prepare(device, B)`` is
    called first; a captured call then allocates the output alone (nothing with ``out=``).
    ValueError at construction: K.check_augment_tables' faults."""

    def __init__(self, cameras: Sequence, image_camera: Sequence[int]):
        self.cameras = tuple(CameraAugmentation.of(c) for c in cameras)
        self.tables = K.check_augment_tables(image_camera, [c.row() for c in self.cameras])
        self.image_camera = tuple(self.tables[0])
        self._dev = {}   # device -> (image_camera, cam_params)
        self._ws = {}    # (device, B) -> workspace

    @property
    def n_cam(self) -> int:
        return len(self.cameras)

    def device_tables(self, device):
        """(image_camera int32 (I,), cam_params fp32 (n_cam, 9)) on `device`."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = (
                torch.tensor(self.tables[0], dtype=torch.int32, device=device),
                torch.tensor(self.tables[1], dtype=torch.float32, device=device))
        return self._dev[device]

    def workspace(self, device, B: int) -> torch.Tensor:
        """The kept workspace for B samples on `device`."""
        key = (torch.device(device), int(B))
        if key not in self._ws:
            need = K.image_augment_workspace(B, len(self.image_camera))
            self._ws[key] = torch.empty((need,), dtype=torch.uint8, device=key[0])
        return self._ws[key]

    def prepare(self, device, B: int) -> "ImageAugmentation":
        """Make the device tables and the workspace for B samples now, outside any capture."""
        self.device_tables(device)
        self.workspace(device, B)
        return self

    def __call__(self, images: torch.Tensor, rng: torch.Tensor, sample_offset: int = 0,
                 out: torch.Tensor | None = None, params_out: torch.Tensor | None = None):
        """images uint8 (B, I, H, W, 3) on the device, I = len(image_camera); rng the int32
        {seed, step} words; params_out (optional) fp32 (B, n_cam, 8) receives w, h, x0, y0, d, fc,
        fs, 0 of every (sample, camera). ValueError before any launch: K.image_augment's checks;
        fp32 images are refused (the augmentation is defined on uint8 frames)."""
        if not torch.is_tensor(images) or images.dtype != torch.uint8:
            raise ValueError("image augmentation takes uint8 frames (B, I, H, W, 3), got "
                             f"{getattr(images, 'dtype', type(images))}")
        if not images.is_cuda:
            raise ValueError("images must live on the GPU")
        if images.dim() != 5 or images.shape[1] != len(self.image_camera):
            raise ValueError(f"images {tuple(images.shape)}: expected (B, "
                             f"{len(self.image_camera)}, H, W, 3)")
        cam, par = self.device_tables(images.device)
        return K.image_augment(images, rng, cam, par, sample_offset, out, params_out,
                               self.workspace(images.device, images.shape[0]), tables=self.tables)
