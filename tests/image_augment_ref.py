"""numpy float32 restatement of the image augmentation (include/mmt_api.h "image augmentation",
csrc/augment.hip): random resized crop, bilinear and corner-aligned, plus brightness, contrast and
saturation jitter of uint8 frames. Written from the specification, one numpy float32 operation per
rounded operation of the kernel, so the GPU tests compare bits. The draws come from oracle.rng.

Every array below is float32 and every binary operation is between float32 operands: numpy then
rounds each result to float32 once, which is what the kernel's __f*_rn intrinsics do."""
import numpy as np

from oracle import rng as R

F = np.float32
LAYER = 0xFFF6
FIELDS = ("scale_lo", "scale_hi", "ratio_lo", "ratio_hi", "brightness", "contrast_lo",
          "contrast_hi", "sat_lo", "sat_hi")
IDENTITY = (1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0)
# the two parameter sets of the tests: Octo's ranges and a wild set
OCTO = (0.8, 1.0, 0.9, 1.1, 0.1, 0.9, 1.1, 0.9, 1.1)
WILD = (0.05, 1.0, 0.5, 2.0, 0.5, 0.2, 3.0, 0.0, 3.0)


def uniforms(seed: int, step: int, g: int, cam: int) -> np.ndarray:
    """u_0 .. u_6 of (global sample g, camera cam): the 24-bit uniforms at counters 8 g + j."""
    key = R.stream_key(seed, step, LAYER, cam)
    ctr = (np.uint64(8) * np.uint64(g) + np.arange(7, dtype=np.uint64)) & R.M32
    return R.uniform01(key, ctr)


def _lerp(lo, hi, u):
    return F(lo) + u * (F(hi) - F(lo))


def draw_params(seed: int, step: int, g: int, cam: int, row) -> dict:
    """w, h, x0, y0, d, fc, fs (and area, rho) of one (sample, camera); row: the camera's FIELDS."""
    u = uniforms(seed, step, g, cam)
    slo, shi, rlo, rhi, br, clo, chi, tlo, thi = (F(v) for v in row)
    area = _lerp(slo, shi, u[0])
    rho = _lerp(rlo, rhi, u[1])
    w = np.minimum(F(1), np.sqrt(area * rho))
    h = np.minimum(F(1), np.sqrt(area / rho))
    x0 = u[2] * (F(1) - w)
    y0 = u[3] * (F(1) - h)
    d = ((F(2) * u[4] - F(1)) * br) * F(255)
    fc = _lerp(clo, chi, u[5])
    fs = _lerp(tlo, thi, u[6])
    out = dict(area=area, rho=rho, w=w, h=h, x0=x0, y0=y0, d=d, fc=fc, fs=fs)
    assert all(v.dtype == np.float32 for v in out.values())
    return out


def axis(org0, step, n: int):
    """Sample positions of the n outputs along an axis of n pixels: (i0, i1, t), int64 and
    float32. s = org0 (n - 1) + float(r) step."""
    r = np.arange(n, dtype=np.float32)
    s = org0 * F(n - 1) + r * step
    assert s.dtype == np.float32
    i0 = np.minimum(np.floor(s).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    t = s - i0.astype(np.float32)
    return i0, i1, t


def augment_frame(img: np.ndarray, p: dict) -> np.ndarray:
    """One uint8 (H, W, 3) frame under the parameters p."""
    H, W, _ = img.shape
    iy, iy1, ty = axis(p["y0"], p["h"], H)
    ix, ix1, tx = axis(p["x0"], p["w"], W)
    f = img.astype(np.float32)
    ty, tx = ty[:, None, None], tx[None, :, None]
    p00, p01 = f[iy][:, ix], f[iy][:, ix1]
    p10, p11 = f[iy1][:, ix], f[iy1][:, ix1]
    top = p00 + (p01 - p00) * tx
    bot = p10 + (p11 - p10) * tx
    v = top + (bot - top) * ty
    # contrast mean: exact integer sums over the source box, then float(sum) / float(n)
    box = img[iy[0]:iy1[-1] + 1, ix[0]:ix1[-1] + 1].astype(np.uint64)
    n = box.shape[0] * box.shape[1]
    m = box.sum(axis=(0, 1)).astype(np.float32) / F(n)
    d, fc, fs = p["d"], p["fc"], p["fs"]
    v1 = v + d
    mb = m + d
    v2 = (v1 - mb) * fc + mb
    gray = (F(0.299) * v2[..., 0] + F(0.587) * v2[..., 1]) + F(0.114) * v2[..., 2]
    v3 = gray[..., None] + (v2 - gray[..., None]) * fs
    assert v3.dtype == np.float32
    return np.rint(np.clip(v3, F(0), F(255))).astype(np.uint8)


def augment(images: np.ndarray, seed: int, step: int, image_camera, cam_params,
            sample_offset: int = 0):
    """images uint8 (B, I, H, W, 3) -> (out uint8 of that shape, params float32 (B, n_cam, 8) =
    w, h, x0, y0, d, fc, fs, 0)."""
    B, I = images.shape[:2]
    n_cam = len(cam_params)
    out = np.empty_like(images)
    params = np.zeros((B, n_cam, 8), np.float32)
    for b in range(B):
        ps = [draw_params(seed, step, sample_offset + b, c, cam_params[c]) for c in range(n_cam)]
        for c, p in enumerate(ps):
            params[b, c, :7] = [p[k] for k in ("w", "h", "x0", "y0", "d", "fc", "fs")]
        for i in range(I):
            out[b, i] = augment_frame(images[b, i], ps[image_camera[i]])
    return out, params
