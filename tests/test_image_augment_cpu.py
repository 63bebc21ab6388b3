"""CPU: the image augmentation outside the kernel: facts of the numpy float32 restatement
(tests/image_augment_ref.py) that the GPU tests compare bits against, the C ABI's rejections on
the library loaded without a GPU, the config key, the YAML and the preset."""
from dataclasses import asdict

import numpy as np
import pytest

from multi_modal_transformers_tokenmerge_amd import config_loader as C
from multi_modal_transformers_tokenmerge_amd.models.octo.config import PRESETS, OctoConfig, get_config
from tests import image_augment_ref as R

F = np.float32
SIZES = [(5, 7), (16, 16), (64, 48)]


def _frames(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _p(**kw):
    p = dict(w=1, h=1, x0=0, y0=0, d=0, fc=1, fs=1)
    p.update(kw)
    return {k: F(v) for k, v in p.items()}


# ------------------------------------------------------------------------ restatement facts
@pytest.mark.parametrize("H,W", SIZES + [(256, 256)])
def test_identity_parameters_return_the_input(H, W):
    img = _frames((2, 2, H, W, 3), seed=H)
    out, params = R.augment(img, 7, 3, [0, 1], [R.IDENTITY, R.IDENTITY])
    np.testing.assert_array_equal(out, img)
    np.testing.assert_array_equal(params[..., :7], np.broadcast_to(
        np.array([1, 1, 0, 0, 0, 1, 1], np.float32), (2, 2, 7)))
    assert not params[..., 7].any()


@pytest.mark.parametrize("H,W", SIZES)
def test_zero_saturation_gives_gray(H, W):
    img = _frames((H, W, 3), seed=1)
    out = R.augment_frame(img, _p(w=0.7, h=0.9, x0=0.1, y0=0.05, d=12, fc=1.3, fs=0))
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()
    assert out.std() > 0


@pytest.mark.parametrize("H,W", SIZES)
def test_constant_image_stays_constant_under_the_crop(H, W):
    img = np.empty((H, W, 3), np.uint8)
    img[:] = (31, 140, 222)
    for seed in range(8):
        p = R.draw_params(seed, 1, seed, 0, (0.05, 1.0, 0.5, 2.0, 0.0, 1.0, 1.0, 1.0, 1.0))
        np.testing.assert_array_equal(R.augment_frame(img, p), img)


def test_known_answer_2x2():
    """By hand. Crop w = h = 0.5 at x0 = y0 = 0.5 of a 2 x 2 frame: rows and columns sample at
    0.5 (between the two) and 1.0 (the last). Gray frame [[0, 100], [200, 60]]: the resampled
    values are [[90, 80], [130, 60]] (top = 50, bottom = 130, their midpoint 90; ...); the box is
    the whole frame, mean 360 / 4 = 90."""
    img = np.repeat(np.array([[0, 100], [200, 60]], np.uint8)[..., None], 3, axis=2)
    crop = dict(w=0.5, h=0.5, x0=0.5, y0=0.5)
    got = R.augment_frame(img, _p(**crop))
    np.testing.assert_array_equal(got[..., 0], [[90, 80], [130, 60]])
    # brightness +10 and contrast 2 about mean + 10 = 100: (v + 10 - 100) 2 + 100
    got = R.augment_frame(img, _p(d=10, fc=2, **crop))
    np.testing.assert_array_equal(got[..., 1], [[100, 80], [180, 40]])
    # contrast 4: 100, 60, 260 and -20: the one clamp, at the end
    got = R.augment_frame(img, _p(d=10, fc=4, **crop))
    np.testing.assert_array_equal(got[..., 2], [[100, 60], [255, 0]])
    # a coloured pixel, saturation 0: the gray 0.299 r + 0.587 g + 0.114 b = 29.9 + 117.4 + 5.7
    one = np.array([[[100, 200, 50]]], np.uint8)
    np.testing.assert_array_equal(R.augment_frame(one, _p(fs=0)), [[[153, 153, 153]]])
    # saturation 2: gray + 2 (v - gray) = 47, 247, -53
    np.testing.assert_array_equal(R.augment_frame(one, _p(fs=2)), [[[47, 247, 0]]])
    # rint rounds half to even: 2 x 1 frame [1, 2] sampled at 0.5 is 1.5 -> 2; [2, 3]: 2.5 -> 2
    for lo, want in ((1, 2), (2, 2)):
        col = np.repeat(np.array([[lo], [lo + 1]], np.uint8)[..., None], 3, axis=2)
        got = R.augment_frame(col, _p(h=0.5, y0=0.5))
        assert got[0, 0, 0] == want and got[1, 0, 0] == lo + 1


def test_slots_of_one_camera_share_the_draw_and_cameras_do_not():
    frame = _frames((2, 1, 16, 16, 3), seed=5)
    img = np.repeat(frame, 3, axis=1)
    out, params = R.augment(img, 11, 4, [0, 1, 0], [R.OCTO, R.OCTO])
    np.testing.assert_array_equal(out[:, 0], out[:, 2])
    assert (out[:, 0] != out[:, 1]).any()
    assert (params[:, 0, :7] != params[:, 1, :7]).all()
    assert (params[0] != params[1]).any()          # and samples differ


@pytest.mark.parametrize("row", [R.OCTO, R.WILD], ids=["octo", "wild"])
def test_draws_lie_in_their_ranges(row):
    us = []
    for g in range(200):
        p = R.draw_params(3, g % 5, g, g % 2, row)
        assert F(row[0]) <= p["area"] <= F(row[1]) and F(row[2]) <= p["rho"] <= F(row[3])
        assert F(row[5]) <= p["fc"] <= F(row[6]) and F(row[7]) <= p["fs"] <= F(row[8])
        assert 0 < p["w"] <= 1 and 0 < p["h"] <= 1
        assert 0 <= p["x0"] <= F(1) - p["w"] and 0 <= p["y0"] <= F(1) - p["h"]
        assert abs(p["d"]) <= F(row[4]) * F(255)
        us.append(R.uniforms(3, g % 5, g, g % 2))
    us = np.stack(us)
    assert us.dtype == np.float32 and (us >= 0).all() and (us < 1).all()
    assert len(np.unique(us)) == us.size           # seven distinct counters per draw


def test_sample_positions_stay_inside_the_frame():
    for H, W in SIZES + [(256, 256)]:
        for g in range(100):
            p = R.draw_params(1, 2, g, 0, R.WILD)
            for org, step, n in ((p["y0"], p["h"], H), (p["x0"], p["w"], W)):
                s = org * F(n - 1) + np.arange(n, dtype=np.float32) * step
                assert s.min() >= 0 and s.max() <= n - 1


# ------------------------------------------------------------------------ C ABI, no GPU
PTR = 1 << 20          # non-null, 16-B aligned; never dereferenced on a rejected call
N = 2 * 3 * 8 * 8 * 3


def _aug(lib, images=PTR, B=2, I=3, H=8, W=8, rng=PTR, offset=0, cams=PTR, params=PTR, n_cam=2,
         out=PTR + (1 << 16), params_out=None, ws=PTR + (1 << 18), ws_bytes=1 << 12):
    return lib.mmt_image_augment(images, B, I, H, W, rng, offset, cams, params, n_cam, out,
                                 params_out, ws, ws_bytes, None)


REJECTED = [
    ("null-images", lambda l: _aug(l, images=None)),
    ("null-rng", lambda l: _aug(l, rng=None)),
    ("null-image_camera", lambda l: _aug(l, cams=None)),
    ("null-cam_params", lambda l: _aug(l, params=None)),
    ("null-out", lambda l: _aug(l, out=None)),
    ("null-workspace", lambda l: _aug(l, ws=None)),
    ("images-unaligned", lambda l: _aug(l, images=PTR + 8)),
    ("out-unaligned", lambda l: _aug(l, out=PTR + (1 << 16) + 4)),
    ("workspace-unaligned", lambda l: _aug(l, ws=PTR + (1 << 18) + 8)),
    ("rng-unaligned", lambda l: _aug(l, rng=PTR + 2)),
    ("cam_params-unaligned", lambda l: _aug(l, params=PTR + 1)),
    ("params_out-unaligned", lambda l: _aug(l, params_out=PTR + (1 << 19) + 2)),
    ("B-0", lambda l: _aug(l, B=0)),
    ("I-0", lambda l: _aug(l, I=0)),
    ("I-65", lambda l: _aug(l, I=65)),
    ("H-0", lambda l: _aug(l, H=0)),
    ("W-neg", lambda l: _aug(l, W=-8)),
    ("H-2049", lambda l: _aug(l, H=2049, out=PTR + (1 << 30))),
    ("W-2049", lambda l: _aug(l, W=2049, out=PTR + (1 << 30))),
    ("n_cam-0", lambda l: _aug(l, n_cam=0)),
    ("n_cam-17", lambda l: _aug(l, n_cam=17)),
    ("in-place", lambda l: _aug(l, out=PTR)),
    ("overlap-tail", lambda l: _aug(l, out=PTR + N - 16)),
    ("overlap-head", lambda l: _aug(l, images=PTR + N - 16, out=PTR)),
    ("offset-neg", lambda l: _aug(l, offset=-1)),
    ("workspace-small", lambda l: _aug(l, ws_bytes=2 * 3 * 8 * 16 - 1)),
]


@pytest.mark.parametrize("call", [c[1] for c in REJECTED], ids=[c[0] for c in REJECTED])
def test_entry_point_rejects_without_gpu(call):
    """Each returns MMT_ERR_INVALID before any HIP call, with a message naming the entry."""
    from multi_modal_transformers_tokenmerge_amd import _C
    lib = _C.lib()
    # leave another entry point's message behind first, so a stale one cannot satisfy the check
    assert lib.mmt_step_advance(None, None) == -1 and b"mmt_step_advance" in lib.mmt_last_error()
    assert call(lib) == -1
    msg = lib.mmt_last_error()
    assert msg and b"mmt_image_augment" in msg, msg


def test_workspace_size_and_binding():
    import re
    from pathlib import Path
    from multi_modal_transformers_tokenmerge_amd import _C
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    assert K.image_augment_workspace(2, 3) == 2 * 3 * 8 * 16
    for bad in ((0, 1), (1, 0), (1, 65)):
        with pytest.raises(_C.MMTError, match="mmt_image_augment_workspace"):
            K.image_augment_workspace(*bad)
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mmt_api.h").read_text()
    m = re.search(r"int mmt_image_augment\((.*?)\);", hdr, flags=re.S)
    assert len(_C.SIGNATURES["mmt_image_augment"]) == len(m.group(1).split(","))
    assert "0xFFF6" in hdr
    from multi_modal_transformers_tokenmerge_amd.csrc import build
    assert "augment.hip" in build.NO_CONTRACT


# ------------------------------------------------------------------------ tables and config
def test_check_augment_tables():
    from multi_modal_transformers_tokenmerge_amd import _kernels as K
    cams, rows = K.check_augment_tables([0, 1, 0], [R.OCTO, R.WILD], 3)
    assert cams == [0, 1, 0] and rows == [tuple(map(float, R.OCTO)), tuple(map(float, R.WILD))]

    def row(**kw):
        d = dict(zip(R.FIELDS, R.OCTO))
        d.update(kw)
        return tuple(d[k] for k in R.FIELDS)
    bad_rows = [row(scale_lo=0.0), row(scale_lo=-0.1), row(scale_hi=1.01), row(scale_lo=0.9, scale_hi=0.8),
                row(ratio_lo=0.0), row(ratio_lo=1.2), row(brightness=-0.1), row(brightness=1.5),
                row(contrast_lo=-0.5), row(contrast_lo=1.2), row(sat_lo=-1.0), row(sat_lo=2.0),
                row(sat_hi=float("nan")), row(contrast_hi=float("inf")), R.OCTO[:8]]
    for r in bad_rows:
        with pytest.raises(ValueError):
            K.check_augment_tables([0], [r])
    for cams in ([1], [-1], [0.5], [], [0] * 65):
        with pytest.raises(ValueError):
            K.check_augment_tables(cams, [R.OCTO])
    with pytest.raises(ValueError):
        K.check_augment_tables([0, 0], [R.OCTO], 3)            # not the images' slot count
    with pytest.raises(ValueError):
        K.check_augment_tables([0], [])
    with pytest.raises(ValueError):
        K.check_augment_tables([0], [R.OCTO] * 17)


def test_camera_augmentation_and_presets():
    from multi_modal_transformers_tokenmerge_amd.tokenizers.images.augment import (
        OCTO_PRIMARY, OCTO_WRIST, CameraAugmentation, ImageAugmentation)
    assert CameraAugmentation().row() == R.IDENTITY
    assert OCTO_PRIMARY.row() == R.OCTO
    assert OCTO_WRIST.row() == (1.0, 1.0, 1.0, 1.0) + R.OCTO[4:]
    assert CameraAugmentation.of(dict(scale=[0.5, 1], brightness=0.2)).row() == \
        (0.5, 1.0, 1.0, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0)
    for bad in (dict(scale=(0.0, 1.0)), dict(scale=(0.5, 1.5)), dict(ratio=(2.0, 1.0)),
                dict(brightness=2.0), dict(contrast=(-1.0, 1.0)), dict(saturation=(1.0,)),
                dict(scale=0.5), dict(brightness="x")):
        with pytest.raises(ValueError):
            CameraAugmentation(**bad)
    with pytest.raises(ValueError):
        CameraAugmentation.of(dict(hue=0.1))
    aug = ImageAugmentation([OCTO_PRIMARY, dict(brightness=0.1)], [0, 1, 0, 1])
    assert aug.n_cam == 2 and aug.image_camera == (0, 1, 0, 1)
    with pytest.raises(ValueError):
        ImageAugmentation([OCTO_PRIMARY], [0, 1])


TWO_CAM = "[TaskDescriptionPrefix{32}] [Image{256};Image{256};Readout{4}]*2"


def test_config_validation():
    assert OctoConfig().image_augmentation is None
    assert all(c.image_augmentation is None for n, c in PRESETS.items() if not n.endswith("-aug"))
    cam = dict(scale=(0.8, 1.0))
    one = OctoConfig(image_augmentation=dict(cameras=[cam]))
    assert one.image_camera() == [0]
    two = OctoConfig(input_sequence=TWO_CAM, num_observation_blocks=2,
                     image_augmentation=dict(cameras=[cam, {}]))
    assert two.image_camera() == [0, 1, 0, 1]        # a history window shares its camera's draw
    own = OctoConfig(input_sequence=TWO_CAM, num_observation_blocks=2,
                     image_augmentation=dict(cameras=[cam, {}], image_camera=[0, 0, 1, 1]))
    assert own.image_camera() == [0, 0, 1, 1]
    bad = [dict(cameras=[]), dict(cameras=[cam, cam]), dict(camera=[cam]), [cam],
           dict(cameras=[dict(scale=(0.0, 1.0))]), dict(cameras=[dict(hue=0.1)]),
           dict(cameras=[cam], image_camera=[0, 0]), dict(cameras=[cam], image_camera=[1]),
           dict(cameras=[cam], extra=1)]
    for aug in bad:
        with pytest.raises(ValueError):
            OctoConfig(image_augmentation=aug)
    for aug in (dict(cameras=[cam]), dict(cameras=[cam, cam, cam]),
                dict(cameras=[cam, cam], image_camera=[0, 1, 0]),
                dict(cameras=[cam, cam], image_camera=[0, 0, 0, 0]),
                dict(cameras=[cam, cam], image_camera=[0, 1, 2, 0])):
        with pytest.raises(ValueError):
            OctoConfig(input_sequence=TWO_CAM, num_observation_blocks=2, image_augmentation=aug)
    with pytest.raises(ValueError):                  # no Image set to augment
        OctoConfig(input_sequence="[TaskDescriptionPrefix{32}] [Readout{4}]",
                   image_augmentation=dict(cameras=[cam]))


def test_yaml_and_preset_load():
    a = asdict(C.load_octo_config("octo_small_tome16_aug"))
    b = asdict(PRESETS["octo-small-tome16-aug"])
    assert b["image_augmentation"] == dict(cameras=[dict(
        scale=(0.8, 1.0), ratio=(0.9, 1.1), brightness=0.1, contrast=(0.9, 1.1),
        saturation=(0.9, 1.1))])
    assert not {k: (a[k], b[k]) for k in a if k not in ("name", "stem") and a[k] != b[k]}
    c = asdict(PRESETS["octo-small-tome16"])
    assert {k for k in b if b[k] != c[k]} == {"name", "image_augmentation"}
    assert get_config("octo_small_tome16_aug").image_augmentation == b["image_augmentation"]
    assert C.load_octo_config("octo_small_tome16").image_augmentation is None
    # the key parses from an override too, image_camera included
    key = "tokenizers.images.augmentation"
    y = C.octo_config_from_yaml(C.compose("octo_base_2cam", overrides=[
        key + "={cameras: [{scale: [0.8, 1.0]}, {brightness: 0.1}], image_camera: [0, 1, 0, 1]}"]))
    assert y.image_camera() == [0, 1, 0, 1] and len(y.image_augmentation["cameras"]) == 2
    with pytest.raises(ValueError):
        C.octo_config_from_yaml(C.compose("octo_small_tome16", overrides=[key + "={cameras: 3}"]))


def test_model_holds_the_augmentation_on_cpu():
    from multi_modal_transformers_tokenmerge_amd.models.octo.octo import Octo
    cam = dict(scale=(0.8, 1.0), brightness=0.1)
    on = Octo(get_config("octo-tiny", image_augmentation=dict(cameras=[cam])), device="cpu", seed=0)
    off = Octo(get_config("octo-tiny"), device="cpu", seed=0)
    assert off.augmentation is None and on.augmentation.image_camera == (0,)
    assert on.store.n == off.store.n                 # no parameter
