"""GPU: the image augmentation kernel (csrc/augment.hip mmt_image_augment) against the numpy
float32 restatement tests/image_augment_ref.py, bit for bit: the pixels, and the parameters
through their int32 views. Shapes: odd sizes whose images do not start 16-B aligned (5 x 7: byte
stores, pieces of the sum that straddle images), sizes no multiple of a thread's 16 pixels, more
than one workgroup per image (256 x 256), several image slots per camera."""
import numpy as np
import pytest
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from multi_modal_transformers_tokenmerge_amd import _kernels as K
from multi_modal_transformers_tokenmerge_amd.tokenizers.images.augment import (
    CameraAugmentation, ImageAugmentation)
from tests import image_augment_ref as R

pytestmark = pytest.mark.gpu

CAMS = [0, 1, 0]
SEED, STEP = 1234, 5
CONTRAST_OFF = (0.8, 1.0, 0.9, 1.1, 0.1, 1.0, 1.0, 0.9, 1.1)
SETS = {"octo": [R.OCTO, R.OCTO], "wild": [R.WILD, R.WILD], "identity": [R.IDENTITY, R.IDENTITY],
        "contrast-off": [CONTRAST_OFF, CONTRAST_OFF], "mixed": [R.WILD, R.IDENTITY]}


def _frames(shape, seed=0):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, shape, dtype=np.uint8)
    img[0, 0, : shape[2] // 2] //= 4          # a dark band and a bright one: the clamp is reached
    img[-1, -1, :, : shape[3] // 2] |= 0xC0
    return img


def _rng(dev, seed=SEED, step=STEP):
    return torch.tensor([seed, step], dtype=torch.int32, device=dev)


def _tables(dev, rows, cams=CAMS):
    return (torch.tensor(cams, dtype=torch.int32, device=dev),
            torch.tensor(rows, dtype=torch.float32, device=dev))


def _run(dev, img, rows, offset=0, rng=None, cams=CAMS, sentinel=0xA5):
    B, I = img.shape[:2]
    cam_t, par_t = _tables(dev, rows, cams)
    out = torch.full(img.shape, sentinel, dtype=torch.uint8, device=dev)
    params = torch.full((B, len(rows), 8), float("nan"), device=dev)
    got = K.image_augment(torch.from_numpy(img).to(dev), _rng(dev) if rng is None else rng, cam_t,
                          par_t, offset, out=out, params_out=params)
    assert got is out
    K.device_status()
    return out.cpu().numpy(), params.cpu().numpy()


def _compare(got, want, gp, wp):
    np.testing.assert_array_equal(gp.view(np.int32), wp.view(np.int32))
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at (b, i, y, x, ch) = {bad[0]}: " \
        f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("H,W", [(5, 7), (16, 16), (64, 48)])
def test_bits_match_the_restatement(dev, H, W, name):
    img = _frames((3, 3, H, W, 3), seed=H * W)
    want, wp = R.augment(img, SEED, STEP, CAMS, SETS[name], sample_offset=3)
    for sentinel in (0xA5, 0x5A):             # two fills: every byte of out is written
        got, gp = _run(dev, img, SETS[name], offset=3, sentinel=sentinel)
        _compare(got, want, gp, wp)
    if name == "identity":
        np.testing.assert_array_equal(got, img)


@pytest.mark.parametrize("name", ["octo", "wild"])
def test_bits_match_at_256(dev, name):
    img = _frames((3, 3, 256, 256, 3), seed=9)
    want, wp = R.augment(img, SEED, STEP, CAMS, SETS[name])
    got, gp = _run(dev, img, SETS[name])
    _compare(got, want, gp, wp)


def test_slots_of_a_camera_share_the_draw(dev):
    frame = _frames((3, 1, 16, 16, 3), seed=2)
    got, _ = _run(dev, np.repeat(frame, 3, axis=1).copy(), SETS["octo"])
    np.testing.assert_array_equal(got[:, 0], got[:, 2])
    assert (got[:, 0] != got[:, 1]).any()


def test_sample_offset_selects_the_global_sample(dev):
    img = _frames((4, 3, 16, 16, 3), seed=3)
    full, fp = _run(dev, img, SETS["wild"])
    part, pp = _run(dev, img[2:].copy(), SETS["wild"], offset=2)
    np.testing.assert_array_equal(full[2:], part)
    np.testing.assert_array_equal(fp[2:].view(np.int32), pp.view(np.int32))


def test_same_step_same_bits_other_step_other_crop(dev):
    img = _frames((3, 3, 16, 16, 3), seed=4)
    a, pa = _run(dev, img, SETS["octo"])
    b, pb = _run(dev, img, SETS["octo"])
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(pa.view(np.int32), pb.view(np.int32))
    c, pc = _run(dev, img, SETS["octo"], rng=_rng(dev, step=STEP + 1))
    assert (a != c).any() and (pa[..., :7] != pc[..., :7]).all()
    want, wp = R.augment(img, SEED, STEP + 1, CAMS, SETS["octo"])
    _compare(c, want, pc, wp)


def test_module_call_matches_and_is_capturable(dev):
    """ImageAugmentation: the same bits as the raw call, and a captured call follows the device
    step counter on replay (no host value baked in)."""
    img = _frames((2, 3, 16, 16, 3), seed=6)
    aug = ImageAugmentation([CameraAugmentation(*_fields(R.OCTO)),
                             dict(zip(("scale", "ratio", "brightness", "contrast", "saturation"),
                                      _fields(R.WILD)))], CAMS)
    rows = [R.OCTO, R.WILD]
    x = torch.from_numpy(img).to(dev)
    rng = _rng(dev)
    out = torch.empty_like(x)
    params = torch.empty((2, 2, 8), device=dev)
    aug.prepare(dev, 2)                            # the tables and the workspace, before a capture
    aug(x, rng, out=out, params_out=params)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        aug(x, rng, out=out, params_out=params)
    for step in (STEP, STEP + 7):
        rng.copy_(torch.tensor([SEED, step], dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        want, wp = R.augment(img, SEED, step, CAMS, rows)
        _compare(out.cpu().numpy(), want, params.cpu().numpy(), wp)


def _fields(row):
    return (row[0:2], row[2:4], row[4], row[5:7], row[7:9])


def test_wrapper_value_errors(dev):
    img = torch.zeros((2, 3, 8, 8, 3), dtype=torch.uint8, device=dev)
    rng = _rng(dev)
    cam, par = _tables(dev, SETS["octo"])
    ok = dict(images=img, rng=rng, image_camera=cam, cam_params=par)

    def bad(**kw):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            K.image_augment(**args)

    bad(images=img.float())                                   # dtype
    bad(images=img.cpu())                                     # device
    bad(images=img[:, :, :, :4])                              # contiguity
    bad(images=img[..., 0])                                   # rank
    bad(images=torch.zeros((2, 3, 8, 8, 4), dtype=torch.uint8, device=dev))
    bad(images=torch.zeros((2, 3, 8, 2049, 3), dtype=torch.uint8, device=dev))
    bad(images=img.flatten()[1:1 + 2 * 3 * 8 * 5 * 3].view(2, 3, 8, 5, 3))   # misaligned
    bad(rng=rng.long())
    bad(rng=rng.cpu())
    bad(image_camera=cam[:2])                                 # not one entry per slot
    bad(image_camera=cam.long())
    bad(image_camera=torch.tensor([0, 2, 0], dtype=torch.int32, device=dev))   # no such camera
    bad(image_camera=torch.tensor([0, -1, 0], dtype=torch.int32, device=dev))
    bad(cam_params=par[:, :8].contiguous())
    bad(cam_params=par.double())
    bad(cam_params=par.cpu())
    for col, v in ((0, 0.0), (0, 0.9), (1, 1.5), (2, 0.0), (2, 1.2), (4, -0.1), (4, 1.1),
                   (5, -1.0), (5, 1.2), (7, -0.5), (7, 1.2), (8, float("nan"))):
        p = par.clone()
        p[1, col] = v                                         # lo > hi, or outside its domain
        if (col, v) == (0, 0.9):
            p[1, 1] = 0.85
        bad(cam_params=p)
    bad(out=img)                                              # in place
    bad(out=torch.empty_like(img).float())
    bad(out=torch.empty((2, 3, 8, 8, 3), dtype=torch.uint8))  # host
    bad(params_out=torch.empty((2, 2, 7), device=dev))
    bad(params_out=torch.empty((2, 2, 8), device=dev, dtype=torch.float64))
    bad(workspace=torch.empty(16, dtype=torch.uint8, device=dev))
    bad(sample_offset=-1)
    bad(tables=([0, 1], [R.OCTO, R.OCTO]))                    # not the tensors' sizes
    # the module refuses fp32 frames and a slot count that is not its own
    aug = ImageAugmentation([{}, {}], CAMS)
    for x in (img.float(), img[:, :2].contiguous(), img.cpu()):
        with pytest.raises(ValueError):
            aug(x, rng)
    # the C ABI itself: a device-side camera index out of range is read as camera 0 and reported
    out = torch.empty_like(img)
    ws = torch.empty(K.image_augment_workspace(2, 3), dtype=torch.uint8, device=dev)
    far = torch.tensor([0, 7, 0], dtype=torch.int32, device=dev)
    _C.call("mmt_image_augment", _C.ptr(img), 2, 3, 8, 8, _C.ptr(rng), 0, _C.ptr(far), _C.ptr(par),
            2, _C.ptr(out), None, _C.ptr(ws), ws.numel(), _C.stream_ptr())
    with pytest.raises(_C.MMTError):
        K.device_status()
    K.device_status()                                         # the word is cleared by the read
