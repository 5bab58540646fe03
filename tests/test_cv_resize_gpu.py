"""GPU: the annotator's two cv2 resizes on the device (csrc/tg_cv_resize.hip: ``ops.cv_area_u8`` / ``ops.cv_linear_u8``), bit-equal to the NumPy restatement
of tests/cv_resize_reference.py, and ``LineartDetector`` on the routes that need them.

The kernels are compared for equality: the contract is integer arithmetic (INTER_LINEAR) or a fixed sequence of single fp32 operations (INTER_AREA).  The
detector as a whole carries the network's rounding: as in tests/test_lineart_gpu.py its byte map is measured against the float64 composition (restated
AREA -> float64 network -> byte step -> restated LINEAR -> invert) and must be within max(1.5 x the rounded emulation's error, floor), floor 1.0 on the mean
level error; the emulation is the same composition with the network run by torch in the storage dtype (on the device, as the 512 x 512 case of
tests/test_lineart_gpu.py does).

Beyond the listed shapes: ``[1, 4, 2001, 3] -> (2, 2000)``, where the table's 1e-3 threshold drops entries (at 1000 -> 999 it drops none, see
tests/test_cv_resize_cpu.py), and a 13-fold vertical INTER_LINEAR downscale, whose tiles do not fit the LDS stage and take the kernel's direct path."""
import functools

import numpy as np
import pytest
import torch

from tests import cv_resize_reference as CR
from tests import lineart_reference as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL_DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPES = [torch.bfloat16, torch.float16]


def _ids(dt):
    return {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dt]


def _rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _unit(u8, dtype):
    """uint8 [B, H, W, 3] (ndarray) -> byte / 255 as NCHW in dtype, on the CPU (what image_from_u8, range_mode 0, is bit-equal to)"""
    return torch.from_numpy(u8.astype(np.float32) / 255.0).permute(0, 3, 1, 2).to(dtype)


# ---- INTER_AREA ------------------------------------------------------------------------------------------------------------------------------------

AREA_CASES = [
    ((2, 64, 96, 3), (24, 36)),        # general path, 8 / 3 on both axes
    ((1, 37, 53, 3), (14, 20)),        # odd sizes, ragged tiles
    ((2, 48, 64, 3), (24, 32)),        # 2 x 2 fast path
    ((1, 48, 96, 3), (16, 24)),        # 3 x 4 fast path
    ((1, 48, 64, 3), (24, 24)),        # one axis integer: the general path
    ((1, 4, 1000, 3), (2, 999)),       # entries next to the 1e-3 thresholds
    ((1, 4, 2001, 3), (2, 2000)),      # entries the thresholds drop
    ((2, 24, 40, 3), (24, 40)),        # the identity
    ((1, 130, 70, 3), (49, 66)),       # more than one tile on both axes, several entry counts
]


@pytest.mark.parametrize("shape,size", AREA_CASES, ids=lambda v: "x".join(str(i) for i in v))
def test_area_bit_equal(shape, size):
    from theatergen_amd import ops
    img = _rand_u8(shape, 11 + shape[1])
    want = np.stack([CR.area_u8(img[b], *size) for b in range(shape[0])])
    src = torch.from_numpy(img).to(DEV)
    for dtype in ALL_DTYPES:
        x, u8 = ops.cv_area_u8(src, size, dtype, u8_out=True)
        assert x.dtype == dtype and tuple(x.shape) == (shape[0], 3, *size) and tuple(u8.shape) == (shape[0], *size, 3)
        got = u8.cpu().numpy()
        bad = got != want
        assert not bad.any(), f"{_ids(dtype)}: {int(bad.sum())} of {bad.size} bytes differ, first at {tuple(np.argwhere(bad)[0])}"
        assert torch.equal(x, ops.image_from_u8(u8, dtype, range_mode=0))
        assert torch.equal(x.cpu(), _unit(want, dtype))
        assert torch.equal(ops.cv_area_u8(src, size, dtype), x)                    # without the optional byte output


def test_area_argument_errors():
    from theatergen_amd import ops
    src = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(NotImplementedError, match="shrinking"):
        ops.cv_area_u8(src, (16, 32), torch.bfloat16)
    with pytest.raises(NotImplementedError):
        ops.cv_area_u8(torch.zeros((1, 1000, 16, 3), dtype=torch.uint8, device=DEV), (64, 16), torch.bfloat16)     # 15.6 rows per row: above the entry limit
    with pytest.raises(ValueError, match="uint8"):
        ops.cv_area_u8(src.float(), (8, 8), torch.bfloat16)


# ---- INTER_LINEAR ----------------------------------------------------------------------------------------------------------------------------------

LINEAR_CASES = [
    ((2, 24, 36, 3), (64, 96)),
    ((1, 14, 20, 3), (37, 53)),        # odd sizes: the element-wide stores
    ((1, 64, 96, 3), (24, 36)),        # a downscale
    ((1, 3, 3, 3), (8, 8)),
    ((1, 80, 40, 3), (6, 20)),         # 13.3-fold vertical downscale: a tile's rows exceed the stage, the direct path
    ((2, 20, 24, 3), (20, 24)),        # the identity
]


def _grey(shape, seed):
    g = _rand_u8(shape[:3] + (1,), seed).repeat(3, axis=3)
    return g


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "invert"])
@pytest.mark.parametrize("shape,size", LINEAR_CASES, ids=lambda v: "x".join(str(i) for i in v))
def test_linear_bit_equal(shape, size, invert):
    from theatergen_amd import ops
    v = _grey(shape, 23 + shape[1])
    assert (v[..., 0] == v[..., 1]).all() and (v[..., 0] == v[..., 2]).all()
    assert shape[1] * shape[2] < 64 or LR.distinct_levels(v) >= 64                 # a condition on the inputs (3 x 3 has nine pixels)
    if invert:
        want = np.stack([CR.annotator_tail(255 - v[b], *size) for b in range(shape[0])])      # v holds 255 - t: resize t, then invert
    else:
        want = np.stack([CR.linear_u8(v[b], *size) for b in range(shape[0])])
    src = torch.from_numpy(v).to(DEV)
    u8 = ops.cv_linear_u8(src, size, invert=invert)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (shape[0], *size, 3)
    bad = u8.cpu().numpy() != want
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} bytes differ, first at {tuple(np.argwhere(bad)[0])}"
    for dtype in ALL_DTYPES:
        both_u8, pt = ops.cv_linear_u8(src, size, invert=invert, dtype=dtype)
        assert torch.equal(both_u8, u8)
        assert pt.dtype == dtype and torch.equal(pt.cpu(), _unit(want, dtype))
        assert torch.equal(ops.cv_linear_u8(src, size, invert=invert, dtype=dtype, u8_out=False), pt)       # "pt" alone


def test_linear_argument_errors():
    from theatergen_amd import ops
    src = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="no output"):
        ops.cv_linear_u8(src, (32, 32), u8_out=False)
    with pytest.raises(ValueError, match="uint8"):
        ops.cv_linear_u8(src.float(), (32, 32))


# ---- both kernels: determinism, batch independence ------------------------------------------------------------------------------------------------------

def test_batch_independent_and_deterministic():
    from theatergen_amd import ops
    img = torch.from_numpy(_rand_u8((2, 64, 96, 3), 31)).to(DEV)
    a = ops.cv_area_u8(img, (24, 36), torch.bfloat16, u8_out=True)
    b = ops.cv_area_u8(img, (24, 36), torch.bfloat16, u8_out=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in range(2):
        one = ops.cv_area_u8(img[i:i + 1], (24, 36), torch.bfloat16, u8_out=True)
        assert torch.equal(one[0], a[0][i:i + 1]) and torch.equal(one[1], a[1][i:i + 1])
    fast = ops.cv_area_u8(img, (32, 48), torch.float16, u8_out=True)               # the block-sum kernel
    assert torch.equal(ops.cv_area_u8(img[1:2], (32, 48), torch.float16, u8_out=True)[1], fast[1][1:2])
    v = torch.from_numpy(_grey((2, 24, 36, 3), 37)).to(DEV)
    a = ops.cv_linear_u8(v, (64, 96), invert=True, dtype=torch.bfloat16)
    b = ops.cv_linear_u8(v, (64, 96), invert=True, dtype=torch.bfloat16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in range(2):
        one = ops.cv_linear_u8(v[i:i + 1], (64, 96), invert=True, dtype=torch.bfloat16)
        assert torch.equal(one[0], a[0][i:i + 1]) and torch.equal(one[1], a[1][i:i + 1])


# ---- the detector -------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _native(dtype):
    from theatergen_amd.lineart import LineartGenerator
    g = LineartGenerator()
    g.load_state_dict(LR.seeded_generator().state_dict())
    return g.to(device=DEV, dtype=dtype).eval()


def _detector(dtype, **kw):
    from theatergen_amd.lineart import LineartDetector
    return LineartDetector(_native(dtype), **kw)


def _compose(gen, img, net, out, dtype):
    """restated AREA -> the network `gen` on the storage-rounded input -> byte step -> restated LINEAR -> invert; uint8 [H, W, 3]"""
    small = CR.area_u8(img, *net)
    x = LR.preprocess(small).to(dtype)
    p = next(gen.parameters())
    line = LR.run(gen, x.to(p.dtype))[0]
    t = 255 - LR.byte_map(line)                                                    # the annotator's map before its inversion, three channels
    return CR.annotator_tail(t, *out)


@functools.lru_cache(maxsize=None)
def _case_512(dtype):
    img = LR.sample_image(3, 512, 512)
    ref = _compose(LR.rounded_copy(LR.seeded_generator(), dtype), img, (192, 192), (512, 512), dtype)             # float64 network
    # the storage-dtype network, run by torch on the device (fp16 convolutions on the host take ten seconds at this size)
    emu = _compose(LR.rounded_copy(LR.seeded_generator(), dtype, dtype).to(DEV), img, (192, 192), (512, 512), dtype)
    assert LR.distinct_levels(ref) >= 64                                           # a condition on the inputs: a near-constant map would pass anything
    return img, ref, LR.level_diff(emu, ref)


def _hand(dtype, img, net, out):
    """cv_linear_u8(generator(cv_area_u8(img))) composed by hand -> device uint8 [1, H, W, 3]"""
    from theatergen_amd import ops
    x = ops.cv_area_u8(torch.from_numpy(img).to(DEV)[None], net, dtype)
    return ops.cv_linear_u8(_native(dtype)(x), out, invert=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_detector_512_at_192_against_float64(dtype):
    img, ref, (e_mean, e_max) = _case_512(dtype)
    got = _detector(dtype)(img, detect_resolution=192, image_resolution=512, output_type="np")
    assert got.shape == (512, 512, 3) and got.dtype == np.uint8
    mean, mx = LR.level_diff(got, ref)
    print(f"lineart detector {_ids(dtype)} 512 x 512 at 192 / 512: native mean {mean:.4f} max {mx} | emulation mean {e_mean:.4f} max {e_max}")
    assert mean <= max(1.5 * e_mean, 1.0) and mx <= max(1.5 * e_max, 0.0), (mean, mx, e_mean, e_max)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_detector_consistency(dtype):
    from PIL import Image
    from theatergen_amd import pipelines
    imgs = [LR.sample_image(3, 512, 512), LR.sample_image(4, 512, 512)]
    det = _detector(dtype)
    kw = dict(detect_resolution=192, image_resolution=512)
    pil = det(imgs[0], **kw)
    assert isinstance(pil, Image.Image) and pil.mode == "RGB" and pil.size == (512, 512)
    got = np.asarray(pil)
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
    assert np.array_equal(got, _hand(dtype, imgs[0], (192, 192), (512, 512))[0].cpu().numpy())
    assert np.array_equal(det(imgs[0], output_type="np", **kw), got)
    pt = det(imgs[0], output_type="pt", **kw)
    assert pt.is_cuda and pt.dtype == dtype and tuple(pt.shape) == (1, 3, 512, 512)
    assert torch.equal(pt.cpu(), _unit(got[None], dtype))
    assert torch.equal(_detector(dtype, output_type="pt")(imgs[0], **kw), pt)
    many = det.detect_many(imgs, **kw)
    assert np.array_equal(np.asarray(many[0]), got) and np.array_equal(np.asarray(many[1]), np.asarray(det(imgs[1], **kw)))
    many_pt = det.detect_many(imgs, output_type="pt", **kw)
    assert torch.equal(many_pt[0], pt) and tuple(many_pt[1].shape) == (1, 3, 512, 512)
    assert pipelines._adapter_image(pt, 512, 512) is pt                            # the SDXL branch takes the "pt" output as given


def test_detector_workload_shape():
    """the SDXL call: a 1024 x 1024 image at detect_resolution = 384, image_resolution = 1024 (the network at 384 x 384: transposed convs 96 and 192 wide)"""
    dtype = torch.bfloat16
    img = LR.sample_image(5, 1024, 1024)
    det = _detector(dtype)
    a = det(img, detect_resolution=384, image_resolution=1024, output_type="np")
    assert a.shape == (1024, 1024, 3) and a.dtype == np.uint8
    assert LR.distinct_levels(a) >= 64
    assert np.array_equal(det(img, detect_resolution=384, image_resolution=1024, output_type="np"), a)
    assert np.array_equal(_hand(dtype, img, (384, 384), (1024, 1024))[0].cpu().numpy(), a)
    pt = det(img, detect_resolution=384, image_resolution=1024, output_type="pt")
    assert tuple(pt.shape) == (1, 3, 1024, 1024) and torch.equal(pt.cpu(), _unit(a[None], dtype))


@pytest.mark.parametrize("h,w,net", [(128, 192, (64, 128)), (128, 256, (64, 128))], ids=["2x1.5", "2x2"])
def test_detector_route_without_linear_launch(h, w, net):
    """detect 64 / image 64: INTER_AREA in front (128 x 256: the 2 x 2 block path; 128 x 192 halves the rows and takes two thirds of the columns), the
    output size equals the network size: the bytes are the generator's on the AREA result, nothing behind it"""
    from theatergen_amd import ops
    from theatergen_amd.lineart import plan_resizes
    dtype = torch.bfloat16
    plan = plan_resizes(h, w, 64, 64)
    assert plan.net == net and plan.out == net and plan.area and not plan.linear
    img = LR.sample_image(6, h, w)
    got = _detector(dtype)(img, detect_resolution=64, image_resolution=64, output_type="np")
    small = CR.area_u8(img, *net)
    want = _native(dtype)(ops.image_from_u8(torch.from_numpy(small).to(DEV)[None], dtype, range_mode=0))
    assert np.array_equal(got, want[0].cpu().numpy())
    pt = _detector(dtype)(img, detect_resolution=64, image_resolution=64, output_type="pt")
    assert torch.equal(pt.cpu(), _unit(got[None], dtype))


def test_detector_identity_route_is_unchanged():
    """512 / 512 on a 64-multiple image: no resize launch, the generator's bytes as before"""
    from theatergen_amd import ops
    dtype = torch.bfloat16
    img = LR.sample_image(7, 64, 128)
    got = _detector(dtype)(img, detect_resolution=64, image_resolution=64, output_type="np")
    want = _native(dtype)(ops.image_from_u8(torch.from_numpy(img).to(DEV)[None], dtype, range_mode=0))
    assert np.array_equal(got, want[0].cpu().numpy())
