"""GPU: the lineart annotator on the device (theatergen_amd/lineart.py, csrc/tg_lineart.hip) against the float64 restatement of tests/lineart_reference.py.

Per-layer tolerances are worked out from the number formats: one rounding to the storage dtype (half an ulp: 2^-8 relative in bf16, 2^-11 in fp16) plus
the worst case of a length-K fp32 sum, K * 2^-24 * sum |a| |b|.  The whole-network bound is not fixed in advance: the same restatement run by torch on the
CPU in the storage dtype (the rounded emulation) is measured against float64, and the native result must be within 1.5 x its error (other summation order,
other rounding points), with a floor of one level on the mean of the byte map.

Measured on MI355X (native / emulation; relative L2 of the sigmoid map, mean and max level difference of the byte map): profiles/lineart_findings.md."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lineart_reference as LR

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24
DEV = "cuda"


def _ids(dt):
    return "bf16" if dt == torch.bfloat16 else "fp16"


def _randn(shape, seed, dtype, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale + shift).to(dtype)


def _check(got, ref, dtype, extra_abs):
    """|got - ref| <= half an ulp of the storage dtype at ref + extra_abs (scalar or tensor), everywhere"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    tol = HALF_ULP[dtype] * ref.abs() + extra_abs
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} off; worst {float(((got - ref).abs() - tol).max()):.3e} over the tolerance"


@functools.lru_cache(maxsize=None)
def _native(dtype):
    from theatergen_amd.lineart import LineartGenerator
    g = LineartGenerator()
    g.load_state_dict(LR.seeded_generator().state_dict())
    return g.to(device=DEV, dtype=dtype).eval()


@functools.lru_cache(maxsize=None)
def _oracle(dtype):
    return LR.rounded_copy(LR.seeded_generator(), dtype)                       # float64, storage-rounded weights


@functools.lru_cache(maxsize=None)
def _emulation(dtype, device="cpu"):
    return LR.rounded_copy(LR.seeded_generator(), dtype, dtype).to(device)


@functools.lru_cache(maxsize=None)
def _case(dtype, B, H, W):
    """(images uint8 list, x storage dtype NCHW on the CPU, float64 maps [B, H, W], float64 byte maps, emulation errors per image)"""
    imgs = [LR.sample_image(s, H, W) for s in range(B)]
    x = torch.cat([LR.preprocess(i) for i in imgs]).to(dtype)
    ref = LR.run(_oracle(dtype), x.double())
    em = LR.run(_emulation(dtype), x)
    ref_u8 = [LR.byte_map(ref[b]) for b in range(B)]
    errs = []
    for b in range(B):
        assert LR.distinct_levels(ref_u8[b]) >= 64                              # a condition on the inputs: a near-constant map would pass anything
        errs.append((LR.rel_l2(em[b], ref[b]),) + LR.level_diff(LR.byte_map(em[b]), ref_u8[b]))
    return imgs, x, ref, ref_u8, errs


# ---- InstanceNorm (+ ReLU, + residual) alone ------------------------------------------------------------------------------------------------------

def _in_input(B, hw, c, dtype, seed):
    x = _randn((B, hw, c), seed, torch.float64, scale=1.5, shift=0.3)
    x *= torch.linspace(0.5, 2.0, B, dtype=torch.float64)[:, None, None]        # distinct images
    x[:, :, 0] = torch.arange(1, B + 1, dtype=torch.float64)[:, None] * 0.75    # zero variance
    x[:, :, 1] = 64.0 + _randn((B, hw), seed + 1, torch.float64)                # |mean| >> std
    return x.to(dtype)


def _in_ref(x, relu, res):
    x = x.double()
    mean, var = x.mean(dim=1, keepdim=True), x.var(dim=1, unbiased=False, keepdim=True)
    y = (x - mean) / torch.sqrt(var + 1e-5)
    if relu:
        y = y.clamp_min(0)
    return y + res.double() if res is not None else y


# fp32 statistics: the mean within a few ulps of fp32 at |mean| <= 64 (4e-6 * 8), the scale within 1e-6 relative of values <= ~6 standard deviations
IN_ABS = 1e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("B,h,w", [(2, 24, 40), (1, 128, 192)])
@pytest.mark.parametrize("relu,with_res", [(False, False), (True, False), (False, True)])
def test_instnorm_dense(dtype, B, h, w, relu, with_res):
    from theatergen_amd import ops
    x = _in_input(B, h * w, 64, dtype, 3)
    res = _randn((B, h * w, 64), 5, dtype) if with_res else None
    got = ops.lineart_instnorm(x.to(DEV).reshape(-1, 64), B, h, w, 64, relu=relu, res=res.to(DEV).reshape(-1, 64) if with_res else None)
    ref = _in_ref(x, relu, res)
    # the residual is added in fp32 before the one rounding
    _check(got.reshape(B, h * w, 64), ref, dtype, IN_ABS)
    if not relu and not with_res:
        assert bool((got.reshape(B, h * w, 64)[:, :, 0] == 0).all())             # zero variance: exactly 0, not NaN


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("c,h,w", [(256, 4, 6), (128, 6, 10)])
def test_instnorm_layouts(dtype, c, h, w):
    """the reflect-bordered input / residual / output and the parity-class input address the same pixels as the dense layout"""
    from theatergen_amd import ops
    B = 2
    x = _in_input(B, h * w, c, dtype, 11).reshape(B, h, w, c)
    res = _randn((B, h, w, c), 13, dtype)
    ref = _in_ref(x.reshape(B, h * w, c), True, res.reshape(B, h * w, c)).reshape(B, h, w, c)
    pad = lambda t: F.pad(t.double().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1)
    junk = lambda t: (F.pad(t.double(), (0, 0, 1, 1, 1, 1), value=777.0)).to(dtype)          # a border the kernel must not read
    xd = x.to(DEV)
    # bordered input + bordered residual -> bordered output
    got = ops.lineart_instnorm(junk(x).to(DEV).reshape(-1, c), B, h, w, c, layout=ops.LINEART_BORDER, relu=True, res=junk(res).to(DEV).reshape(-1, c),
                               res_layout=ops.LINEART_BORDER, border=True).reshape(B, h + 2, w + 2, c)
    _check(got, pad(ref), dtype, IN_ABS)
    inner = got[:, 1:-1, 1:-1]
    assert torch.equal(got, F.pad(inner.float().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1).to(dtype))   # the border is a copy
    dense = ops.lineart_instnorm(xd.reshape(-1, c), B, h, w, c, relu=True, res=res.to(DEV).reshape(-1, c)).reshape(B, h, w, c)
    assert torch.equal(inner, dense)
    # parity-class input [B, (h/2)(w/2), 4 c]
    par = x.reshape(B, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).contiguous().to(DEV)
    got = ops.lineart_instnorm(par.reshape(-1, 4 * c), B, h, w, c, layout=ops.LINEART_PARITY, relu=True, res=res.to(DEV).reshape(-1, c)).reshape(B, h, w, c)
    assert torch.equal(got, dense)


# ---- each conv form alone -------------------------------------------------------------------------------------------------------------------------

def _sum_tol(x_abs_conv, K):
    return K * U32 * x_abs_conv


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("h,w", [(4, 6), (8, 12)])
def test_reflect_conv3x3(dtype, h, w):
    """ReflectionPad2d(1) + Conv2d(256, 256, 3): the InstanceNorm apply pass writes the reflect-bordered image, the pad-1 conv runs on it, interior read"""
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_conv3x3
    B, c = 2, 256
    z = _randn((B, h * w, c), 21, dtype).to(DEV)
    wt = _randn((c, c, 3, 3), 22, dtype, scale=0.03)
    bias = _randn((c,), 23, dtype, scale=0.1)
    zb = ops.lineart_instnorm(z.reshape(-1, c), B, h, w, c, relu=True, border=True)                      # [B (h+2)(w+2), c]
    y = _native(dtype)._conv3x3(zb, pack_conv3x3(wt).to(DEV), B, h + 2, w + 2, c, bias.to(DEV))
    got = y.reshape(B, h + 2, w + 2, c)[:, 1:-1, 1:-1]
    zn = zb.reshape(B, h + 2, w + 2, c)[:, 1:-1, 1:-1].double().cpu().permute(0, 3, 1, 2)                # the values as stored
    zp = F.pad(zn, (1, 1, 1, 1), mode="reflect")
    ref = F.conv2d(zp, wt.double(), bias.double()).permute(0, 2, 3, 1)
    mag = F.conv2d(zp.abs(), wt.double().abs(), bias.double().abs()).permute(0, 2, 3, 1)
    _check(got, ref, dtype, _sum_tol(mag, 9 * c))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_conv7_in(dtype):
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_conv7x7_fp32
    B, h, w = 2, 16, 24
    x = torch.rand((B, 3, h, w), generator=torch.Generator().manual_seed(31), dtype=torch.float64).to(dtype)
    wt = _randn((64, 3, 7, 7), 32, dtype, scale=0.1)
    bias = _randn((64,), 33, dtype, scale=0.1)
    got = ops.lineart_conv7_in(x.to(DEV), pack_conv7x7_fp32(wt).to(DEV), bias.float().to(DEV)).reshape(B, h, w, 64)
    xp = F.pad(x.double(), (3, 3, 3, 3), mode="reflect")
    ref = F.conv2d(xp, wt.double(), bias.double()).permute(0, 2, 3, 1)
    mag = F.conv2d(xp.abs(), wt.double().abs(), bias.double().abs()).permute(0, 2, 3, 1)
    _check(got, ref, dtype, _sum_tol(mag, 147))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_conv7_out(dtype):
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_conv7x7_to1_fp32
    B, h, w = 2, 16, 24
    x = _randn((B, h, w, 64), 41, dtype).clamp_min(0)
    wt = _randn((1, 64, 7, 7), 42, dtype, scale=0.03)
    bias = float(_randn((1,), 43, dtype, scale=0.1)[0])
    u8, sig = ops.lineart_conv7_out(x.to(DEV).reshape(-1, 64), B, h, w, pack_conv7x7_to1_fp32(wt).to(DEV), bias, want_sigmoid=True)
    xp = F.pad(x.double().permute(0, 3, 1, 2), (3, 3, 3, 3), mode="reflect")
    pre = F.conv2d(xp, wt.double()) + bias
    mag = F.conv2d(xp.abs(), wt.double().abs()) + abs(bias)
    ref = torch.sigmoid(pre)[:, 0]
    # sigmoid' <= 1/4; the fp32 exp / division add a few ulps of fp32 at values <= 1
    tol = 0.25 * _sum_tol(mag[:, 0], 3136) + 4 * U32
    assert bool(((sig.double().cpu() - ref).abs() <= tol).all())
    u8, sig = u8.cpu().numpy(), sig.cpu().numpy()
    assert (u8[..., 0] == u8[..., 1]).all() and (u8[..., 0] == u8[..., 2]).all()
    want = 255 - np.clip((sig * np.float32(255.0)).astype(np.int64), 0, 255)
    assert (u8[..., 0] == want).all()                                             # the byte step on the kernel's own sigmoid: truncation, 255 - m
    ref_u8 = 255 - np.clip((ref.numpy() * 255.0), 0, 255).astype(np.uint8).astype(np.int64)
    diff = np.abs(u8[..., 0].astype(np.int64) - ref_u8)
    assert diff.max() <= 1
    frac = ref.numpy() * 255.0
    near = np.abs(frac - np.round(frac)) <= 255.0 * tol.numpy() + 255.0 * 2 * U32
    assert (near | (diff == 0)).all()                                             # a level differs only where 255 s sits on an integer within the tolerance


def _unshuffle(y, layout, B, h, w, n):
    """the transposed conv's result as an image [B, 2h, 2w, n] (test-side view of the parity-class layout)"""
    from theatergen_amd import ops
    if layout == ops.LINEART_DENSE:
        return y.reshape(B, 2 * h, 2 * w, n)
    return y.reshape(B, h, w, 2, 2, n).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("cin,cout,h,w,route", [(256, 128, 4, 6, "conv3x3"), (128, 64, 4, 6, "conv3x3"), (256, 128, 8, 16, "up2"), (128, 64, 8, 16, "up2")])
def test_transposed_conv(dtype, cin, cout, h, w, route):
    from theatergen_amd import ops
    B = 2
    gen = _native(dtype)
    conv = gen.model3[0] if cin == 256 else gen.model3[3]
    x = _randn((B, h, w, cin), 51, dtype).clamp_min(0)
    y, layout = gen.conv_transpose(f"t_{cin}", conv, x.to(DEV).reshape(-1, cin), B, h, w)
    assert layout == (ops.LINEART_DENSE if route == "up2" else ops.LINEART_PARITY)
    got = _unshuffle(y, layout, B, h, w, cout)
    wt, bias = conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu()
    xn = x.double().permute(0, 3, 1, 2)
    ref = F.conv_transpose2d(xn, wt, bias, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    mag = F.conv_transpose2d(xn.abs(), wt.abs(), bias.abs(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    _check(got, ref, dtype, _sum_tol(mag, 4 * cin))


# ---- the whole generator ----------------------------------------------------------------------------------------------------------------------------

def _within(native, emu, floor=0.0):
    return native <= max(1.5 * emu, floor)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("B,H,W", [(1, 32, 48), (2, 64, 64), (1, 128, 192)])
def test_generator_against_float64(dtype, B, H, W):
    imgs, x, ref, ref_u8, errs = _case(dtype, B, H, W)
    u8, sig = _native(dtype)(x.to(DEV), want_sigmoid=True)
    u8, sig = u8.cpu().numpy(), sig.cpu()
    for b in range(B):
        l2 = LR.rel_l2(sig[b], ref[b])
        mean, mx = LR.level_diff(u8[b], ref_u8[b])
        e_l2, e_mean, e_max = errs[b]
        print(f"lineart {_ids(dtype)} [{B},3,{H},{W}] image {b}: native relL2 {l2:.3e} mean {mean:.4f} max {mx} | emulation relL2 {e_l2:.3e} "
              f"mean {e_mean:.4f} max {e_max}")
        assert _within(l2, e_l2) and _within(mean, e_mean, 1.0) and _within(mx, e_max), (l2, mean, mx, errs[b])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_generator_is_deterministic_and_batch_independent(dtype):
    imgs, x, *_ = _case(dtype, 2, 64, 64)
    gen = _native(dtype)
    a = gen(x.to(DEV), want_sigmoid=True)
    b = gen(x.to(DEV), want_sigmoid=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    one = gen(x[1:2].to(DEV), want_sigmoid=True)
    assert torch.equal(a[0][1:2], one[0]) and torch.equal(a[1][1:2], one[1])


# ---- LineartDetector end to end -----------------------------------------------------------------------------------------------------------------------

def _detector(dtype):
    from theatergen_amd.lineart import LineartDetector
    return LineartDetector(_native(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_detector_64(dtype):
    from PIL import Image
    from theatergen_amd import pipelines
    imgs, x, ref, ref_u8, errs = _case(dtype, 2, 64, 64)
    det = _detector(dtype)
    pil = det(imgs[0], detect_resolution=64, image_resolution=64)
    assert isinstance(pil, Image.Image) and pil.mode == "RGB" and pil.size == (64, 64)
    got = np.asarray(pil)
    mean, mx = LR.level_diff(got, ref_u8[0])
    assert _within(mean, errs[0][1], 1.0) and _within(mx, errs[0][2]), (mean, mx, errs[0])
    # "pt": the same bytes as map / 255 in the model dtype, [1, 3, H, W] on the device; per call or as the instance default
    pt = det(imgs[0], detect_resolution=64, image_resolution=64, output_type="pt")
    assert pt.is_cuda and pt.dtype == dtype and tuple(pt.shape) == (1, 3, 64, 64)
    want = (torch.from_numpy(got.astype(np.float32) / 255.0).permute(2, 0, 1)[None]).to(dtype)
    assert torch.equal(pt.cpu(), want)
    from theatergen_amd.lineart import LineartDetector
    assert torch.equal(LineartDetector(_native(dtype), output_type="pt")(imgs[0], detect_resolution=64, image_resolution=64), pt)
    # input forms: PIL image, device uint8 tensor, grey
    assert np.array_equal(np.asarray(det(Image.fromarray(imgs[0]), detect_resolution=64, image_resolution=64)), got)
    assert np.array_equal(np.asarray(det(torch.from_numpy(imgs[0]).to(DEV), detect_resolution=64, image_resolution=64)), got)
    grey = imgs[0][:, :, 0]
    assert np.array_equal(np.asarray(det(grey, detect_resolution=64, image_resolution=64)),
                          np.asarray(det(np.stack([grey] * 3, axis=2), detect_resolution=64, image_resolution=64)))
    # detect_many = the single calls
    many = det.detect_many(imgs, detect_resolution=64, image_resolution=64)
    assert np.array_equal(np.asarray(many[0]), got)
    assert np.array_equal(np.asarray(many[1]), np.asarray(det(imgs[1], detect_resolution=64, image_resolution=64)))
    # stage 2 takes the "pt" output as it is when the pipeline object has no prepare_image
    ctl = pipelines._control_image(object(), pt, 64, 64, torch.device(DEV), dtype)
    assert tuple(ctl.shape) == (2, 3, 64, 64) and torch.equal(ctl[0], pt[0]) and torch.equal(ctl[1], pt[0])
    with pytest.raises(ValueError, match="coarse"):
        det(imgs[0], coarse=True, detect_resolution=64, image_resolution=64)
    with pytest.raises(NotImplementedError):
        det(imgs[0])                                                               # 64 x 64 at the default 512 / 512 would need cv2's resize


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_detector_512(dtype):
    """One 512 x 512 image at the defaults.  Oracle: the storage-dtype emulation run by torch on the device (float64 at this size is left out to keep the
    test short).  Both carry their own error against the exact map: the emulation's mean level error e is taken from the 128 x 192 case (the error per
    pixel depends on the receptive field, not on the image size), the native one is bounded by max(1.5 e, 1) there, so the two differ by at most their sum."""
    img = LR.sample_image(7, 512, 512)
    det = _detector(dtype)
    pil = det(img)
    assert pil.size == (512, 512)
    got = np.asarray(pil)
    em = LR.run(_emulation(dtype, DEV), LR.preprocess(img).to(dtype))
    em_u8 = LR.byte_map(em[0])
    assert LR.distinct_levels(em_u8) >= 64
    e_mean = _case(dtype, 1, 128, 192)[4][0][1]
    mean, mx = LR.level_diff(got, em_u8)
    print(f"lineart {_ids(dtype)} 512 x 512: native vs device emulation mean {mean:.4f} max {mx}; emulation's own mean error at 128 x 192 {e_mean:.4f}")
    assert mean <= max(1.5 * e_mean, 1.0) + e_mean, (mean, e_mean)
    pt = det(img, output_type="pt")
    assert torch.equal(pt.cpu(), (torch.from_numpy(got.astype(np.float32) / 255.0).permute(2, 0, 1)[None]).to(dtype))
