"""The lineart annotator on the device: stage 2's ControlNet control image (reference ``generate.py:96,132``:
``controlnet_aux.LineartDetector.from_pretrained("lllyasviel/Annotators")``; called as ``processor(np.array(input_img))``, ``models/pipelines.py:711``).

``LineartGenerator`` is controlnet_aux's ``Generator(input_nc=3, output_nc=1, n_residual_blocks=3, sigmoid=True)`` with its parameter names, so an
``sk_model.pth`` / ``sk_model2.pth`` state dict loads with ``load_state_dict``:

    model0  ReflectionPad2d(3), Conv2d(3, 64, 7), InstanceNorm2d, ReLU
    model1  Conv2d(64, 128, 3, s2, p1), IN, ReLU, Conv2d(128, 256, 3, s2, p1), IN, ReLU
    model2  3 x ResidualBlock: x + [ReflectionPad2d(1), Conv2d(256, 256, 3), IN, ReLU, ReflectionPad2d(1), Conv2d(256, 256, 3), IN](x)
    model3  ConvTranspose2d(256, 128, 3, s2, p1, op1), IN, ReLU, ConvTranspose2d(128, 64, 3, s2, p1, op1), IN, ReLU
    model4  ReflectionPad2d(3), Conv2d(64, 1, 7), Sigmoid

Device route (no torch arithmetic; activations token-major NHWC in the storage dtype):
  * the two 7x7 convs and every InstanceNorm (+ ReLU, + residual) are the kernels of csrc/tg_lineart.hip;
  * ReflectionPad2d(1) is address arithmetic in the InstanceNorm apply pass, which writes the reflect-bordered image; the existing pad-1 ``ops.conv3x3``
    runs over that (h + 2) x (w + 2) image and the next InstanceNorm reads the interior of its result;
  * the stride-2 convs are ``ops.conv3x3(stride=2)``;
  * a transposed conv is ``ops.conv_up2`` on ``pack_convT3x3_s2_up2`` weights where tg_conv_up2 takes the geometry (low-resolution width 8 .. 64); elsewhere
    (512 x 512: widths 128 and 256) it is one pad-1 ``ops.conv3x3`` on the low-resolution grid with 4 N output channels, one block of N per output parity
    class (``pack_convT3x3_s2_conv3x3``: the unused taps are zero weights), and the following InstanceNorm reads that layout: no pixel-shuffle pass.

``LineartDetector`` is the annotator's ``__call__`` for every call whose detect step shrinks the image or leaves its size alone (``detect_resolution`` <=
the short side): ``cv2.resize(..., INTER_AREA)`` in front of the network and ``cv2.resize(..., INTER_LINEAR)`` + ``255 - map`` behind it are the kernels
of csrc/tg_cv_resize.hip, in the arithmetic of OpenCV's portable C++ path as include/theatergen_hip.h restates it (written from resize.cpp, not run
against a cv2 build).  The SD-1.5 / SD-2.1 flow (a 512 x 512 image at 512 / 512) needs neither and runs as before; the SDXL flow (1024 x 1024 at
``detect_resolution=384, image_resolution=1024``) needs both.  A ``detect_resolution`` above the short side would need LANCZOS4 pixels and raises
NotImplementedError.
"""
import collections

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .unet import _Packed
from .weights_pack import pack_conv3x3, pack_conv7x7_fp32, pack_conv7x7_to1_fp32, pack_convT3x3_s2_conv3x3, pack_convT3x3_s2_up2


class ResidualBlock(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv_block = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(channels, channels, 3), nn.InstanceNorm2d(channels), nn.ReLU(inplace=True),
                                        nn.ReflectionPad2d(1), nn.Conv2d(channels, channels, 3), nn.InstanceNorm2d(channels))


class LineartGenerator(nn.Module):
    """Parameters as in controlnet_aux (``model0.1``, ``model1.{0,3}``, ``model2.{i}.conv_block.{1,5}``, ``model3.{0,3}``, ``model4.1``); GPU only."""

    def __init__(self, input_nc=3, output_nc=1, n_residual_blocks=3):
        super().__init__()
        if input_nc != 3 or output_nc != 1:
            raise NotImplementedError("LineartGenerator: the device kernels are built for input_nc = 3, output_nc = 1")
        self.model0 = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(3, 64, 7), nn.InstanceNorm2d(64), nn.ReLU(inplace=True))
        self.model1 = nn.Sequential(nn.Conv2d(64, 128, 3, stride=2, padding=1), nn.InstanceNorm2d(128), nn.ReLU(inplace=True),
                                    nn.Conv2d(128, 256, 3, stride=2, padding=1), nn.InstanceNorm2d(256), nn.ReLU(inplace=True))
        self.model2 = nn.Sequential(*[ResidualBlock(256) for _ in range(n_residual_blocks)])
        self.model3 = nn.Sequential(nn.ConvTranspose2d(256, 128, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(128), nn.ReLU(inplace=True),
                                    nn.ConvTranspose2d(128, 64, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(64), nn.ReLU(inplace=True))
        self.model4 = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(64, 1, 7), nn.Sigmoid())
        self._p = _Packed()

    @property
    def dtype(self):
        return self.model0[1].weight.dtype

    @property
    def device(self):
        return self.model0[1].weight.device

    # ---- packed weights (once per weight version) -------------------------------------------------------------------------------------------------
    def _conv3(self, name, conv):
        return self._p.get(name, [conv.weight], lambda: pack_conv3x3(conv.weight.detach()))

    def _conv7_in(self):
        c = self.model0[1]
        return self._p.get("c7in", [c.weight, c.bias], lambda: (pack_conv7x7_fp32(c.weight), c.bias.detach().float().contiguous()))

    def _conv7_out(self):
        c = self.model4[1]
        return self._p.get("c7out", [c.weight, c.bias], lambda: (pack_conv7x7_to1_fp32(c.weight), float(c.bias.detach().float().item())))

    @staticmethod
    def _conv3x3(x, wp, b, h, w, cin, bias, stride=1):
        """pad-1 3x3 conv, ONE LAUNCH PER IMAGE: tg_gemm's plan (tile, K split) is a function of the launch's M, so a batched launch could sum in another
        order than the single-image call; per image, an image's bytes do not depend on the batch it is in.  At 512 x 512 one image already fills the chip."""
        oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
        out = torch.empty((b * oh * ow, wp.shape[0]), dtype=x.dtype, device=x.device)
        for i in range(b):
            ops.conv3x3(x[i * h * w:(i + 1) * h * w], wp, 1, h, w, cin, stride=stride, bias=bias, out=out[i * oh * ow:(i + 1) * oh * ow])
        return out

    def conv_transpose(self, name, conv, x, b, h, w):
        """One stride-2 transposed conv over token-major x [b * h * w, cin] -> (tensor, layout for ``ops.lineart_instnorm``) of the 2h x 2w result"""
        cin, cout = conv.in_channels, conv.out_channels
        if ops.conv_up2_eligible(x.dtype, 1, h, w, cin, cout):
            wf = self._p.get(name + "_up2", [conv.weight], lambda: pack_convT3x3_s2_up2(conv.weight))
            out = torch.empty((4 * b * h * w, cout), dtype=x.dtype, device=x.device)
            for i in range(b):
                ops.conv_up2(x[i * h * w:(i + 1) * h * w], wf, 1, h, w, cin, bias=conv.bias, out=out[4 * i * h * w:4 * (i + 1) * h * w])
            return out, ops.LINEART_DENSE
        wf, bias4 = self._p.get(name + "_c3", [conv.weight, conv.bias],
                                lambda: (pack_convT3x3_s2_conv3x3(conv.weight), conv.bias.detach().repeat(4).contiguous()))
        return self._conv3x3(x, wf, b, h, w, cin, bias4), ops.LINEART_PARITY

    def residual_block(self, i, xb, b, h, w, border_out):
        """``x + conv_block(x)`` on the reflect-bordered image xb [b * (h + 2) * (w + 2), 256] -> bordered (``border_out``) or dense result"""
        blk = self.model2[i].conv_block
        c = blk[1].out_channels
        y = self._conv3x3(xb, self._conv3(f"m2_{i}_1", blk[1]), b, h + 2, w + 2, c, blk[1].bias)
        z = ops.lineart_instnorm(y, b, h, w, c, layout=ops.LINEART_BORDER, relu=True, border=True)
        y = self._conv3x3(z, self._conv3(f"m2_{i}_5", blk[5]), b, h + 2, w + 2, c, blk[5].bias)
        return ops.lineart_instnorm(y, b, h, w, c, layout=ops.LINEART_BORDER, res=xb, res_layout=ops.LINEART_BORDER, border=border_out)

    @torch.no_grad()
    def forward(self, x, want_sigmoid=False):
        """x: NCHW [B, 3, H, W] in [0, 1], the model dtype, on the device; H, W multiples of 4, >= 8.  -> uint8 RGB [B, H, W, 3] holding
        ``255 - trunc(255 * sigmoid map)`` three times; with ``want_sigmoid`` also the fp32 sigmoid map [B, H, W]."""
        ops._need_cuda(x)
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != self.dtype:
            raise ValueError(f"LineartGenerator: {self.dtype} [B, 3, H, W] expected, got {x.dtype} {tuple(x.shape)}")
        B, _, H, W = x.shape
        if len(self.model2) == 0:
            raise NotImplementedError("LineartGenerator: n_residual_blocks = 0 is not built")
        if H % 4 or W % 4 or H < 8 or W < 8:
            raise ValueError(f"LineartGenerator: H, W must be multiples of 4 and >= 8 (two stride-2 levels, reflection in the trunk), got {H} x {W}")
        h2, w2, h4, w4 = H // 2, W // 2, H // 4, W // 4
        w0, b0 = self._conv7_in()
        a = ops.lineart_conv7_in(x, w0, b0)
        a = ops.lineart_instnorm(a, B, H, W, 64, relu=True)
        m1 = self.model1
        a = self._conv3x3(a, self._conv3("m1_0", m1[0]), B, H, W, 64, m1[0].bias, stride=2)
        a = ops.lineart_instnorm(a, B, h2, w2, 128, relu=True)
        a = self._conv3x3(a, self._conv3("m1_3", m1[3]), B, h2, w2, 128, m1[3].bias, stride=2)
        a = ops.lineart_instnorm(a, B, h4, w4, 256, relu=True, border=True)
        n = len(self.model2)
        for i in range(n):
            a = self.residual_block(i, a, B, h4, w4, border_out=i + 1 < n)
        m3 = self.model3
        a, lay = self.conv_transpose("m3_0", m3[0], a, B, h4, w4)
        a = ops.lineart_instnorm(a, B, h2, w2, 128, layout=lay, relu=True)
        a, lay = self.conv_transpose("m3_3", m3[3], a, B, h2, w2)
        a = ops.lineart_instnorm(a, B, H, W, 64, layout=lay, relu=True)
        w4p, b4 = self._conv7_out()
        return ops.lineart_conv7_out(a, B, H, W, w4p, b4, want_sigmoid=want_sigmoid)


def resized_size(h, w, resolution):
    """(H, W) controlnet_aux's ``resize_image`` gives an h x w image: the short side scaled to ``resolution``, both sides rounded to multiples of 64"""
    k = float(resolution) / min(h, w)
    return int(round(h * k / 64.0)) * 64, int(round(w * k / 64.0)) * 64


def check_identity_resize(h, w, detect_resolution, image_resolution):
    """The predicate of the route with no resize launch: both of the annotator's cv2 resizes are the identity; anything else raises NotImplementedError
    (``plan_resizes`` is what the detector asks; this stays for callers that need exactly the identity case)"""
    for what, res in (("detect_resolution", detect_resolution), ("image_resolution", image_resolution)):
        got = resized_size(h, w, res)
        if got != (h, w):
            raise NotImplementedError(
                f"LineartDetector: {what}={res} would resize the {h} x {w} image to {got[0]} x {got[1]} with cv2's LANCZOS4 / AREA filters, which are "
                "not built here (only the identity case: sides that are multiples of 64 with the short side equal to both resolutions)")


LineartPlan = collections.namedtuple("LineartPlan", "net out area linear")


def plan_resizes(h, w, detect_resolution, image_resolution):
    """The annotator's two resizes for an h x w image -> ``LineartPlan(net, out, area, linear)``: ``net`` = (H, W) of ``resize_image(image,
    detect_resolution)``, what the network runs at; ``out`` = (H, W) of ``resize_image(<that image>, image_resolution)``, what the map is resized to (the
    annotator computes that second image only for its shape); ``area`` / ``linear``: whether the INTER_AREA launch in front of the network and the
    INTER_LINEAR launch behind it are needed (a size that does not change needs none: the identity case keeps its launches and its bytes).
    ``resize_image`` takes INTER_AREA when its factor k = resolution / short side is <= 1 and LANCZOS4 otherwise; LANCZOS4 pixels are needed only at the
    detect step (k > 1 there: NotImplementedError), and so is an INTER_AREA call that grows an axis (k < 1 with a side rounded up to a multiple of 64)."""
    h, w = int(h), int(w)
    if float(detect_resolution) / min(h, w) > 1:
        got = resized_size(h, w, detect_resolution)
        raise NotImplementedError(
            f"LineartDetector: detect_resolution={detect_resolution} is above the short side of the {h} x {w} image: the annotator would enlarge it to "
            f"{got[0]} x {got[1]} with cv2's LANCZOS4 filter, which is not built here (INTER_AREA in front of the network and INTER_LINEAR behind it are)")
    net = resized_size(h, w, detect_resolution)
    if net[0] < 64 or net[1] < 64:
        raise ValueError(f"LineartDetector: detect_resolution={detect_resolution} gives a {net[0]} x {net[1]} network input for the {h} x {w} image")
    if net[0] > h or net[1] > w:
        raise NotImplementedError(
            f"LineartDetector: detect_resolution={detect_resolution} rounds the {h} x {w} image to {net[0]} x {net[1]}: cv2's INTER_AREA on a growing axis "
            "(where it interpolates linearly) is not built here")
    out = resized_size(net[0], net[1], image_resolution)
    if out[0] < 1 or out[1] < 1:
        raise ValueError(f"LineartDetector: image_resolution={image_resolution} gives a {out[0]} x {out[1]} control image")
    return LineartPlan(net, out, net != (h, w), out != net)


def _to_u8_hwc3(image, device):
    """ndarray / PIL image / device tensor, HWC uint8 (grey, RGB or RGBA) -> device uint8 [H, W, 3] (controlnet_aux ``HWC3``)"""
    if torch.is_tensor(image):
        t = image
        if t.dtype != torch.uint8:
            raise ValueError(f"LineartDetector: uint8 image expected, got {t.dtype}")
        t = t.to(device)
        if t.dim() == 2:
            t = t[:, :, None]
        if t.dim() != 3 or t.shape[2] not in (1, 3, 4):
            raise ValueError(f"LineartDetector: HWC image with 1, 3 or 4 channels expected, got {tuple(t.shape)}")
        if t.shape[2] == 1:
            t = t.expand(-1, -1, 3)
        elif t.shape[2] == 4:
            color, alpha = t[:, :, :3].float(), t[:, :, 3:4].float() / 255.0
            t = (color * alpha + 255.0 * (1.0 - alpha)).clamp(0, 255).to(torch.uint8)
        return t.contiguous()
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise ValueError(f"LineartDetector: uint8 image expected, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError(f"LineartDetector: HWC image with 1, 3 or 4 channels expected, got {a.shape}")
    if a.shape[2] == 1:
        a = np.concatenate([a, a, a], axis=2)
    elif a.shape[2] == 4:
        color, alpha = a[:, :, :3].astype(np.float32), a[:, :, 3:4].astype(np.float32) / 255.0
        a = (color * alpha + 255.0 * (1.0 - alpha)).clip(0, 255).astype(np.uint8)
    return torch.from_numpy(np.array(a, order="C")).to(device)                  # a copy: np.asarray of a PIL image is read-only


class LineartDetector:
    """``controlnet_aux.LineartDetector.__call__`` with the generator on the device.  ``output_type="pil"`` returns what the reference returns (a PIL RGB
    image: ``processor(np.array(input_img))`` drops in unchanged); ``"pt"`` returns the control image as a device tensor [1, 3, H, W] = map / 255 in the
    model dtype, which ``pipelines._control_image`` passes through, so stage 2 has no host round trip for it; ``"np"`` the HWC uint8 array."""

    def __init__(self, model, model_coarse=None, output_type="pil"):
        if output_type not in ("pil", "pt", "np"):
            raise ValueError(f"LineartDetector: output_type must be 'pil', 'pt' or 'np', got {output_type!r}")
        self.model, self.model_coarse, self.output_type = model, model_coarse, output_type

    @classmethod
    def from_state_dict(cls, state_dict, coarse_state_dict=None, dtype=torch.bfloat16, device="cuda", output_type="pil"):
        def make(sd):
            g = LineartGenerator()
            g.load_state_dict(sd)
            return g.to(device=device, dtype=dtype).eval()
        return cls(make(state_dict), make(coarse_state_dict) if coarse_state_dict is not None else None, output_type=output_type)

    @classmethod
    def from_torch(cls, module_or_detector, dtype=torch.bfloat16, device="cuda", output_type="pil"):
        """From a ``controlnet_aux.LineartDetector`` (``.model`` / ``.model_coarse``) or from one generator module with the contract's parameter names"""
        if isinstance(module_or_detector, nn.Module):
            return cls.from_state_dict(module_or_detector.state_dict(), dtype=dtype, device=device, output_type=output_type)
        coarse = getattr(module_or_detector, "model_coarse", None)
        return cls.from_state_dict(module_or_detector.model.state_dict(), coarse.state_dict() if coarse is not None else None, dtype=dtype,
                                   device=device, output_type=output_type)

    def to(self, *args, **kw):
        self.model.to(*args, **kw)
        if self.model_coarse is not None:
            self.model_coarse.to(*args, **kw)
        return self

    def _maps(self, images, coarse, detect_resolution, image_resolution, want_pt=False):
        """list of images of one size -> (device uint8 [B, H, W, 3] or None, device [B, 3, H, W] in the model dtype or None): the control images.  The
        float form comes back only from the INTER_LINEAR launch with ``want_pt`` (then the bytes are not written at all); every other route returns the
        bytes and ``_output`` converts them."""
        model = self.model_coarse if coarse else self.model
        if model is None:
            raise ValueError("LineartDetector: coarse=True needs a coarse model (model_coarse is None)")
        u8 = [_to_u8_hwc3(im, model.device) for im in images]
        H, W = u8[0].shape[:2]
        if any(tuple(t.shape) != (H, W, 3) for t in u8):
            raise ValueError("LineartDetector.detect_many: all images must have one size")
        plan = plan_resizes(H, W, detect_resolution, image_resolution)              # raises before any device work
        batch = torch.stack(u8) if len(u8) > 1 else u8[0][None]
        if plan.area:
            x = ops.cv_area_u8(batch, plan.net, model.dtype)
        else:
            x = ops.image_from_u8(batch, model.dtype, range_mode=0)
        maps = model(x)                                                             # 255 - t, three times
        if not plan.linear:
            return maps, None
        if want_pt:
            return None, ops.cv_linear_u8(maps, plan.out, invert=True, dtype=model.dtype, u8_out=False)
        return ops.cv_linear_u8(maps, plan.out, invert=True), None

    def _output(self, u8, pt, i, output_type):
        """image i of u8 (device uint8 [B, H, W, 3]) or of pt (device [B, 3, H, W])"""
        if output_type == "pt":
            return pt[i:i + 1] if pt is not None else ops.image_from_u8(u8[i][None], self.model.dtype, range_mode=0)
        arr = u8[i].cpu().numpy()
        if output_type == "np":
            return arr
        from PIL import Image
        return Image.fromarray(arr)

    def _output_type(self, output_type):
        output_type = output_type or self.output_type
        if output_type not in ("pil", "pt", "np"):
            raise ValueError(f"LineartDetector: output_type must be 'pil', 'pt' or 'np', got {output_type!r}")
        return output_type

    @torch.no_grad()
    def __call__(self, input_image, coarse=False, detect_resolution=512, image_resolution=512, output_type=None):
        return self.detect_many([input_image], coarse, detect_resolution, image_resolution, output_type)[0]

    @torch.no_grad()
    def detect_many(self, images, coarse=False, detect_resolution=512, image_resolution=512, output_type=None):
        """A list of images of one size in ONE batched forward (InstanceNorm is per image, the resizes too: the same bytes as the single calls) -> list
        of outputs"""
        images = list(images)
        if not images:
            return []
        output_type = self._output_type(output_type)
        u8, pt = self._maps(images, coarse, detect_resolution, image_resolution, want_pt=output_type == "pt")
        return [self._output(u8, pt, i, output_type) for i in range(len(images))]
