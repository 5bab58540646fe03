"""MI355X-native T2I-Adapter (diffusers 0.21.4 ``T2IAdapter(adapter_type="full_adapter_xl")``): the line-art adapter of the SDXL
stage-2 flow (reference ``models/pipelines.py:634-697``: ``controlnetpipe.adapter(adapter_input)``).

Module / parameter names equal the diffusers state-dict keys (``adapter.conv_in.weight``, ``adapter.body.{k}.in_conv.weight``,
``adapter.body.{k}.resnets.{j}.block{1,2}.weight``), so ``from_state_dict`` of a diffusers checkpoint loads as is.

    x = PixelUnshuffle(f)(image); x = conv_in(x)                           3 x 3, pad 1
    body[k] = AdapterBlock: [AvgPool2d(2, 2, ceil_mode)] -> [in_conv 1 x 1 if in != out] -> num_res_blocks x (x + block2(relu(block1(x))))
    returns the output of every body block (four features: /f, /f, /2f, /2f of the image)

Execution: activations are token-major [B*h*w, C] end to end.  ``tg_pixel_unshuffle`` writes the layout ``conv_in`` reads, the 3 x 3
convolutions run on the implicit-GEMM conv, the 1 x 1 convolutions are GEMMs with bias (and the resnet's residual in the epilogue),
ReLU and the pool are elementwise launches of their own (the hot GEMM / conv epilogues are not touched).  No PyTorch compute."""
import torch
import torch.nn as nn

from . import ops
from .unet import _Act, _load_on_meta, _Packed
from .weights_pack import pack_conv3x3


class AdapterResnetBlock(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.block1 = nn.Conv2d(channels, channels, 3, padding=1)
        self.act = nn.ReLU()
        self.block2 = nn.Conv2d(channels, channels, 1)
        self._p = _Packed()

    def run(self, x: _Act):
        w1 = self._p.get("b1", [self.block1.weight], lambda: pack_conv3x3(self.block1.weight.detach()))
        h = ops.conv3x3(x.t, w1, x.b, x.h, x.w, x.c, bias=self.block1.bias)
        h = ops.relu(h, out=h)
        w2 = self.block2.weight.reshape(x.c, x.c)
        return _Act(ops.linear(h, w2, self.block2.bias, res=x.t), x.b, x.h, x.w, x.c)


class AdapterBlock(nn.Module):
    def __init__(self, in_channels, out_channels, num_res_blocks, down=False):
        super().__init__()
        self.down = down
        self.downsample = nn.AvgPool2d(kernel_size=2, stride=2, ceil_mode=True) if down else None
        self.in_conv = nn.Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else None
        self.resnets = nn.Sequential(*[AdapterResnetBlock(out_channels) for _ in range(num_res_blocks)])

    def run(self, x: _Act):
        if self.down:
            x = _Act(ops.avgpool2x2(x.t, x.b, x.h, x.w), x.b, (x.h + 1) // 2, (x.w + 1) // 2, x.c)
        if self.in_conv is not None:
            cout = self.in_conv.weight.shape[0]
            x = _Act(ops.linear(x.t, self.in_conv.weight.reshape(cout, x.c), self.in_conv.bias), x.b, x.h, x.w, cout)
        for r in self.resnets:
            x = r.run(x)
        return x


class FullAdapterXL(nn.Module):
    def __init__(self, in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=16):
        super().__init__()
        if len(channels) != 4:
            raise ValueError("FullAdapterXL: four body blocks (channels of length 4)")
        self.in_channels, self.downscale_factor = in_channels, downscale_factor
        self.unshuffle = nn.PixelUnshuffle(downscale_factor)
        self.conv_in = nn.Conv2d(in_channels * downscale_factor ** 2, channels[0], 3, padding=1)
        body = []
        for i in range(len(channels)):
            if i == 1:
                body.append(AdapterBlock(channels[0], channels[1], num_res_blocks))
            elif i == 2:
                body.append(AdapterBlock(channels[1], channels[2], num_res_blocks, down=True))
            else:
                body.append(AdapterBlock(channels[i], channels[i], num_res_blocks))
        self.body = nn.ModuleList(body)
        self.total_downscale_factor = downscale_factor * 2
        self._p = _Packed()

    def run(self, x):
        """x NCHW [B, in_channels, H, W] in the storage dtype -> list of token-major ``_Act`` features"""
        B, cin, H, W = x.shape
        f = self.downscale_factor
        if cin != self.in_channels or H % f or W % f:
            raise ValueError(f"T2I-Adapter input must be [B, {self.in_channels}, H, W] with H, W multiples of {f}, got {tuple(x.shape)}")
        t = ops.pixel_unshuffle(x, f)
        w_in = self._p.get("conv_in", [self.conv_in.weight], lambda: pack_conv3x3(self.conv_in.weight.detach()))
        h, w = H // f, W // f
        y = _Act(ops.conv3x3(t, w_in, B, h, w, cin * f * f, bias=self.conv_in.bias), B, h, w, self.conv_in.weight.shape[0])
        feats = []
        for blk in self.body:
            y = blk.run(y)
            feats.append(y)
        return feats


class T2IAdapter(nn.Module):
    """``T2IAdapter(in_channels, channels, num_res_blocks, downscale_factor, adapter_type="full_adapter_xl")``: ``adapter(image)`` returns the
    four features as NCHW tensors (the diffusers surface); ``adapter(image, token_major=True)`` returns token-major ``_Act`` features the UNet
    and ``DenoiseEngine.set_adapter`` take without a transpose."""

    def __init__(self, in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=16, adapter_type="full_adapter_xl"):
        super().__init__()
        if adapter_type != "full_adapter_xl":
            raise NotImplementedError(f"T2IAdapter: adapter_type {adapter_type!r} is not supported (full_adapter_xl only)")
        self.config = dict(in_channels=in_channels, channels=tuple(channels), num_res_blocks=num_res_blocks, downscale_factor=downscale_factor,
                           adapter_type=adapter_type)
        self.adapter = FullAdapterXL(in_channels, channels, num_res_blocks, downscale_factor)
        for p_ in self.parameters():
            p_.requires_grad_(False)

    @property
    def dtype(self):
        return self.adapter.conv_in.weight.dtype

    @property
    def device(self):
        return self.adapter.conv_in.weight.device

    @property
    def total_downscale_factor(self):
        return self.adapter.total_downscale_factor

    def forward(self, x, token_major=False):
        if not x.is_cuda:
            raise RuntimeError("theatergen_amd T2IAdapter runs on the GPU only (no CPU fallback)")
        with torch.no_grad():
            feats = self.adapter.run(x.to(self.dtype))
            if token_major:
                return feats
            return [ops.transpose(f.t, f.b, f.hw, f.c).reshape(f.b, f.c, f.h, f.w) for f in feats]

    __call__ = forward

    @classmethod
    def from_state_dict(cls, state_dict, device="cuda", dtype=torch.bfloat16, **config):
        """``config``: the constructor arguments (in_channels, channels, num_res_blocks, downscale_factor); keys carry the ``adapter.`` prefix"""
        return _load_on_meta(lambda: cls(**config), state_dict, device, dtype)
