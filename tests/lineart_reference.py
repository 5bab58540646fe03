"""The lineart annotator restated in plain ``torch.nn`` (the oracle of tests/test_lineart_*.py; no dependency on controlnet_aux or cv2).

Written from controlnet_aux's ``lineart/__init__.py``: ``Generator(input_nc=3, output_nc=1, n_residual_blocks=3, sigmoid=True)`` with
``nn.InstanceNorm2d`` defaults (no affine, eps 1e-5, biased variance) and a bias on every conv, and ``LineartDetector.__call__`` for the case both of its
resizes are the identity.  The tests run it in float64 on the CPU (the oracle), in the storage dtype on the CPU (the rounded emulation that sets the
bound) and in the storage dtype on the device (the oracle of the one 512 x 512 case)."""
import copy
import functools

import numpy as np
import torch
import torch.nn as nn


class ResidualBlock(nn.Module):
    def __init__(self, in_features):
        super().__init__()
        self.conv_block = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(in_features, in_features, 3), nn.InstanceNorm2d(in_features),
                                        nn.ReLU(inplace=True), nn.ReflectionPad2d(1), nn.Conv2d(in_features, in_features, 3),
                                        nn.InstanceNorm2d(in_features))

    def forward(self, x):
        return x + self.conv_block(x)


class Generator(nn.Module):
    def __init__(self, input_nc=3, output_nc=1, n_residual_blocks=3, sigmoid=True):
        super().__init__()
        self.model0 = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(input_nc, 64, 7), nn.InstanceNorm2d(64), nn.ReLU(inplace=True))
        model1, in_features, out_features = [], 64, 128
        for _ in range(2):
            model1 += [nn.Conv2d(in_features, out_features, 3, stride=2, padding=1), nn.InstanceNorm2d(out_features), nn.ReLU(inplace=True)]
            in_features, out_features = out_features, out_features * 2
        self.model1 = nn.Sequential(*model1)
        self.model2 = nn.Sequential(*[ResidualBlock(in_features) for _ in range(n_residual_blocks)])
        model3, out_features = [], in_features // 2
        for _ in range(2):
            model3 += [nn.ConvTranspose2d(in_features, out_features, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(out_features),
                       nn.ReLU(inplace=True)]
            in_features, out_features = out_features, out_features // 2
        self.model3 = nn.Sequential(*model3)
        model4 = [nn.ReflectionPad2d(3), nn.Conv2d(64, output_nc, 7)]
        if sigmoid:
            model4 += [nn.Sigmoid()]
        self.model4 = nn.Sequential(*model4)

    def forward(self, x):
        return self.model4(self.model3(self.model2(self.model1(self.model0(x)))))

    def pre_sigmoid(self, x):
        return self.model4[1](self.model4[0](self.model3(self.model2(self.model1(self.model0(x))))))


def sample_image(seed, h, w):
    """A seeded uint8 RGB image [h, w, 3] with structure at several scales (smooth ramps, blocks, noise): not near-constant anywhere"""
    g = torch.Generator().manual_seed(1000 + seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    img = torch.stack([0.5 + 0.5 * torch.sin(6.0 * xx + 2.0 * seed + c) * torch.cos(4.0 * yy - c) for c in range(3)], dim=-1)
    blocks = torch.rand(((h + 7) // 8, (w + 7) // 8, 3), generator=g)
    blocks = blocks.repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w]
    img = 0.5 * img + 0.35 * blocks + 0.15 * torch.rand((h, w, 3), generator=g)
    return (img.clamp(0, 1) * 255).round().to(torch.uint8).numpy()


@functools.lru_cache(maxsize=None)
def seeded_generator(seed=0):
    """Default inits under a fixed seed, float64; the last conv scaled (and its bias shifted) so that the pre-sigmoid map of ``sample_image(0, 32, 48)`` has
    mean 0 and standard deviation 1.5: the sigmoid map then spans most of [0, 1] instead of sitting at 0.5"""
    torch.manual_seed(seed)
    g = Generator().double().eval()
    with torch.no_grad():
        z = g.pre_sigmoid(preprocess(sample_image(0, 32, 48)).double())
        last = g.model4[1]
        scale = 1.5 / float(z.std())
        last.weight.mul_(scale)
        last.bias.copy_((last.bias - z.mean()) * scale)
    return g


def rounded_copy(gen, dtype, compute_dtype=torch.float64):
    """The generator with every parameter rounded to the storage dtype, held in ``compute_dtype``"""
    g = copy.deepcopy(gen)
    with torch.no_grad():
        for p in g.parameters():
            p.copy_(p.to(dtype).to(p.dtype))
    return g.to(compute_dtype).eval()


def preprocess(image_u8):
    """HWC uint8 RGB (ndarray) -> float32 NCHW [1, 3, H, W] in [0, 1] (steps 1 - 3 of the call with identity resizes)"""
    a = np.asarray(image_u8)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3
    return torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1)[None]


def byte_map(line):
    """sigmoid map [H, W] (any float dtype) -> uint8 [H, W, 3] control image: 255 - (line * 255).clip(0, 255).astype(uint8), replicated (steps 5 - 8)"""
    m = (line.detach().double().cpu().numpy() * 255.0).clip(0, 255).astype(np.uint8)
    return 255 - np.stack([m, m, m], axis=2)


def resized_size(h, w, resolution):
    k = float(resolution) / min(h, w)
    return int(np.round(h * k / 64.0)) * 64, int(np.round(w * k / 64.0)) * 64


@torch.no_grad()
def run(gen, x):
    """x [B, 3, H, W] already in the storage-rounded values -> sigmoid maps [B, H, W] in gen's dtype"""
    p = next(gen.parameters())
    return gen(x.to(device=p.device, dtype=p.dtype))[:, 0]


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm())


def level_diff(a_u8, ref_u8):
    d = np.abs(np.asarray(a_u8).astype(np.int32) - np.asarray(ref_u8).astype(np.int32))
    return float(d.mean()), int(d.max())


def distinct_levels(u8):
    return int(np.unique(np.asarray(u8)).size)
