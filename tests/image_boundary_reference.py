"""Host restatement of the uint8 <-> NCHW image boundary (``tg_image_from_u8`` / ``tg_image_to_u8``): the expressions of the pipelines, as numpy / torch
functions, and the search for inputs on which rounding half to even and half away from zero differ.  No GPU, no library."""
import numpy as np
import torch


def from_u8_host(images_u8, dtype, range_mode, copies):
    """uint8 ndarray [B, H, W, 3] -> tensor [copies * B, 3, H, W] in ``dtype``: ``a.astype(float32) / 255.0`` (numpy: an IEEE fp32 division), for the VAE
    input ``2.0 * x - 1.0`` (theatergen_amd/pipelines.py final_image_generation; reference models/pipelines.py:617-620), for the ControlNet control image
    as it is (``prepare_image``, :712-722); ``cat([x] * copies)``; one ``.to(dtype)``."""
    x = torch.from_numpy(np.asarray(images_u8).astype(np.float32) / 255.0).permute(0, 3, 1, 2)
    if range_mode == 1:
        x = 2.0 * x - 1.0
    return torch.cat([x] * copies).to(dtype).contiguous()


def to_u8_host(image):
    """tensor [B, 3, H, W] (any float dtype, CPU) -> uint8 ndarray [B, H, W, 3]: the expression of ``pipelines.decode``, ``_to_pil`` and the tail of
    ``final_image_generation`` (reference models/pipelines.py:163-173, 852-854).  NaN has no defined value here (``astype`` of NaN)."""
    arr = (image.float() / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    with np.errstate(invalid="ignore"):
        return (arr * 255).round().astype("uint8")


def to_u8_chain(x):
    """the fp32 value handed to ``round`` for fp32 inputs ``x`` (ndarray): every step rounded to fp32 as in ``to_u8_host``"""
    x = np.asarray(x, np.float32)
    y = np.clip(x / np.float32(2) + np.float32(0.5), np.float32(0), np.float32(1)).astype(np.float32)
    return (y * np.float32(255)).astype(np.float32)


def ties():
    """[(k, x)]: fp32 inputs x whose chain lands exactly on k + 0.5.  For k in 0..254: x = 2 * (fl((k + .5) / 255) - .5) in fp32, kept when the fp32
    chain gives exactly k + .5.  Half-to-even sends it to k for even k and to k + 1 for odd k; half-away-from-zero always to k + 1."""
    out = []
    for k in range(255):
        x = np.float32(2) * (np.float32(np.float32(k + 0.5) / np.float32(255)) - np.float32(0.5))
        if float(to_u8_chain(np.array([x], np.float32))[0]) == k + 0.5:
            out.append((k, np.float32(x)))
    return out


def division_vs_reciprocal():
    """the byte values u for which fp32 ``u / 255`` and ``u * (1 / 255)`` differ"""
    u = np.arange(256, dtype=np.float32)
    return np.nonzero((u / np.float32(255)) != (u * (np.float32(1) / np.float32(255))))[0]


def all_bytes_images(batch, h, w, seed):
    """uint8 [batch, h, w, 3] in which, where there is room (h * w >= 256), every byte value occurs in every channel of every image, in a different
    order per channel and per image: a channel mix-up or a wrong image / copy offset cannot cancel out.  Smaller images take a prefix of the order."""
    g = np.random.default_rng(seed)
    n = h * w
    out = np.empty((batch, n, 3), np.uint8)
    for b in range(batch):
        for c in range(3):
            vals = np.concatenate([g.permutation(256) for _ in range((n + 255) // 256)])[:n]
            out[b, :, c] = vals.astype(np.uint8)
    return out.reshape(batch, h, w, 3)
