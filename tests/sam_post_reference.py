"""fp64 restatement of SAM's mask post-processing, and the OR rule of the reference's last resize (shared by test_sam_decoder_cpu / _gpu).

``post_values``  transformers' ``post_process_masks`` up to the comparison: bilinear to the padded size, crop to the reshaped size, bilinear to the original
                 size, all ``align_corners=False``, in float64.  The mask is ``post_values(...) > threshold``.
``resize_bool``  the reference's ``F.interpolate(mask.float(), target, mode='bilinear').type(bool)`` (models/sam.py:50), as it is.
``or_taps``      the same as an OR over the taps of non-zero weight, from ATen's fp32 index arithmetic restated in numpy: src = max(fma(scale, dst + 0.5, -0.5), 0)
                 (ONE rounding: ATen's CPU kernels contract the expression; restated through float64, where the product and the difference are exact),
                 i0 = floor(src), i1 = min(i0 + 1, in - 1), weights (1 - l, l) with l = src - i0.  1 - l is never 0 (l < 1), so
                 tap i0 always counts and tap i1 counts when l > 0.  A product of two non-zero weights cannot underflow (each is >= 2^-24), and a sum of
                 non-negative terms is non-zero when one term is: the float result is non-zero exactly when a counted tap is set.
"""
import numpy as np
import torch
import torch.nn.functional as F


def post_values(logits, padded_size, reshaped_size, original_size):
    """logits [..., L, L] (any float dtype) -> float64 [..., h0, w0]"""
    x = torch.as_tensor(logits).double()
    lead = x.shape[:-2]
    x = x.reshape((1, -1) + tuple(x.shape[-2:]))
    x = F.interpolate(x, (int(padded_size), int(padded_size)), mode="bilinear", align_corners=False)
    x = x[..., :int(reshaped_size[0]), :int(reshaped_size[1])]
    x = F.interpolate(x, (int(original_size[0]), int(original_size[1])), mode="bilinear", align_corners=False)
    return x.reshape(tuple(lead) + tuple(x.shape[-2:]))


def resize_bool(mask, target):
    """mask bool / uint8 [..., h, w] -> bool [..., ht, wt], the reference's float route"""
    m = torch.as_tensor(mask)
    lead = m.shape[:-2]
    m = m.reshape((1, -1) + tuple(m.shape[-2:])).type(torch.float)
    out = F.interpolate(m, (int(target[0]), int(target[1])), mode="bilinear").type(torch.bool)
    return out.reshape(tuple(lead) + tuple(out.shape[-2:]))


def axis_taps(in_size, out_size):
    """(i0, i1, use1) int / int / bool arrays [out_size]: the two source indices of every destination index and whether the second has non-zero weight"""
    scale = np.float32(in_size) / np.float32(out_size)
    dst = np.arange(out_size, dtype=np.float64)
    src = (np.float64(scale) * (dst + 0.5) - 0.5).astype(np.float32)          # a 24-bit by 17-bit product and its difference are exact in float64
    src = np.maximum(src, np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    lam = src - i0.astype(np.float32)
    return i0, i1, (lam > 0) & (i1 != i0)


def or_taps(mask, target):
    """mask bool / uint8 [..., h, w] -> bool [..., ht, wt] by the OR rule"""
    m = np.asarray(torch.as_tensor(mask).cpu()).astype(bool)
    y0, y1, uy = axis_taps(m.shape[-2], int(target[0]))
    x0, x1, ux = axis_taps(m.shape[-1], int(target[1]))
    rows0, rows1 = m[..., y0, :], m[..., y1, :] & uy[:, None]
    out = rows0[..., x0] | (rows0[..., x1] & ux) | rows1[..., x0] | (rows1[..., x1] & ux)
    return torch.from_numpy(out)
