"""CPU (no GPU): the lineart annotator's host side: parameter names, the transposed-conv weight repacks evaluated against tg_conv_up2's / tg_gemm's
documented contracts in float64, the identity-resize predicate, and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lineart_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tg_lineart_instnorm_scratch_bytes", "tg_lineart_instnorm", "tg_lineart_conv7_in", "tg_lineart_conv7_out")


def test_state_dict_names_and_shapes_match_the_restatement():
    from theatergen_amd.lineart import LineartGenerator
    ours = {k: tuple(v.shape) for k, v in LineartGenerator().state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in LR.Generator().state_dict().items()}
    assert ours == ref
    expected = {"model0.1", "model1.0", "model1.3", "model3.0", "model3.3", "model4.1"} | {f"model2.{i}.conv_block.{j}" for i in range(3) for j in (1, 5)}
    assert {k.rsplit(".", 1)[0] for k in ours} == expected
    g = LineartGenerator()
    g.load_state_dict(LR.seeded_generator().state_dict())          # strict: a controlnet_aux-style state dict loads as it is


def _up2_contract(x, wf, bias):
    """tg_conv_up2 as include/theatergen_hip.h documents it, in x's dtype on the CPU: x [B, h, w, C], wf [4, N, 4 C] tap-major (ty, tx, c) ->
    [B, 2h, 2w, N]; input pixel (i + py + ty - 1, j + px + tx - 1), zero outside the image"""
    B, h, w, C_ = x.shape
    N = wf.shape[1]
    out = torch.zeros(B, 2 * h, 2 * w, N, dtype=x.dtype)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))                                # rows / columns -1 and h / w
    for py in range(2):
        for px in range(2):
            wc = wf[2 * py + px].reshape(N, 2, 2, C_)
            acc = bias[None, None, None, :].expand(B, h, w, N).clone()
            for ty in range(2):
                for tx in range(2):
                    win = xp[:, py + ty:py + ty + h, px + tx:px + tx + w]          # padded index = i + py + ty - 1 + 1
                    acc = acc + torch.einsum("bijc,nc->bijn", win, wc[:, ty, tx])
            out[:, py::2, px::2] = acc
    return out


def _conv3x3_parity_contract(x, wp, bias4):
    """tg_gemm mode 1 (stride 1, pad 1, weight [N', 9 C] tap-major (ky, kx, c)) on the low-resolution grid, then the parity-class layout of
    tg_lineart_instnorm (layout 2) read back as an image: x [B, h, w, C] -> [B, 2h, 2w, N' / 4]"""
    B, h, w, C_ = x.shape
    n4 = wp.shape[0]
    wt = wp.reshape(n4, 3, 3, C_).permute(0, 3, 1, 2)
    y = F.conv2d(x.permute(0, 3, 1, 2), wt, bias4, padding=1).permute(0, 2, 3, 1)             # [B, h, w, 4 N]
    n = n4 // 4
    out = torch.zeros(B, 2 * h, 2 * w, n, dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            out[:, py::2, px::2] = y[..., (2 * py + px) * n:(2 * py + px + 1) * n]
    return out


@pytest.mark.parametrize("h,w", [(3, 5), (4, 4)])
@pytest.mark.parametrize("cin,cout", [(8, 4), (4, 8)])
def test_transposed_conv_repacks_against_conv_transpose2d(h, w, cin, cout):
    from theatergen_amd.weights_pack import pack_convT3x3_s2_conv3x3, pack_convT3x3_s2_up2
    g = torch.Generator().manual_seed(7 * h + w + cin)
    x = torch.randn(2, cin, h, w, dtype=torch.float64, generator=g)
    wt = torch.randn(cin, cout, 3, 3, dtype=torch.float64, generator=g)
    bias = torch.randn(cout, dtype=torch.float64, generator=g)
    ref = F.conv_transpose2d(x, wt, bias, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    scale = float(ref.abs().max())
    wf = pack_convT3x3_s2_up2(wt)
    assert tuple(wf.shape) == (4, cout, 4 * cin) and wf.dtype == wt.dtype
    assert int((wf != 0).sum()) == 9 * cin * cout                    # a permutation with zeros: every original tap exactly once
    got = _up2_contract(x.permute(0, 2, 3, 1).contiguous(), wf, bias)
    assert float((got - ref).abs().max()) <= 1e-12 * scale
    wp = pack_convT3x3_s2_conv3x3(wt)
    assert tuple(wp.shape) == (4 * cout, 9 * cin)
    assert int((wp != 0).sum()) == 9 * cin * cout
    got = _conv3x3_parity_contract(x.permute(0, 2, 3, 1).contiguous(), wp, bias.repeat(4))
    assert float((got - ref).abs().max()) <= 1e-12 * scale


def test_conv7_packs_are_exact_permutations():
    from theatergen_amd.weights_pack import pack_conv7x7_fp32, pack_conv7x7_to1_fp32
    w = torch.randn(64, 3, 7, 7).to(torch.bfloat16)
    p = pack_conv7x7_fp32(w)
    assert p.dtype == torch.float32 and tuple(p.shape) == (147, 64)
    assert p[(2 * 7 + 3) * 7 + 5, 11] == w[11, 2, 3, 5].float()
    w1 = torch.randn(1, 64, 7, 7).to(torch.float16)
    p1 = pack_conv7x7_to1_fp32(w1)
    assert p1.dtype == torch.float32 and tuple(p1.shape) == (49, 64)
    assert p1[4 * 7 + 6, 33] == w1[0, 33, 4, 6].float()


def test_identity_resize_predicate():
    from theatergen_amd.lineart import check_identity_resize, resized_size
    check_identity_resize(512, 512, 512, 512)
    check_identity_resize(512, 768, 512, 512)
    for h, w, det, img in ((500, 500, 512, 512), (512, 512, 384, 1024), (512, 512, 256, 512)):
        with pytest.raises(NotImplementedError, match="cv2"):
            check_identity_resize(h, w, det, img)
    for h, w, res in ((512, 512, 512), (500, 500, 512), (512, 768, 512), (480, 640, 384), (1000, 333, 512), (96, 160, 512)):
        assert resized_size(h, w, res) == LR.resized_size(h, w, res)


def test_detector_argument_errors_without_a_device():
    from theatergen_amd.lineart import LineartDetector, LineartGenerator
    det = LineartDetector(LineartGenerator())
    with pytest.raises(ValueError, match="coarse"):
        det(np.zeros((512, 512, 3), np.uint8), coarse=True)
    with pytest.raises(NotImplementedError):
        det(np.zeros((500, 500, 3), np.uint8))
    with pytest.raises(ValueError, match="output_type"):
        LineartDetector(LineartGenerator(), output_type="jpeg")


def test_new_symbols_are_declared_and_bound():
    from theatergen_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(tg_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 308 and "#define TG_ABI_VERSION 308" in header
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    for name in NEW_SYMBOLS:
        assert getattr(h, name) is not None
    # host-side validation, before any launch
    assert h.tg_lineart_instnorm_scratch_bytes(1, 8, 8, 96) == -1
    assert h.tg_lineart_instnorm_scratch_bytes(2, 512, 512, 64) == 2 * 64 * (128 * 16 + 8)
    assert h.tg_lineart_instnorm(0, 16, 0, 1, 8, 8, 96, 1e-5, 0, None, 0, 32, 0, 48, None) == -1 and b"tg_lineart_instnorm" in h.tg_last_error()
    assert h.tg_lineart_conv7_in(0, 16, 1, 3, 3, 16, 16, 32, None) == -1 and b"h, w >= 4" in h.tg_last_error()
    assert h.tg_lineart_conv7_out(0, 16, 1, 3, 3, 16, 0.0, 32, None, None) == -1 and b"h, w >= 4" in h.tg_last_error()
