"""No GPU: the Upsample2D weight fold (``weights_pack.pack_conv3x3_up2``) against the unfolded layer in fp64, and the host-side contract of
``tg_conv_up2`` / ``tg_conv_up2_eligible`` (include/theatergen_hip.h): every refusal happens before any launch, so it needs no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from theatergen_amd import _lib
from theatergen_amd.weights_pack import pack_conv3x3_up2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def folded_conv(x, wf, bias=None):
    """the class / tap formula of the header, literally: out[b, n, 2i+py, 2j+px] = bias[n] + sum_{ty, tx, c} Wf[2py+px][n][ty, tx, c] * X[b, c, i+py+ty-1, j+px+tx-1],
    X zero outside the image.  x [B, C, h, w], wf [4, N, 4C] -> [B, N, 2h, 2w] in x's dtype."""
    B, Cc, h, w = x.shape
    N = wf.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))                                        # xp[..., r, s] = X[..., r - 1, s - 1]
    out = torch.zeros(B, N, 2 * h, 2 * w, dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            wc = wf[2 * py + px].reshape(N, 2, 2, Cc)
            acc = torch.zeros(B, N, h, w, dtype=x.dtype)
            for ty in range(2):
                for tx in range(2):
                    win = xp[:, :, py + ty:py + ty + h, px + tx:px + tx + w]       # X[i + py + ty - 1, j + px + tx - 1]
                    acc += torch.einsum("bchw,nc->bnhw", win, wc[:, ty, tx])
            out[:, :, py::2, px::2] = acc
    if bias is not None:
        out += bias[None, :, None, None]
    return out


@pytest.mark.parametrize("B,h,w,Cc,N", [(2, 8, 8, 16, 12), (1, 5, 7, 8, 4), (1, 16, 16, 4, 8)])
def test_fold_equals_upsample_then_conv_fp64(B, h, w, Cc, N):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Cc, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(N, Cc, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, b, padding=1)
    got = folded_conv(x, pack_conv3x3_up2(wt), b)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
def test_fold_shape_dtype_and_single_rounding(dtype):
    g = torch.Generator().manual_seed(8)
    wt = torch.randn(6, 5, 3, 3, generator=g).to(dtype)
    wf = pack_conv3x3_up2(wt)
    assert wf.shape == (4, 6, 20) and wf.dtype == dtype and wf.is_contiguous()
    # class (1, 0), tap (ty 0, tx 1) = rows {0, 1} x columns {1, 2}: summed in fp32 (fp64 for fp64), rounded once
    acc = wt.double() if dtype == torch.float64 else wt.float()
    want = (acc[:, :, 0, 1] + acc[:, :, 0, 2] + acc[:, :, 1, 1] + acc[:, :, 1, 2]).to(dtype)
    assert torch.equal(wf[2].reshape(6, 2, 2, 5)[:, 0, 1], want)
    # the corner taps are copies
    assert torch.equal(wf[0].reshape(6, 2, 2, 5)[:, 0, 0], wt[:, :, 0, 0]) and torch.equal(wf[3].reshape(6, 2, 2, 5)[:, 1, 1], wt[:, :, 2, 2])


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert re.search(r"^int\s+tg_conv_up2_eligible\s*\(\s*const tg_gemm_desc\*\s*d\s*\)\s*;", header, flags=re.M)
    assert re.search(r"^int\s+tg_conv_up2\s*\(\s*const tg_gemm_desc\*\s*d\s*,\s*void\*\s*stream\s*\)\s*;", header, flags=re.M)
    assert "#define TG_ABI_VERSION 308" in header
    assert _lib.SIGNATURES["tg_conv_up2_eligible"] == (_lib.i32, [C.POINTER(_lib.GemmDesc)])
    assert _lib.SIGNATURES["tg_conv_up2"] == (_lib.i32, [C.POINTER(_lib.GemmDesc), _lib.vp])
    L = _lib.lib()
    assert L.tg_version() == 308
    assert L.tg_conv_up2.argtypes == [C.POINTER(_lib.GemmDesc), _lib.vp] and L.tg_conv_up2_eligible.restype == _lib.i32


def _desc(batch=2, h=8, w=8, cin=64, n=64, dtype=0):
    d = _lib.GemmDesc()
    d.dtype, d.mode, d.stride, d.upsample = dtype, 1, 1, 1
    d.a0 = d.w = d.out = 16                                            # never dereferenced: every case below is decided on the host
    d.c0 = cin
    d.batch, d.in_h, d.in_w, d.out_h, d.out_w = batch, h, w, 2 * h, 2 * w
    d.M, d.N, d.K = 4 * batch * h * w, n, 16 * cin
    d.ldc, d.out_scale = n, 1.0
    return d


ELIGIBLE = [(2, 8, 8, 64, 192), (4, 16, 16, 128, 64), (1, 32, 32, 64, 320), (1, 64, 64, 64, 128), (16, 8, 8, 128, 128), (16, 32, 32, 640, 640)]
# batch 1 at 8 x 8 (half a block), the SD-2.1 widths, everything above low-resolution width 64, a block that straddles two images
INELIGIBLE = [(1, 8, 8, 64, 64), (2, 12, 12, 64, 64), (2, 24, 24, 64, 64), (2, 48, 48, 64, 64), (1, 96, 96, 64, 64), (1, 128, 128, 64, 64),
              (2, 6, 16, 64, 64), (1, 16, 8, 64, 64), (2, 8, 8, 32, 64)]


def test_eligibility():
    L = _lib.lib()
    for s in ELIGIBLE:
        assert L.tg_conv_up2_eligible(C.byref(_desc(*s))) == 1, s
    for s in INELIGIBLE:
        assert L.tg_conv_up2_eligible(C.byref(_desc(*s))) == 0, s


def test_refusals_need_no_device():
    L = _lib.lib()

    def rc(d):
        return L.tg_conv_up2(C.byref(d), None)

    d = _desc()
    d.a1, d.c1 = 16, 64                                               # two sources
    assert rc(d) < 0 and L.tg_conv_up2_eligible(C.byref(d)) == 0
    d = _desc()
    d.K = 9 * 64                                                      # the unfolded K
    assert rc(d) == -1 and b"16*c0" in L.tg_last_error()
    d = _desc()
    d.res, d.ldres = 16, 64                                           # a residual
    assert rc(d) == -3
    d = _desc()
    d.bvec, d.ldbvec, d.rows_per_batch = 16, 64, 256
    assert rc(d) == -3
    d = _desc()
    d.act = 1
    assert rc(d) == -3
    d = _desc()
    d.out_scale = 0.5
    assert rc(d) == -3
    for s in INELIGIBLE:                                              # geometry
        assert rc(_desc(*s)) == -3, s
    d = _desc()
    d.upsample = 0
    assert rc(d) == -1
    d = _desc()
    d.w = 8                                                           # misaligned weights
    assert rc(d) == -1
    d = _desc(batch=4096, h=64, w=64, cin=64, n=64)                    # 2^31-byte output
    assert rc(d) == -3


def test_env_switch_is_read_at_import():
    env = dict(os.environ, TG_UP_FOLD="0", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", "import theatergen_amd.unet as u; print(u._UP_FOLD)"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "False", out.stderr[-400:]
    from theatergen_amd import unet
    assert unet._UP_FOLD is (os.environ.get("TG_UP_FOLD", "1") != "0")
