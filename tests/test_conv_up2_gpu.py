"""GPU: ``ops.conv_up2`` (tg_conv_up2: Upsample2D with the nearest x2 folded into four 2x2-tap convs) against the unfolded kernel bit for bit on
exact-arithmetic operands, against the fp64 unfolded conv of the STORED weights on random ones, its writes, its determinism, and the routing /
weight cache of ``Upsample2D.run``.

Rounding: the folded weights are sums of up to four stored taps rounded once more to the storage dtype, so the folded layer carries one extra weight
rounding; simulated in exact arithmetic on the CPU the rel-L2 against fp64 is 2.35e-3 (bf16) / 2.94e-4 (fp16) after the output rounding (unfolded:
1.65e-3 / 2.08e-4), inside ``l2_tol`` = 3e-3 / 4e-4 of tests/launch_check.py, which is the bound asserted here."""
import pytest
import torch
import torch.nn.functional as F

from tests import launch_check as lc
from tests import parity_metrics as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
# (B, h, w, C, N): stacked 8 x 8 windows + ragged N (slow weight path); 16 / 32 wide; output width 128; several row tiles at width 8
CASES = [(2, 8, 8, 64, 192), (4, 16, 16, 128, 64), (1, 32, 32, 64, 320), (1, 64, 64, 64, 128), (16, 8, 8, 128, 128)]
_REF = {}


def rnd(shape, dtype, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _tokens(x):            # [B, C, h, w] -> token-major [B*h*w, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _ref64(x, wt, b):
    """fp64 unfolded layer of the stored operands -> token-major [B*2h*2w, N]"""
    y = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), wt.double(), b.double(), padding=1)
    return _tokens(y)


def _random_case(case, dtype):
    """operands (CPU, storage dtype) and the fp64 reference of one case, computed once and shared"""
    key = (case, dtype)
    if key not in _REF:
        B, h, w, Cc, N = case
        g = torch.Generator().manual_seed(1000 + CASES.index(case))
        x = rnd((B, Cc, h, w), dtype, g)
        wt = rnd((N, Cc, 3, 3), dtype, g, (9 * Cc) ** -0.5)
        b = rnd((N,), dtype, g)
        _REF[key] = (x, wt, b, _ref64(x, wt, b))
    return _REF[key]


def _ops():
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_conv3x3, pack_conv3x3_up2
    return ops, pack_conv3x3, pack_conv3x3_up2


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_operands_match_the_unfolded_kernel_bit_for_bit(case, dtype):
    ops, pack9, pack_up2 = _ops()
    B, h, w, Cc, N = case
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-2, 3, (B, Cc, h, w), generator=g).to(dtype)
    wt = torch.randint(-2, 3, (N, Cc, 3, 3), generator=g).to(dtype)
    b = torch.randint(-2, 3, (N,), generator=g).to(dtype)
    xt, bd = _tokens(x).to(DEV), b.to(DEV)
    got = ops.conv_up2(xt, pack_up2(wt).to(DEV), B, h, w, Cc, bias=bd)
    old = ops.conv3x3(xt, pack9(wt).to(DEV), B, h, w, Cc, upsample=True, bias=bd)
    torch.cuda.synchronize()
    assert got.shape == old.shape == (4 * B * h * w, N)
    diff = (got.view(torch.int16) != old.view(torch.int16))
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} elements differ, first at {diff.nonzero()[0].tolist()}"
    # and both are the exact result: every sum fits fp32, one rounding to the storage dtype
    assert torch.equal(got.cpu(), _ref64(x, wt, b).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_random_operands_against_fp64_unfolded_conv(case, dtype):
    ops, _, pack_up2 = _ops()
    B, h, w, Cc, N = case
    x, wt, b, ref = _random_case(case, dtype)
    got = ops.conv_up2(_tokens(x).to(DEV), pack_up2(wt).to(DEV), B, h, w, Cc, bias=b.to(DEV))
    torch.cuda.synchronize()
    m = pm.metrics(got.float().cpu(), ref)
    print(f"conv_up2 {case} {dtype}: rel_l2 {m['rel_l2']:.3e} max_rel {m['max_rel']:.3e}")
    pm.check(got.float().cpu(), ref, f"kernel: conv_up2 {case}", lc.l2_tol(dtype), lc.rel_tol(dtype), dtype=str(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_writes_every_element_nothing_else_and_is_deterministic(case, dtype):
    ops, _, pack_up2 = _ops()
    B, h, w, Cc, N = case
    x, wt, b, _ = _random_case(case, dtype)
    xt, wf, bd = _tokens(x).to(DEV), pack_up2(wt).to(DEV), b.to(DEV)
    M, G = 4 * B * h * w, 64
    runs = []
    for _ in range(2):
        buf = torch.full((M + 2 * G, N), float("nan"), dtype=dtype, device=DEV)
        guard = buf.view(torch.int16).clone()
        out = ops.conv_up2(xt, wf, B, h, w, Cc, bias=bd, out=buf[G:G + M])
        torch.cuda.synchronize()
        assert out.data_ptr() == buf[G:].data_ptr()
        assert not bool(torch.isnan(buf[G:G + M]).any()), "an output element was not written"
        now = buf.view(torch.int16)
        assert torch.equal(now[:G], guard[:G]) and torch.equal(now[G + M:], guard[G + M:]), "a guard row changed"
        runs.append(buf[G:G + M].view(torch.int16).clone())
    assert torch.equal(runs[0], runs[1])


def _upsampler(Cc, dtype, seed):
    from theatergen_amd.unet import Upsample2D
    up = Upsample2D(Cc)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        up.conv.weight.copy_(torch.randn(up.conv.weight.shape, generator=g) * (9 * Cc) ** -0.5)
        up.conv.bias.copy_(torch.randn(Cc, generator=g))
    return up.to(DEV, dtype)


def _run_module(up, x):
    from theatergen_amd.unet import _Act
    B, Cc, h, w = x.shape
    y = up.run(_Act(_tokens(x).to(DEV), B, h, w, Cc))
    torch.cuda.synchronize()
    assert (y.b, y.h, y.w, y.c) == (B, 2 * h, 2 * w, Cc)
    return y.t


def _count_up2(monkeypatch):
    from theatergen_amd import ops
    calls, orig = [], ops.conv_up2

    def counted(*a, **k):
        calls.append(a[2:6])
        return orig(*a, **k)
    monkeypatch.setattr(ops, "conv_up2", counted)
    return calls


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1, 8, 8, 64), (2, 12, 12, 64)], ids=["1x8x8", "2x12x12"])
def test_ineligible_geometry_takes_the_unfolded_path(shape, dtype, monkeypatch):
    B, h, w, Cc = shape
    calls = _count_up2(monkeypatch)
    up = _upsampler(Cc, dtype, 3)
    x = rnd((B, Cc, h, w), dtype, torch.Generator().manual_seed(4))
    got = _run_module(up, x)
    assert calls == []
    ref = _ref64(x, up.conv.weight.detach().cpu(), up.conv.bias.detach().cpu())
    pm.check(got.float().cpu(), ref, f"Upsample2D unfolded {shape}", lc.l2_tol(dtype), lc.rel_tol(dtype), dtype=str(dtype))


def test_switch_off_takes_the_unfolded_path(monkeypatch):
    from theatergen_amd import unet
    dtype, (B, h, w, Cc) = torch.bfloat16, (2, 8, 8, 64)
    calls = _count_up2(monkeypatch)
    up = _upsampler(Cc, dtype, 5)
    x = rnd((B, Cc, h, w), dtype, torch.Generator().manual_seed(6))
    ref = _ref64(x, up.conv.weight.detach().cpu(), up.conv.bias.detach().cpu())
    monkeypatch.setattr(unet, "_UP_FOLD", True)
    on = _run_module(up, x)
    assert calls == [(B, h, w, Cc)]
    monkeypatch.setattr(unet, "_UP_FOLD", False)           # what TG_UP_FOLD=0 sets at import (tests/test_conv_up2_cpu.py checks the reading)
    off = _run_module(up, x)
    assert calls == [(B, h, w, Cc)]
    for got in (on, off):
        pm.check(got.float().cpu(), ref, "Upsample2D switch", lc.l2_tol(dtype), lc.rel_tol(dtype), dtype=str(dtype))


def test_in_place_weight_update_refolds(monkeypatch):
    from theatergen_amd import unet
    monkeypatch.setattr(unet, "_UP_FOLD", True)
    dtype, (B, h, w, Cc) = torch.bfloat16, (2, 8, 8, 64)
    calls = _count_up2(monkeypatch)
    up = _upsampler(Cc, dtype, 7)
    x = rnd((B, Cc, h, w), dtype, torch.Generator().manual_seed(8))
    first = _run_module(up, x).clone()
    with torch.no_grad():
        up.conv.weight.mul_(-0.5).add_(0.01)
    ref = _ref64(x, up.conv.weight.detach().cpu(), up.conv.bias.detach().cpu())
    second = _run_module(up, x)
    assert len(calls) == 2 and not torch.equal(first, second)
    pm.check(second.float().cpu(), ref, "Upsample2D after an in-place weight update", lc.l2_tol(dtype), lc.rel_tol(dtype), dtype=str(dtype))
