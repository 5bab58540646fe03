"""GPU: ``tg_layernorm_add`` (LN(x + res), the sum in fp32) against fp64 from the stored operands.

Bound: the kernel's only rounding is the output's.  The storage formats have p = 8 (bf16) / 11 (fp16) significant bits, so rounding to nearest moves an
element by at most the unit roundoff u = 2^-p of its magnitude (half an ulp is 2^-p of the BOTTOM of the element's binade, hence up to u relative to the
element): max|err| / max|ref| <= u.  Over a tensor the rounding errors are spread over +-half an ulp, rms ulp / sqrt(12) = u / sqrt(3) of the binade's
bottom: rel-L2 <= u / sqrt(3).  Both get 1e-5 for the fp32 statistics (two passes over <= 1280 values: ~sqrt(C) 2^-24 relative).  The route this
replaces, a residual GEMM epilogue followed by ``layernorm``, rounds the sum first: its error on the same operands must be the larger one.
Measured: max 2.2e-3 .. 3.3e-3 (bf16, u = 3.9e-3) and 2.7e-4 .. 4.0e-4 (fp16, u = 4.9e-4)."""
import pytest
import torch

from tests import parity_metrics as pm

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CASES = [(5, 128, 0), (37, 256, 8), (130, 320, 0), (9, 640, 16), (3, 1024, 0)]           # rows, C, extra row pitch of x and res


def bound(dtype):
    """(rel-L2, max) bounds: see the module docstring"""
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    return u / 3 ** 0.5 + 1e-5, u + 1e-5


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("rows,C,pad", CASES)
def test_layernorm_add_against_fp64(rows, C, pad, dname):
    from theatergen_amd import ops
    dt = DTYPES[dname]
    g = torch.Generator().manual_seed(rows * 1000 + C)
    xb = torch.full((rows, C + pad), float("nan"), dtype=dt)
    rb = torch.full((rows, C + pad), float("nan"), dtype=dt)
    xb[:, :C] = (1.5 * torch.randn(rows, C, generator=g)).to(dt)
    rb[:, :C] = (0.7 * torch.randn(rows, C, generator=g) + 0.3).to(dt)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(dt), (0.2 * torch.randn(C, generator=g)).to(dt)
    s = xb[:, :C].double() + rb[:, :C].double()
    want = torch.nn.functional.layer_norm(s, (C,), gamma.double(), beta.double(), 1e-5)
    xd, rd = xb.cuda(), rb.cuda()
    buf = torch.full((rows * C + 1024,), float("nan"), dtype=dt, device="cuda")
    out = buf[:rows * C].view(rows, C)
    ops.layernorm_add(xd[:, :C], rd[:, :C], gamma.cuda(), beta.cuda(), 1e-5, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isnan(buf[rows * C:]).all())
    m = pm.check(out.float().cpu(), want, f"layernorm_add {rows}x{C} {dname}", *bound(dt))
    # the rounded-sum route on the same operands
    old = ops.layernorm((xd[:, :C].float() + rd[:, :C].float()).to(dt).contiguous(), gamma.cuda(), beta.cuda(), 1e-5)
    m_old = pm.metrics(old.float().cpu(), want)
    print(f"layernorm_add {rows}x{C} {dname}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (bounds {bound(dt)[0]:.3e} / {bound(dt)[1]:.3e}); rounded sum first: {m_old['rel_l2']:.3e}")
    assert m["rel_l2"] < m_old["rel_l2"]
    again = ops.layernorm_add(xd[:, :C], rd[:, :C], gamma.cuda(), beta.cuda(), 1e-5)
    assert torch.equal(again.view(torch.int16), out.view(torch.int16))


def test_layernorm_add_refusals_leave_out_untouched():
    from theatergen_amd import ops
    dt = torch.bfloat16
    x = torch.zeros((4, 128), dtype=dt, device="cuda")
    gb = torch.ones(128, dtype=dt, device="cuda")
    out = torch.full((4, 128), 7.0, dtype=dt, device="cuda")
    for kw in (dict(res=torch.zeros((4, 128), dtype=torch.float16, device="cuda")), dict(res=torch.zeros((3, 128), dtype=dt, device="cuda")),
               dict(gamma=torch.ones(64, dtype=dt, device="cuda")), dict(out=torch.full((4, 64), 7.0, dtype=dt, device="cuda"))):
        a = dict(res=x, gamma=gb, out=out)
        a.update(kw)
        with pytest.raises(RuntimeError, match="layernorm_add"):
            ops.layernorm_add(x, a["res"], a["gamma"], gb, 1e-5, out=a["out"])
    big = torch.zeros((2, 1288), dtype=dt, device="cuda")
    with pytest.raises(RuntimeError, match="error -3"):
        ops.layernorm_add(big, big, torch.ones(1288, dtype=dt, device="cuda"), torch.ones(1288, dtype=dt, device="cuda"))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
