"""GPU: ``rc_ff2_kernel`` — ``tg_rc_ff`` at two waves per SIMD (csrc/tg_rowchain.hip; streams of ``rowchain.pack_ff2`` / ``pack_po2``) — against an
fp64 restatement of the chain, against the recorded outputs of the retired one-wave ``rc_ff_kernel`` bit for bit on exact-arithmetic operands
(tests/golden/rc_ff_one_wave_exact.npz), its writes, and the routing of ``FeedForward.run_fused``.

Tolerance: the rel-L2 against fp64 that the one-wave ``rc_ff_kernel`` reached ON THE SAME INPUTS (``PARENT`` below, measured on MI355X at the last
commit that had that kernel; profiles/r4_rowchain_findings.md gives 2.6e-3 bf16 / 3.3e-4 fp16 for its own operands) plus 10 % for the
other MFMA shape's summation order.  Both kernels round the normalised rows, the hidden activations and h3 to the storage dtype at the same places
and evaluate the same erf polynomial, so they differ in the order of the fp32 sums only.
"""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import launch_check as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 320
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# (M, inner, proj_out tail, row pitches (ldh, ldres, ldc)).  M: one workgroup, three, 17 (not a multiple of the 8 XCDs: rc_block_id's uneven split), and
# 1000 (a workgroup whose last waves are partly / wholly past M: clamped loads, predicated stores).  inner 64 / 128: fewer slices than the pipeline is deep.
CASES = {
    "m128_i64": (128, 64, False, (320, 320, 320)),
    "m128_i128_po_pitch": (128, 128, True, (352, 328, 384)),
    "m384_i1280_po": (384, 1280, True, (320, 320, 320)),
    "m384_i128_pitch": (384, 128, False, (352, 328, 384)),
    "m2176_i1280_pitch": (2176, 1280, False, (352, 328, 384)),
    "m2176_i64_po": (2176, 64, True, (320, 320, 320)),
    "m2176_i1280_po_pitch": (2176, 1280, True, (352, 328, 384)),
    "m1000_i128_po": (1000, 128, True, (320, 320, 320)),
}
# rel-L2 against fp64 of the ONE-wave rc_ff_kernel on exactly these operands (MI355X).  A recorded table: that kernel was retired
# (profiles/rc_ff_one_wave_retired_findings.md), so the first column can no longer be regenerated.
PARENT = {
    ("m128_i64", "bf16"): 2.4517e-03,      # two-wave kernel: 2.4517e-03
    ("m128_i64", "fp16"): 3.0976e-04,      # two-wave kernel: 3.0977e-04
    ("m128_i128_po_pitch", "bf16"): 2.5825e-03,      # two-wave kernel: 2.5817e-03
    ("m128_i128_po_pitch", "fp16"): 3.2575e-04,      # two-wave kernel: 3.2571e-04
    ("m384_i1280_po", "bf16"): 2.6339e-03,      # two-wave kernel: 2.6339e-03
    ("m384_i1280_po", "fp16"): 3.3045e-04,      # two-wave kernel: 3.3026e-04
    ("m384_i128_pitch", "bf16"): 2.4513e-03,      # two-wave kernel: 2.4513e-03
    ("m384_i128_pitch", "fp16"): 3.0856e-04,      # two-wave kernel: 3.0875e-04
    ("m2176_i1280_pitch", "bf16"): 2.4906e-03,      # two-wave kernel: 2.4907e-03
    ("m2176_i1280_pitch", "fp16"): 3.1169e-04,      # two-wave kernel: 3.1175e-04
    ("m2176_i64_po", "bf16"): 2.6719e-03,      # two-wave kernel: 2.6718e-03
    ("m2176_i64_po", "fp16"): 3.3420e-04,      # two-wave kernel: 3.3423e-04
    ("m2176_i1280_po_pitch", "bf16"): 2.6229e-03,      # two-wave kernel: 2.6230e-03
    ("m2176_i1280_po_pitch", "fp16"): 3.2853e-04,      # two-wave kernel: 3.2857e-04
    ("m1000_i128_po", "bf16"): 2.6341e-03,      # two-wave kernel: 2.6340e-03
    ("m1000_i128_po", "fp16"): 3.2901e-04,      # two-wave kernel: 3.2899e-04
}
_OPS = {}


def operands(case, dname):
    """CPU operands in the storage dtype and the fp64 chain over them, computed once per (case, dtype) and shared"""
    key = (case, dname)
    if key not in _OPS:
        M, inner, proj, _ = CASES[case]
        dt = DTYPES[dname]
        g = torch.Generator().manual_seed(100 + list(CASES).index(case))
        rn = lambda *s: torch.randn(*s, generator=g)
        o = {"h": (rn(M, C) * 1.2 + 0.2).to(dt), "x0": rn(M, C).to(dt),
             "w1": (rn(2 * inner, C) / C ** 0.5).to(dt), "b1": (0.2 * rn(2 * inner)).to(dt),
             "w2": (rn(C, inner) / inner ** 0.5).to(dt), "b2": (0.1 * rn(C)).to(dt),
             "wp": (rn(C, C) / C ** 0.5).to(dt), "bp": (0.1 * rn(C)).to(dt),
             "gamma": (1 + 0.2 * rn(C)).to(dt), "beta": (0.1 * rn(C)).to(dt)}
        d = {k: v.double() for k, v in o.items()}
        x = F.layer_norm(d["h"], (C,), d["gamma"], d["beta"], 1e-5)
        pr = x @ d["w1"].T + d["b1"]
        h3 = (pr[:, :inner] * F.gelu(pr[:, inner:])) @ d["w2"].T + d["b2"] + d["h"]
        o["ref"] = h3 @ d["wp"].T + d["bp"] + d["x0"] if proj else h3
        _OPS[key] = o
    return _OPS[key]


def _pitched(t, ld, fill=None):
    """the rows of ``t`` inside a device buffer of row pitch ``ld`` (the padding columns hold ``fill``)"""
    buf = torch.full((t.shape[0], ld), float("nan") if fill is None else fill, dtype=t.dtype, device=DEV)
    buf[:, :C] = t.to(DEV)
    return buf, buf[:, :C]


def launch(o, case, eps=1e-5):
    """one ``tg_rc_ff`` launch on the case's pitches; returns (output rows, the whole output buffer)"""
    from theatergen_amd import ops, rowchain
    M, inner, proj, (ldh, ldres, ldc) = CASES[case] if isinstance(case, str) else case
    dev = lambda k: o[k].to(DEV)
    s1, s2, bb2 = rowchain.pack_ff2(dev("w1"), dev("b1"), dev("gamma"), dev("beta"), dev("w2"), dev("b2"))
    wpo = res0 = None
    if proj:
        wpo = rowchain.pack_po2(dev("wp"), dev("bp").float())
        _, res0 = _pitched(o["x0"], ldres, 0.0)
    _, h = _pitched(o["h"], ldh, 0.0)
    obuf = torch.full((M, ldc), float("nan"), dtype=o["h"].dtype, device=DEV)
    out = ops.rc_ff(h, s1, s2, bb2, inner, eps, wpo=wpo, res0=res0, out=obuf[:, :C])
    torch.cuda.synchronize()
    assert out.data_ptr() == obuf.data_ptr()
    return obuf[:, :C], obuf


def rel_l2(got, ref):
    return ((got.double().cpu() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", list(CASES))
def test_against_the_fp64_chain(case, dname):
    """``PARENT`` was measured on the one-wave ``rc_ff_kernel`` at the last commit that had it (``meta`` of tests/golden/rc_ff_one_wave_exact.npz names
    it); that kernel is gone, so the table can no longer be regenerated and stays as recorded, with the 1.1 factor of the module docstring"""
    o = operands(case, dname)
    got, buf = launch(o, case)
    err = rel_l2(got, o["ref"])
    bound = 1.1 * PARENT[(case, dname)]
    print(f"rc_ff2 {case} {dname}: rel_l2 {err:.3e} (one-wave kernel {PARENT[(case, dname)]:.3e}, bound {bound:.3e})")
    assert torch.isfinite(got).all(), "an output element was not written"
    assert bool(torch.isnan(buf[:, C:]).all()), "a padding column of the output rows was written"
    assert err <= bound


def _exact_operands(M, inner, dt, seed):
    """Operands on which BOTH kernels are exact up to the shared roundings, whatever the order of their sums:
      * rows of +-1 with 160 of each and eps = 3: mean 0, variance 1, rstd = rsqrt(4) -> normalised rows +-0.5 after the rounding;
      * proj rows with four +-1 weights (sums in {-2 .. 2}) and integer biases: value in +-[3, 8], gate in [2, 7], so the hidden activations
        a * gelu(g) lie in +-[5.8, 56]: multiples of 2^-5 (bf16) / 2^-8 (fp16) below 2^6;
      * net.2 rows with 128 weights +-1: every partial sum is a multiple of that quantum below 2^13 — exact in fp32;
      * proj_out rows with ONE weight (+-1, +-2) and integer bias / residual: one product per output."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    sign = lambda *s: ri(0, 1, *s) * 2 - 1
    h = torch.stack([torch.cat([torch.ones(160), -torch.ones(160)])[torch.randperm(C, generator=g)] for _ in range(M)])
    w1 = torch.zeros(2 * inner, C)
    for r in range(2 * inner):
        w1[r, torch.randperm(C, generator=g)[:4]] = sign(4).float()
    b1 = torch.cat([sign(inner) * ri(5, 6, inner), ri(4, 5, inner)]).float()
    w2 = torch.zeros(C, inner)
    nz = min(128, inner)
    for r in range(C):
        w2[r, torch.randperm(inner, generator=g)[:nz]] = sign(nz).float()
    wp = torch.zeros(C, C)
    wp[torch.arange(C), torch.randperm(C, generator=g)] = (sign(C) * ri(1, 2, C)).float()
    o = {"h": h, "x0": ri(-4, 4, M, C).float(), "w1": w1, "b1": b1, "w2": w2, "b2": ri(-3, 3, C).float(), "wp": wp, "bp": ri(-3, 3, C).float(),
         "gamma": torch.ones(C), "beta": torch.zeros(C)}
    return {k: v.to(dt) for k, v in o.items()}


_EXACT_SHAPES = {"m384_i128_po": (384, 128, True), "m2176_i1280_po": (2176, 1280, True), "m1000_i64": (1000, 64, False)}      # (M, inner, proj_out tail)
_EXACT_KEYS = ("h", "x0", "w1", "b1", "w2", "b2", "wp", "bp", "gamma", "beta")          # the fixed order of the golden's operand digest
_GOLD = []


def _one_wave_golden():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rc_ff_one_wave_exact.npz")))
    return _GOLD[0]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("sid", list(_EXACT_SHAPES))
def test_exact_operands_match_the_one_wave_kernel_bit_for_bit(sid, dname):
    """The one-wave kernel is retired: its outputs on these operands were recorded once, at the last commit that had it, into
    tests/golden/rc_ff_one_wave_exact.npz (``meta`` there: commit, command, library digest) — per (shape, dtype) the sha256 of the output rows' int16
    view and of the operands' bytes, and the whole output of the smallest shape."""
    gold = _one_wave_golden()
    M, inner, proj = _EXACT_SHAPES[sid]
    o = _exact_operands(M, inner, DTYPES[dname], 7)
    raw = lambda t: t.detach().cpu().contiguous().view(torch.int16).numpy()
    digest = hashlib.sha256()
    for k in _EXACT_KEYS:
        digest.update(raw(o[k]).tobytes())
    assert digest.hexdigest() == str(gold[f"operands_sha256/{sid}/{dname}"]), "operands changed: _exact_operands no longer generates what the golden was recorded on"
    new, _ = launch(o, (M, inner, proj, (352, 328, 384)), eps=3.0)
    assert torch.isfinite(new).all() and new.float().abs().max() > 16          # the operands do reach the outputs
    got = raw(new)
    if f"out/{sid}/{dname}" in gold.files:
        diff = got != gold[f"out/{sid}/{dname}"]
        assert not bool(diff.any()), f"{int(diff.sum())} of {diff.size} elements differ, first at {np.argwhere(diff)[0].tolist()}"
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(gold[f"out_sha256/{sid}/{dname}"]), "kernel changed: the output rows differ from the one-wave kernel's"


def test_deterministic_and_guard_rows_untouched():
    case, dname = "m1000_i128_po", "bf16"
    from theatergen_amd import ops, rowchain
    o = operands(case, dname)
    M, inner, _, _ = CASES[case]
    dev = lambda k: o[k].to(DEV)
    s1, s2, bb2 = rowchain.pack_ff2(dev("w1"), dev("b1"), dev("gamma"), dev("beta"), dev("w2"), dev("b2"))
    wpo = rowchain.pack_po2(dev("wp"), dev("bp").float())
    G, runs = 32, []
    for _ in range(2):
        buf = torch.full((M + 2 * G, C), float("nan"), dtype=o["h"].dtype, device=DEV)
        guard = buf.view(torch.int16).clone()
        ops.rc_ff(dev("h"), s1, s2, bb2, inner, 1e-5, wpo=wpo, res0=dev("x0"), out=buf[G:G + M])
        torch.cuda.synchronize()
        now = buf.view(torch.int16)
        assert torch.equal(now[:G], guard[:G]) and torch.equal(now[G + M:], guard[G + M:]), "a guard row changed"
        runs.append(buf[G:G + M].clone())
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))


def test_run_fused_routes_by_mode_bit(monkeypatch):
    """``TG_RC_MODE`` bit 2 routes the feed-forward through ``tg_rc_ff``: below ``MIN_ROWS_CHAIN`` no launch, above it exactly one, within the fp64 bound
    of a single launch.  Bit 5, which once chose between two kernels, is ignored: 15 and 47 take the same path"""
    from theatergen_amd import ops, rowchain
    from theatergen_amd.unet import FeedForward
    torch.manual_seed(3)
    dt, M = torch.bfloat16, 384
    ff = FeedForward(C).to(DEV, dt)
    norm = torch.nn.LayerNorm(C).to(DEV, dt)
    with torch.no_grad():
        norm.weight.add_(0.1 * torch.randn(C, device=DEV))
        norm.bias.add_(0.1 * torch.randn(C, device=DEV))
    x = (torch.randn(M, C, device=DEV) * 1.2).to(dt)
    wp, bp, x0 = (torch.randn(C, C, device=DEV) / C ** 0.5).to(dt), torch.randn(C, device=DEV).to(dt), torch.randn(M, C, device=DEV).to(dt)
    d = lambda t: t.detach().double()
    xn = F.layer_norm(d(x), (C,), d(norm.weight), d(norm.bias), norm.eps)
    pr = xn @ d(ff.net[0].proj.weight).T + d(ff.net[0].proj.bias)
    h3 = (pr[:, :4 * C] * F.gelu(pr[:, 4 * C:])) @ d(ff.net[2].weight).T + d(ff.net[2].bias) + d(x)
    ref = h3 @ d(wp).T + d(bp) + d(x0)
    seen, orig = [], ops.rc_ff

    def rec(*a, **k):
        seen.append(k)
        return orig(*a, **k)
    monkeypatch.setattr(ops, "rc_ff", rec)
    for mode in (15, 47):
        with monkeypatch.context() as m:
            del seen[:]
            m.setattr(rowchain, "MODE", mode)
            assert ff.run_fused(x, norm, (wp, bp, x0)) is None and seen == []          # 384 rows: below MIN_ROWS_CHAIN
            m.setattr(rowchain, "MIN_ROWS_CHAIN", 128)
            got = ff.run_fused(x, norm, (wp, bp, x0))
            torch.cuda.synchronize()
            assert len(seen) == 1, (mode, seen)
            assert ((d(got) - ref).norm() / ref.norm()).item() < lc.l2_tol(dt)          # the project's single-launch bound (tests/launch_check.py)
