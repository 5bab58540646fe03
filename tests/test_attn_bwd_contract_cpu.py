"""CPU: pins tests/attn_bwd_contract.py (the fp64 restatement the GPU edge tests of the attention reverse pass compare against) and shows
that the comparison has teeth at the tolerances those tests use.

  * with the two roundings off the restatement IS fp64 autograd of  w softmax(s Q K^T) V (+ w <extra, P>)  (1e-10 of the peak);
  * an fp32 model of the kernels (statistics pass lse / D, then P = exp(s - lse), P and dS rounded to the storage dtype, fp32 accumulation,
    outputs rounded once) passes the whole-tensor and per-block comparison at 1.5 x launch_check's tolerances (4.5e-3 / 6e-4 rel-L2);
  * the same model with one realistic fault injected fails it; leaving dS unrounded does NOT (it is inside the rounding floor: the
    comparison does not claim to see which of two equally accurate roundings an implementation chose).
"""
import pytest
import torch

from tests import attn_bwd_contract as ab
from tests import launch_check as lc

DTYPES = [torch.bfloat16, torch.float16]
# (batch, n, heads, head_dim, q multiplier): 72 / 264 / 1096 all end in an 8-key ragged tile; x4 = a peaked softmax
SHAPES = [(2, 72, 3, 40, 1.0), (1, 264, 2, 64, 1.0), (1, 264, 2, 64, 4.0), (1, 1096, 2, 64, 1.0)]
WEIGHT = 0.4


def tols(dtype):
    return 1.5 * lc.l2_tol(dtype), 1.5 * lc.rel_tol(dtype)


def test_tolerances_are_the_per_launch_attention_bound():
    assert tols(torch.bfloat16) == pytest.approx((4.5e-3, 1.5e-2)) and tols(torch.float16) == pytest.approx((6e-4, 3.75e-3))


# ---- fp32 model of the kernels, with fault switches ----------------------------------------------------------------------------------
def _model_head(q, k, v, do, scale, ds_scale, extra, dtype, fault, want_kv):
    q, k, v, do = (t.float() for t in (q, k, v, do))
    nk = k.shape[0]
    tail0 = nk - nk % 64                                              # first key of the ragged last tile
    s = (q @ k.t()) * scale
    dP = do @ v.t()
    if extra is not None:
        e = extra.float().clone()
        if fault == "extra_skips_ragged_tile":
            e[:, tail0:] = 0
        dP = dP + e
    ns = tail0 if fault == "stats_drop_tail" else nk                 # keys the statistics pass sees
    lse = torch.logsumexp(s[:, :ns], dim=-1, keepdim=True)
    D = (torch.exp(s[:, :ns] - lse) * dP[:, :ns]).sum(-1, keepdim=True)
    P = torch.exp(s - lse)
    dS = (scale if fault == "ds_scale_is_scale" else ds_scale) * P * (dP - D)
    P = P.to(dtype).float()
    if fault != "ds_unrounded":
        dS = dS.to(dtype).float()
    dq = dS @ k
    return (dq, dS.t() @ q, P.t() @ do) if want_kv else (dq,)


def model(a, fault=None):
    """{"dq" (, "dk", "dv")}: the fp32 model over a descriptor, rounded once to the storage dtype"""
    cross = "n_q" in a
    B, H, D = a["batch"], a["heads"], a["head_dim"]
    ext = {r.name: r.view() for r in (ab.cross_read_extents(a) if cross else ab.self_read_extents(a))}
    dtype = ext["q"].dtype
    names = ("dq",) if cross else ("dq", "dk", "dv")
    out = {x: torch.empty((B, a["n_q"] if cross else a["n"], H * D), dtype=dtype) for x in names}
    for b in range(B):
        for h in range(H):
            cs = slice(h * D, (h + 1) * D)
            ex = ext["extra"][b, h] if "extra" in ext else None
            g = _model_head(ext["q"][b, :, cs], ext["k"][b, :, cs], ext["v"][b, :, cs], ext["dout"][b, :, cs], a["scale"],
                            a["ds_scale"] if cross else a["scale"], ex, dtype, fault, not cross)
            for x, t in zip(names, g):
                out[x][b, :, cs] = t.to(dtype)
    if fault == "dk_block_stale":                                     # the last (item, head)'s last 128-row block keeps what the buffer held
        n = a["n"]
        out["dk"][B - 1, (n - 1) // 128 * 128:, (H - 1) * D:] = 0
    if fault == "dv_heads_swapped":
        dv = out["dv"].clone()
        out["dv"][:, :, :D], out["dv"][:, :, D:2 * D] = dv[:, :, D:2 * D], dv[:, :, :D]
    return out


_CASES = {}


def case(kind, dtype, shape):
    """descriptor + fp64 reference, built once per (kind, dtype, shape) and left unchanged"""
    key = (kind, dtype, shape)
    if key not in _CASES:
        B, n, H, D, qmul = shape
        if kind == "self":
            a = ab.make_self_case(dtype, B, n, H, D, qmul=qmul)
            ref = ab.self_reference(a)
        else:
            a = ab.make_cross_case(dtype, B, n, n, H, D, qmul=qmul, with_extra=True, weight=WEIGHT)
            ref = ab.cross_reference(a)
        _CASES[key] = (a, ref)
    return _CASES[key]


def verdict(kind, dtype, shape, fault):
    a, ref = case(kind, dtype, shape)
    got = model(a, fault)
    l2, mx = tols(dtype)
    res = {x: ab.compare(got[x], ref[x], a["heads"], l2, mx) for x in got}
    for x, (ok, m) in res.items():
        print(f"{kind} {str(dtype)[6:]} {shape} fault={fault} {x}: ok={ok} rel_l2={m['rel_l2']:.2e} max={m['max_rel']:.2e} "
              f"block={m['block_rel_l2']:.2e}@{m['block_at']} block_max={m['block_max_rel']:.2e}")
    return res


# ---- the restatement is autograd's formula ------------------------------------------------------------------------------------------
def _heads(t, H):
    B, n, inner = t.shape
    return t.double().reshape(B, n, H, inner // H).permute(0, 2, 1, 3)


def _merge(t):
    B, H, n, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, H * D)


def _close(got, ref, what):
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    assert err <= 1e-10, f"{what}: {err:.2e} of the peak"


@pytest.mark.parametrize("layout", ["plain", "fused"])
def test_self_restatement_without_roundings_is_fp64_autograd(layout):
    a = ab.make_self_case(torch.bfloat16, 2, 72, 3, 40, layout=layout)
    assert ab.transposes_consistent(a)
    H = a["heads"]
    ext = {r.name: r.view() for r in ab.self_read_extents(a)}
    q, k, v = (_heads(ext[x], H).clone().requires_grad_(True) for x in ("q", "k", "v"))
    o = torch.softmax(a["scale"] * (q @ k.transpose(-1, -2)), -1) @ v
    want = torch.autograd.grad(o, [q, k, v], _heads(ext["dout"], H))
    got = ab.self_reference(a, rounded=False)
    for x, w in zip(("dq", "dk", "dv"), want):
        _close(got[x], _merge(w), f"{x} ({layout})")
    rounded = ab.self_reference(a)
    assert all(not torch.equal(rounded[x], got[x]) for x in got), "the roundings of P / dS are switched on by default"


@pytest.mark.parametrize("layout", ["plain", "pitched"])
@pytest.mark.parametrize("with_extra", [False, True])
def test_cross_restatement_without_roundings_is_fp64_autograd(layout, with_extra):
    """ds_scale = 0.4 x scale: the loss is  w (<dO, P V> + <extra, P>)  — ``extra`` is per unit of the segment's weight"""
    a = ab.make_cross_case(torch.float16, 2, 100, 77, 3, 40, with_extra=with_extra, weight=WEIGHT, layout=layout)
    assert ab.transposes_consistent(a) and a["ds_scale"] != a["scale"]
    H = a["heads"]
    ext = {r.name: r.view() for r in ab.cross_read_extents(a)}
    q = _heads(ext["q"], H).clone().requires_grad_(True)
    P = torch.softmax(a["scale"] * (q @ _heads(ext["k"], H).transpose(-1, -2)), -1)
    outs, grads = [WEIGHT * (P @ _heads(ext["v"], H))], [_heads(ext["dout"], H)]
    if with_extra:
        outs.append(P)
        grads.append(WEIGHT * ext["extra"].double())
    want = torch.autograd.grad(outs, q, grads)[0]
    _close(ab.cross_reference(a, rounded=False)["dq"], _merge(want), f"cross dq ({layout}, extra={with_extra})")


def test_reference_reads_through_the_pitches():
    """the pitched descriptors hold NaN wherever the contract does not read: a reference that walked the wrong pitch would return NaN;
    the same data in both layouts gives the same result"""
    for dtype in DTYPES:
        p, f = (ab.make_self_case(dtype, 2, 72, 3, 40, layout=lay) for lay in ("plain", "fused"))
        rp, rf = ab.self_reference(p), ab.self_reference(f)
        assert all(torch.equal(rp[x], rf[x]) and bool(torch.isfinite(rf[x]).all()) for x in rp)
        cp, cf = (ab.make_cross_case(dtype, 2, 100, 77, 3, 40, layout=lay) for lay in ("plain", "pitched"))
        assert torch.equal(ab.cross_reference(cp)["dq"], ab.cross_reference(cf)["dq"])
        regs = {r.name: r for r in ab.self_written_region(f)}
        assert regs["dq"].sizes == (2, 72, 120) and regs["dq"].strides == (77 * 368, 368, 1) and regs["stats"].sizes == (2, 3, 72, 2)


# ---- a correct implementation passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_fp32_model_passes_whole_tensor_and_every_block(kind, dtype, shape):
    for x, (ok, m) in verdict(kind, dtype, shape, None).items():
        assert ok, f"{kind} {x} {shape} {dtype}: {m}"
    a, ref = case(kind, dtype, shape)
    fn = ab.self_reference if kind == "self" else ab.cross_reference
    r32 = fn(a, work=torch.float32, round_out=True)
    l2, mx = tols(dtype)
    for x in ref:
        ok, m = ab.compare(r32[x], ref[x], a["heads"], l2, mx)
        assert ok, f"fp32 restatement {kind} {x} {shape} {dtype}: {m}"


# ---- injected faults ---------------------------------------------------------------------------------------------------------------
BF16, FP16 = torch.bfloat16, torch.float16
# fault -> (kind, the (dtype, shape) at which it must FAIL, the outputs that fail there)
FAULTS = {
    # the statistics pass masks the whole ragged tile (8 of 1096 keys): the hardest of the four shapes, in the looser dtype
    "stats_drop_tail": ("self", BF16, SHAPES[3], ("dq", "dk", "dv")),
    # 8 of 72 keys lose their d loss / d P
    "extra_skips_ragged_tile": ("cross", BF16, SHAPES[0], ("dq",)),
    "ds_scale_is_scale": ("cross", BF16, SHAPES[1], ("dq",)),
    # one of 18 (item, head, block) units: the block figure is 1.0 where the whole tensor shows its share only
    "dk_block_stale": ("self", BF16, SHAPES[3], ("dk",)),
    "dv_heads_swapped": ("self", BF16, SHAPES[2], ("dv",)),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_injected_fault_fails_the_comparison(fault):
    kind, dtype, shape, outs = FAULTS[fault]
    res = verdict(kind, dtype, shape, fault)
    for x in outs:
        assert not res[x][0], f"{fault}: {x} passed {res[x][1]}"
    for x in set(res) - set(outs):
        assert res[x][0], f"{fault}: {x} is not touched by this fault and must pass {res[x][1]}"


def test_stale_block_shows_at_full_size_in_the_block_figure():
    res = verdict("self", BF16, SHAPES[3], "dk_block_stale")
    m = res["dk"][1]
    assert m["block_rel_l2"] > 0.99 and m["block_at"] == [0, 1, 8] and m["rel_l2"] < 0.2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_unrounded_ds_is_inside_the_floor_and_passes(dtype, shape):
    """what the comparison does NOT claim: an implementation that keeps dS in fp32 is as close to the restatement as one that rounds it"""
    for kind in ("self", "cross"):
        for x, (ok, m) in verdict(kind, dtype, shape, "ds_unrounded").items():
            assert ok, f"{kind} {x} {shape} {dtype}: {m}"


# ---- the x8 input of the GPU edge tests ---------------------------------------------------------------------------------------------
X8 = (1, 264, 2, 64, 8.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_x8_peaked_softmax_is_a_well_conditioned_input(kind, dtype):
    """Q x8: scores of spread 8, most rows hold one probability above 1/2 and a quarter one above 0.9 (P o (dP - D) cancels there).  The reference stays well conditioned —
    the fp32 model, whose statistics carry fp32 rounding of scores ~ 30, still passes at the unchanged tolerances — so the GPU edge tests
    use this input as it stands."""
    a, ref = case(kind, dtype, X8)
    ext = {r.name: r.view() for r in (ab.cross_read_extents(a) if kind == "cross" else ab.self_read_extents(a))}
    q, k = ext["q"][0, :, :64].double(), ext["k"][0, :, :64].double()
    pmax = torch.softmax(a["scale"] * (q @ k.t()), -1).amax(-1)
    assert float((pmax > 0.5).double().mean()) > 0.5, "not peaked: under half of the rows have one probability above 1/2"
    for x, (ok, m) in verdict(kind, dtype, X8, None).items():
        assert ok and m["finite"], f"{kind} {x} {dtype}: {m}"
