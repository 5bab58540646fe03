"""GPU: ``tg_attention_bwd_wide`` / ``tg_attention_bwd_cross_wide`` (csrc/tg_attention_bwd.hip: the recompute reverse pass of attention for
64 < head_dim <= 160 — SD-1.5's inner levels) against the fp64 restatement of the C-ABI contract (tests/attn_bwd_contract.py), the ``ops``
wrappers, and the opt-in routing of ``backward.attention_input_grad`` (``backward.FLASH_BWD_WIDE``).

Every descriptor case gets the three checks of tests/test_attn_bwd_edges_gpu.py::run_case — comparison with the restatement (whole tensor and
every (item, head, 128-row block)), sentinel bytes outside the written region untouched, a replay into NaN-filled outputs with the same bits and
no NaN — by pointing that module's ``descriptor`` at the wide entry points.  Inputs hold NaN in every element the contract does not read.

Tolerances: that file's (1.5 x launch_check's per-launch bound: rel-L2 4.5e-3 bf16 / 6e-4 fp16, max 1.5e-2 / 3.75e-3 of the peak).  The fp32
model of the kernels sits at 2.1e-3 / 2.5e-4 in the worst block at these shapes (tests/test_attn_bwd_wide_cpu.py).

Shapes: head dims whose cut falls inside a 16-wide k-step (72, 104, 136), inside a 32-wide output tile (72, 80, 104, 136), on the 64-column
panel boundary (128), and on both sides of the output split (96: one workgroup of three tiles; 104: two workgroups of two) and of the
k-step / tile instances (<= 96, <= 128, <= 160).
"""
import ctypes as C

import pytest
import torch

from tests import attn_bwd_contract as ab
from tests import parity_metrics as pm
from tests import test_attn_bwd_edges_gpu as edges

pytestmark = pytest.mark.gpu
DEV = edges.DEV
DTYPES = edges.DTYPES
TG_ERR_ARG, TG_ERR_UNSUPPORTED = -1, -3
_name = edges._name
_T = edges._gpu_transpose
_narrow_descriptor = edges.descriptor


def _wide_descriptor(a):
    from theatergen_amd import _lib
    d, _ = _narrow_descriptor(a)
    L = _lib.lib()
    return d, (L.tg_attention_bwd_cross_wide if "n_q" in a else L.tg_attention_bwd_wide)


@pytest.fixture(autouse=True)
def _wide_entry_points(monkeypatch):
    monkeypatch.setattr(edges, "descriptor", _wide_descriptor)


def run_case(a, what):
    assert edges.descriptor is _wide_descriptor
    return edges.run_case(a, "wide " + what)


# ---- self-attention ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [72, 80, 96, 104, 128, 136, 160])
def test_self_head_dims(dtype, d):
    a = ab.make_self_case(dtype, 1, 136, 3, d, device=DEV, transpose=_T)
    run_case(a, f"self n=136 d={d} {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [80, 160])
@pytest.mark.parametrize("n", [8, 64, 72, 128, 136, 264])
def test_self_sequence_lengths(dtype, n, d):
    """2 items x 2 heads: one partial tile (8), exact tile boundaries (64 — at d = 160 SD-1.5's mid block — and 128), an 8-row ragged tile
    (72, 136), three row blocks and the remainder branch of the XCD walk (264: 12 workgroups at d = 80, 24 halves at d = 160, statistics 12)"""
    a = ab.make_self_case(dtype, 2, n, 2, d, device=DEV, transpose=_T)
    run_case(a, f"self n={n} d={d} {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_grid_not_a_multiple_of_eight(dtype):
    """3 items x 3 heads x 2 row blocks = 18 workgroups, distinct data per (item, head)"""
    a = ab.make_self_case(dtype, 3, 136, 3, 80, device=DEV, transpose=_T)
    q = a["q"].reshape(3, 136, 3, 80)
    assert len({float(q[b, :, h].double().sum()) for b in range(3) for h in range(3)}) == 9
    run_case(a, f"self grid 3x3x136 d=80 {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [80, 160])
def test_self_fused_qkv_buffer_and_padded_pitches(dtype, d):
    a = ab.make_self_case(dtype, 2, 136, 2, d, device=DEV, layout="fused", transpose=_T)
    assert a["ld"] == 3 * 2 * d + 8 and a["t_ld"] == 144 and a["q"].data_ptr() != a["k"].data_ptr()
    assert a["k"].untyped_storage().data_ptr() == a["q"].untyped_storage().data_ptr() == a["v"].untyped_storage().data_ptr()
    run_case(a, f"self fused n=136 d={d} {_name(dtype)}")


# ---- cross-attention -----------------------------------------------------------------------------------------------------------------
CROSS_PAIRS = [(100, 1), (1, 4), (130, 8), (128, 64), (130, 65), (100, 77), (130, 129)]      # (n_q, n_k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("d", [80, 160])
@pytest.mark.parametrize("n_q,n_k", CROSS_PAIRS)
def test_cross_key_and_query_counts(dtype, n_q, n_k, d, with_extra):
    """2 items x 3 heads, ds_scale = 0.4 x scale, every row-major operand pitched with a gap between items, extra_ld = n_k + 3 with NaN in the
    pad, kt zero in columns [n_k, roundup8(n_k)) and NaN in the eight columns after them"""
    a = ab.make_cross_case(dtype, 2, n_q, n_k, 3, d, device=DEV, with_extra=with_extra, weight=0.4, layout="pitched", transpose=_T)
    assert a["extra_ld"] == n_k + 3 and abs(a["ds_scale"] - 0.4 * a["scale"]) < 1e-12 and (a["extra"] is not None) == with_extra
    run_case(a, f"cross nq={n_q} nk={n_k} d={d} extra={with_extra} {_name(dtype)}")


# ---- peaked softmax ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [80, 160])
@pytest.mark.parametrize("qmul", [4.0, 8.0])
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_peaked_softmax(dtype, kind, qmul, d):
    if kind == "self":
        a = ab.make_self_case(dtype, 1, 264, 2, d, device=DEV, qmul=qmul, transpose=_T)
    else:
        a = ab.make_cross_case(dtype, 1, 264, 264, 2, d, device=DEV, qmul=qmul, with_extra=True, weight=0.4, transpose=_T)
    for m in run_case(a, f"{kind} peaked x{qmul:g} n=264 d={d} {_name(dtype)}").values():
        assert m["finite"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_return_the_documented_error_and_write_nothing(dtype):
    mk = dict(device=DEV, transpose=_T)
    ref = edges._refused
    for hd in (64, 76, 168):
        # head dim 76: the operands are built at 80 (make_*_case needs pitches of 8) and the descriptor's head_dim is edited
        build = 80 if hd == 76 else hd
        ref(ab.make_self_case(dtype, 1, 64, 1, build, **mk), TG_ERR_UNSUPPORTED, f"wide self head_dim {hd}", lambda d, hd=hd: setattr(d, "head_dim", hd))
        ref(ab.make_cross_case(dtype, 1, 64, 77, 1, build, **mk), TG_ERR_UNSUPPORTED, f"wide cross head_dim {hd}",
            lambda d, hd=hd: setattr(d, "head_dim", hd))
    ref(ab.make_self_case(dtype, 1, 60, 1, 80, **mk), TG_ERR_UNSUPPORTED, "wide self n % 8 != 0")
    ref(ab.make_self_case(dtype, 1, 64, 2, 80, **mk), TG_ERR_ARG, "wide self t_ld < n", lambda d: setattr(d, "t_ld", 56))
    ref(ab.make_cross_case(dtype, 1, 64, 77, 2, 80, **mk), TG_ERR_ARG, "wide cross extra_ld < n_k", lambda d: setattr(d, "extra_ld", 76))
    ref(ab.make_cross_case(dtype, 1, 64, 77, 2, 80, **mk), TG_ERR_ARG, "wide cross kt pitch below the padded key count",
        lambda d: setattr(d, "t_ld", 72))
    for field in ("q", "k", "v", "dout", "qt", "kt", "doutt", "stats", "dq", "dk", "dv"):
        ref(ab.make_self_case(dtype, 1, 64, 2, 80, **mk), TG_ERR_ARG, f"wide self null {field}", lambda d, f=field: setattr(d, f, None))
    for field in ("q", "dout", "k", "v", "kt", "stats", "dq"):
        ref(ab.make_cross_case(dtype, 1, 64, 77, 2, 80, **mk), TG_ERR_ARG, f"wide cross null {field}", lambda d, f=field: setattr(d, f, None))


# ---- ops wrappers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ops_wrappers_against_the_contract(dtype):
    from theatergen_amd import ops
    l2, mx = edges.tols(dtype)
    a = ab.make_self_case(dtype, 2, 264, 2, 80, device=DEV, transpose=_T)
    ref, mag = ab.self_reference(a), ab.self_reference(a, magnitude=True)
    flat = [a[x].reshape(2 * 264, 160) for x in ("q", "k", "v", "dout")]
    got = ops.attention_bwd_wide(*flat, 2, 264, 2, 80, a["scale"])
    torch.cuda.synchronize()
    for x, g in zip(("dq", "dk", "dv"), got):
        ab.check(g.reshape(2, 264, 160), ref[x], 2, f"ops.attention_bwd_wide {x} {_name(dtype)}", l2, mx, mag[x])
    c = ab.make_cross_case(dtype, 2, 130, 77, 2, 160, device=DEV, with_extra=True, weight=0.4, transpose=_T)
    cref, cmag = ab.cross_reference(c), ab.cross_reference(c, magnitude=True)
    dq = ops.attention_bwd_cross_wide(c["q"].reshape(260, 320), c["dout"].reshape(260, 320), c["k"].reshape(154, 320), c["v"].reshape(154, 320),
                                      2, 130, 77, 2, 160, c["scale"], c["ds_scale"], extra=c["extra"])
    torch.cuda.synchronize()
    ab.check(dq.reshape(2, 130, 320), cref["dq"], 2, f"ops.attention_bwd_cross_wide dq {_name(dtype)}", l2, mx, cmag["dq"])
    with pytest.raises(RuntimeError, match="theatergen_hip error"):
        ops.attention_bwd_wide(*[t[:, :128].contiguous() for t in flat], 2, 264, 2, 64, 0.125)


# ---- routing -------------------------------------------------------------------------------------------------------------------------
ROUTE_OPS = ("attention_bwd", "attention_bwd_cross", "attention_bwd_wide", "attention_bwd_cross_wide", "attn_probs", "softmax_rows", "softmax_bwd_rows")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [64, 264])
def test_routed_self_attention_input_gradient_head_dim_80(dtype, N, monkeypatch):
    """the scenario of test_materialised_self_attention_input_gradient_head_dim_80 with the switch on: one wide call, nothing materialised"""
    from oracle import attention as oa
    from tests.golden import gen_common as gg
    from theatergen_amd import backward
    from theatergen_amd.attention_processor import Attention, AttnProcessor
    monkeypatch.setattr(backward, "FLASH_BWD_WIDE", True)
    g = torch.Generator().manual_seed(80 + N)
    heads, B = 2, 2
    Cc = heads * 80
    l2, mx = edges._fallback_tols(dtype)
    ws = gg.attn_weights(Cc, Cc, seed=21, with_ip=False)
    wsr = {k: v.to(dtype).double() for k, v in ws.items()}
    h = (torch.randn((B, N, Cc), generator=g)).to(dtype)
    dout = (torch.randn((B * N, Cc), generator=g)).to(dtype)
    attn = Attention(query_dim=Cc, heads=heads, dim_head=80)
    attn.load_state_dict(ws)
    attn = attn.to(DEV, dtype)
    hr = h.double().clone().requires_grad_(True)
    ref = torch.autograd.grad(oa.attn_processor(wsr, heads, hr), hr, dout.double().reshape(B, N, Cc))[0].reshape(B * N, Cc)
    calls = edges._count_ops(monkeypatch, ROUTE_OPS)
    got = backward.attention_input_grad(attn, AttnProcessor(), h.to(DEV).reshape(B * N, Cc), B, N, None, dout.to(DEV), None)
    torch.cuda.synchronize()
    assert calls == dict.fromkeys(ROUTE_OPS, 0) | {"attention_bwd_wide": 1}, calls
    pm.check(got, ref, f"wide-routed self-attention input grad d=80 N={N} {dtype}", l2, mx)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ip_scale", [0.4, 0.0])
def test_routed_ip_cross_attention_input_gradient_head_dim_80(dtype, ip_scale, monkeypatch):
    """the scenario of test_materialised_ip_cross_attention_input_gradient_head_dim_80 with the switch on: one wide call per non-zero segment
    (an IP scale of 0 skips the image segment)"""
    from oracle import attention as oa
    from tests.golden import gen_common as gg
    from theatergen_amd import backward
    from theatergen_amd.attention_processor import Attention, IPAttnProcessor
    monkeypatch.setattr(backward, "FLASH_BWD_WIDE", True)
    g = torch.Generator().manual_seed(81)
    heads, B, N, T, ctx = 2, 2, 72, 4, 64
    Cc = heads * 80
    l2, mx = edges._fallback_tols(dtype)
    w = gg.attn_weights(Cc, ctx, seed=22)
    wr = {k: v.to(dtype).double() for k, v in w.items()}
    h = (torch.randn((B, N, Cc), generator=g)).to(dtype)
    enc = (torch.randn((B, 77 + T, ctx), generator=g) * 0.5).to(dtype)
    dout = (torch.randn((B * N, Cc), generator=g)).to(dtype)
    extra = torch.randn(B, heads, N, 77, generator=g) * 0.2
    attn = Attention(query_dim=Cc, cross_attention_dim=ctx, heads=heads, dim_head=80)
    attn.load_state_dict({k: v for k, v in w.items() if "_ip" not in k})
    attn = attn.to(DEV, dtype)
    proc = IPAttnProcessor(hidden_size=Cc, cross_attention_dim=ctx, scale=ip_scale, num_tokens=T)
    proc.load_state_dict({"to_k_ip.weight": w["to_k_ip.weight"], "to_v_ip.weight": w["to_v_ip.weight"]})
    proc = proc.to(DEV, dtype)
    hr = h.double().clone().requires_grad_(True)
    out, probs = oa.ip_attn_processor(wr, heads, hr, enc.double(), ip_scale, T, return_probs=True)
    ref = torch.autograd.grad([out, probs], hr, [dout.double().reshape(B, N, Cc), extra.double()])[0].reshape(B * N, Cc)
    calls = edges._count_ops(monkeypatch, ROUTE_OPS)
    got = backward.attention_input_grad(attn, proc, h.to(DEV).reshape(B * N, Cc), B, N, enc.to(DEV), dout.to(DEV), extra.to(DEV))
    torch.cuda.synchronize()
    assert calls == dict.fromkeys(ROUTE_OPS, 0) | {"attention_bwd_cross_wide": 2 if ip_scale else 1}, calls
    pm.check(got, ref, f"wide-routed ip cross-attention input grad d=80 ip_scale={ip_scale} {dtype}", l2, mx)


# ---- the whole reverse pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_unet_latent_gradient_with_the_wide_route(dtype, monkeypatch):
    """``UNetInputGrad`` on config.tiny() (head dims 32 / 64 / 128 / 128: level 2 and the mid block go wide) with the switch on: the ratio-loss
    gradient vs oracle autograd at the tolerances of test_backward_gpu.py::test_unet_latent_gradient_and_guided_update (bf16 5e-2 / 1e-1, fp16
    8e-3 / 2e-2), equal bits over two runs and from a ``GraphedInputGrad`` replay, and no materialised softmax backward anywhere"""
    from oracle import guidance_loss as og
    from oracle import unet as ou
    from tests.golden import gen_common as gc
    from tests.test_backward_gpu import GUIDE_RATIO, _build
    from theatergen_amd import backward, config
    from theatergen_amd import guidance as G
    monkeypatch.setattr(backward, "FLASH_BWD_WIDE", True)
    cfg = config.tiny()
    unet, sd_r = _build(cfg, dtype)
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(1, 4, 32, 32, generator=g)
    enc = torch.randn(1, 81, cfg.cross_attention_dim, generator=g) * 0.5
    keys = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
    boxes, pos = gc.GUIDANCE_BOXES[2], gc.GUIDANCE_POSITIONS[2]
    t, loss_scale = 741, 30.0
    x = lat.to(dtype).float().clone().requires_grad_(True)
    saved = {}
    ou.unet_forward(cfg, sd_r, x, t, enc.to(dtype).float(), ip_scale=0.4, cross_attention_kwargs={"save_attn_to_dict": saved, "save_keys": keys})
    loss_ref = og.compute_ca_lossv3(saved, boxes, pos, keys, **GUIDE_RATIO) * loss_scale
    grad_ref = torch.autograd.grad(loss_ref, x)[0]

    def loss_fn(sv):
        return G.compute_ca_lossv3(sv, boxes, pos, keys, return_grads=True, loss_scale=loss_scale, **GUIDE_RATIO)
    calls = edges._count_ops(monkeypatch, ("attention_bwd_wide", "attention_bwd_cross_wide", "softmax_bwd_rows"))
    loss, grad = backward.UNetInputGrad(unet).loss_and_grad(lat.to(DEV, dtype), t, enc.to(DEV, dtype), loss_fn, keys)
    torch.cuda.synchronize()
    assert calls["softmax_bwd_rows"] == 0 and calls["attention_bwd_wide"] > 0 and calls["attention_bwd_cross_wide"] > 0, calls
    assert abs(loss.item() - loss_ref.item()) <= 2e-2 * abs(loss_ref.item())
    m = pm.metrics(grad, grad_ref)
    pm.record(f"d loss / d latents, tiny UNet, wide route, ratio loss {dtype}", m)
    l2, mx = (5e-2, 1e-1) if dtype == torch.bfloat16 else (8e-3, 2e-2)
    assert m["finite"] and m["rel_l2"] <= l2 and m["max_rel"] <= mx, m
    loss2, grad2 = backward.UNetInputGrad(unet).loss_and_grad(lat.to(DEV, dtype), t, enc.to(DEV, dtype), loss_fn, keys)
    assert torch.equal(grad, grad2) and loss.item() == loss2.item()
    gig = backward.GraphedInputGrad(unet, lat.to(DEV, dtype), t, enc.to(DEV, dtype), loss_fn, keys, streams=3)
    loss3, grad3 = gig.run()
    torch.cuda.synchronize()
    assert torch.equal(grad3, grad) and loss3.item() == loss.item()
    assert calls["softmax_bwd_rows"] == 0, calls
    del gig
