"""GPU: the IP-Adapter scale as a per-batch-item value, from the three kernels up to the batched stage-1 function.

Kernel level (``tg_attention_ps`` / ``tg_rc_xattn_ps`` / ``tg_xq_attn_ps`` through ``ops``), one vector with distinct values that include 0 at an odd
batch (the XCD-chunked block order then mixes items inside an XCD's chunk):
  1. bit identity per item: the rows of item b of the per-item launch ARE the rows of item b of a scalar launch through the old entry point with
     scale[b] — the value enters the same instruction, read from another address; no tolerance;
  2. every launch against the fp32 / fp64 restatement the kernel's own test uses, at that test's tolerance (helpers copied from
     test_kernels_gpu.py, test_rowchain_gpu.py, test_round5_gpu.py, test_xq_d64_gpu.py);
  3. count 0 and count 1 through a new entry point give the bits of the old entry point.
Processor level: ``IPAttnProcessor`` on its three routes (row chain, fused to_q + attention, three launches), vector vs per-item scalars, bit for bit;
the refusals.  Engine level: ``DenoiseEngine.set_ip_scale`` on the tiny plan.  Stage function: ``pipelines.generate_characters``.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SCALES = [0.0, 0.4, 1.7]
B3 = len(SCALES)


# ---- tolerances and checks, copied from the kernels' own tests ---------------------------------------------------------------------------
def attn_tols(dtype):
    """test_kernels_gpu.py: l2_tol / rel_tol, and test_attention's factor 1.5"""
    return ((3.0e-3, 1.0e-2) if dtype == torch.bfloat16 else (4.0e-4, 2.5e-3)), 1.5


def rc_tols(dtype):
    """test_rowchain_gpu.py::tols"""
    return (3e-3, 1e-2) if dtype == torch.bfloat16 else (4e-4, 2.5e-3)


def xq_tols(dtype):
    """test_round5_gpu.py::test_xq_attn_vs_fp32_reference and test_xq_d64_gpu.py::test_xq_attn_d64_vs_fp64_restatement"""
    return (4e-3, 1.2e-2) if dtype == torch.bfloat16 else (6e-4, 3e-3)


def check(got, ref, what, l2, mx):
    from tests import parity_metrics as pm
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, f"{what}: {got.shape} vs {ref.shape}"
    m = pm.metrics(got, ref)
    print(f"{what}: rel-L2 {m['rel_l2']:.3e} (<= {l2:.1e}) max {m['max_rel']:.3e} (<= {mx:.1e})")
    return pm.check(got, ref, what, l2, mx)


def net_tol(dtype):
    """test_hotpath_gpu.py::net_tol, the bar of test_denoise_engine_vs_oracle_loop: max, with rel-L2 at half of it"""
    return 6e-2 if dtype == torch.bfloat16 else 1.5e-2


def close(got, ref, tol, what):
    return check(torch.as_tensor(got), torch.as_tensor(ref), what, tol / 2, tol)


def rnd(shape, dtype, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _spy(monkeypatch, names):
    """wrap ``theatergen_amd.ops.<name>``: how often each launch ran, and the element count of the IP scale it was given"""
    from theatergen_amd import ops
    calls = {n: [] for n in names}
    for n in names:
        orig = getattr(ops, n)

        def wrapper(*a, _o=orig, _n=n, **k):
            s = k.get("ip_scale", k.get("w1_dev"))
            calls[_n].append(None if s is None else int(s.numel()))
            return _o(*a, **k)
        monkeypatch.setattr(ops, n, wrapper)
    return calls


def _through_new_entry(monkeypatch, old, count):
    """route ``ops``' scalar-form call of ``old`` through ``old + '_ps'`` with ``count`` (0 or 1)"""
    from theatergen_amd import _lib
    h = _lib.lib()
    new = getattr(h, old + "_ps")
    monkeypatch.setattr(h, old, lambda d, s, _new=new, _c=count: _new(d, _c, s))


# ---- tg_attention ------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, heads, scale):
    B, N, Cc = q.shape
    d = Cc // heads
    qh = q.float().reshape(B, N, heads, d).permute(0, 2, 1, 3)
    kh = k.float().reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    vh = v.float().reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    p = (qh @ kh.transpose(-1, -2) * scale).softmax(-1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(B, N, Cc)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("len1", [4, 16])
def test_attention_per_item_scale(dtype, d, len1, monkeypatch):
    """heads 2, n_q 160 (a partial second query block), 77 text keys, 4 / 16 image keys; d = 40 is the FOLD instance"""
    from theatergen_amd import ops
    heads, n_q, len0, B = 2, 160, 77, B3
    Cc = heads * d
    g = torch.Generator().manual_seed(1000 + d + len1)
    q = rnd((B, n_q, Cc), dtype, g)
    k0, v0, k1, v1 = rnd((B, len0, Cc), dtype, g), rnd((B, len0, Cc), dtype, g), rnd((B, len1, Cc), dtype, g), rnd((B, len1, Cc), dtype, g)
    scale = d ** -0.5
    ref0, ref1 = _attn_ref(q, k0, v0, heads, scale), _attn_ref(q, k1, v1, heads, scale)
    pad0, pad1 = (len0 + 7) // 8 * 8, (len1 + 7) // 8 * 8
    vt0 = torch.full((B, Cc, pad0), float("nan"), dtype=dtype)            # padding columns poisoned: never read as data
    vt0[:, :, :len0] = v0.permute(0, 2, 1)
    vt1 = torch.full((B, Cc, pad1), float("nan"), dtype=dtype)
    vt1[:, :, :len1] = v1.permute(0, 2, 1)
    qd, k0d, vt0d, k1d, vt1d = (t.to(DEV) for t in (q, k0, vt0, k1, vt1))

    def run(w):
        out = torch.zeros((B, n_q, Cc), dtype=dtype, device=DEV)
        ops.attention(qd, Cc, n_q * Cc, k0d, Cc, len0 * Cc, vt0d, pad0, Cc * pad0, len0, B, heads, d, n_q, scale, out, Cc, n_q * Cc,
                      k1=k1d, k1_ld=Cc, k1_bs=len1 * Cc, vt1=vt1d, vt1_ld=pad1, vt1_bs=Cc * pad1, len1=len1, w1=123.0, w1_dev=w)
        return out
    (l2, mx), f = attn_tols(dtype)
    what = f"attention d{d} len1 {len1} {dtype}"
    vec = torch.tensor(SCALES, device=DEV)
    got = run(vec)
    check(got, ref0 + vec.cpu().view(B, 1, 1) * ref1, what + " per item", l2 * f, mx * f)
    for b, s in enumerate(SCALES):
        one = run(torch.full((1,), s, device=DEV))                       # the old entry point, one float
        check(one, ref0 + s * ref1, what + f" scalar {s}", l2 * f, mx * f)
        assert torch.equal(got[b], one[b]), f"{what}: item {b} of the per-item launch differs from the scalar launch with {s}"
    assert not torch.equal(got[1], run(torch.full((1,), SCALES[2], device=DEV))[1]), "the values must matter for the test to mean anything"
    # count 0 / 1 through the new entry point = the old entry point
    old = run(torch.full((1,), 0.4, device=DEV))
    for count in (0, 1):
        with monkeypatch.context() as mp:
            _through_new_entry(mp, "tg_attention", count)
            assert torch.equal(run(torch.full((1,), 0.4, device=DEV)), old), f"{what}: tg_attention_ps(count {count}) != tg_attention"
    with pytest.raises(RuntimeError, match="2 elements"):
        run(torch.zeros(2, device=DEV))


def test_attention_wide_keeps_refusing_w1_dev():
    import ctypes as C
    from theatergen_amd import _lib
    d = _lib.AttnDesc()
    x = torch.zeros(8 * 512, dtype=torch.bfloat16, device=DEV)
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.len0 = 0, 1, 1, 512, 8, 8
    d.q = d.k0 = d.vt0 = d.out = x.data_ptr()
    d.q_ld = d.k0_ld = d.out_ld = 512
    d.vt0_ld, d.scale = 8, 512 ** -0.5
    d.w1_dev = torch.zeros(1, device=DEV).data_ptr()
    assert _lib.lib().tg_attention_wide(C.byref(d), None) == -3, "tg_attention_wide must refuse w1_dev (TG_ERR_UNSUPPORTED)"


# ---- tg_rc_xattn -------------------------------------------------------------------------------------------------------------------------------
def _rc_case(B, N, T, dtype, seed):
    """test_rowchain_gpu.py::_xattn_case with the image segment returned apart: ref(w) for w a number or a [B] tensor"""
    C, H, D, L = 320, 8, 40, 77
    g = torch.Generator().manual_seed(seed)
    M = B * N
    t = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
    h = (t(M, C, sc=1.2) + 0.2).to(dtype).to(DEV)
    wq = t(C, C, sc=C ** -0.5).to(dtype).to(DEV)
    wo = t(C, C, sc=C ** -0.5).to(dtype).to(DEV)
    bo = t(C, sc=0.1).to(dtype).to(DEV)
    gamma = (1 + 0.2 * t(C)).to(dtype).to(DEV)
    beta = t(C, sc=0.1).to(dtype).to(DEV)
    k = t(B * L, C).to(dtype).to(DEV)
    v = t(B, L, C).to(dtype).to(DEV)
    kip = t(B * T, C).to(dtype).to(DEV)
    vip = t(B, T, C).to(dtype).to(DEV)
    ldt, ldi = 80, 8 * ((T + 7) // 8)
    vt = torch.zeros(B, C, ldt, device=DEV, dtype=dtype); vt[:, :, :L] = v.transpose(1, 2)
    vtip = torch.zeros(B, C, ldi, device=DEV, dtype=dtype); vtip[:, :, :T] = vip.transpose(1, 2)
    scale = D ** -0.5
    x = F.layer_norm(h.float(), (C,), gamma.float(), beta.float(), 1e-5)
    q = (x @ wq.float().T).reshape(B, N, H, D).permute(0, 2, 1, 3)
    kk = k.float().reshape(B, L, H, D).permute(0, 2, 1, 3)
    vv = v.float().reshape(B, L, H, D).permute(0, 2, 1, 3)
    o_text = torch.softmax(q @ kk.transpose(-1, -2) * scale, -1) @ vv
    ki = kip.float().reshape(B, T, H, D).permute(0, 2, 1, 3)
    vi = vip.float().reshape(B, T, H, D).permute(0, 2, 1, 3)
    o_img = torch.softmax(q @ ki.transpose(-1, -2) * scale, -1) @ vi

    def ref(w):
        w = torch.as_tensor(w, dtype=torch.float32, device=DEV).reshape(-1, 1, 1, 1)
        return (o_text + w * o_img).permute(0, 2, 1, 3).reshape(M, C) @ wo.float().T + bo.float() + h.float()
    return dict(h=h, wq=wq, wo=wo, bo=bo, gamma=gamma, beta=beta, k=k, vt=vt, ldt=ldt, kip=kip, vtip=vtip, ldi=ldi, L=L, scale=scale, ref=ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [4, 16])
@pytest.mark.parametrize("N", [128, 256])
def test_rc_xattn_per_item_scale(dtype, T, N, monkeypatch):
    """C 320; rows_per_batch 128 (one workgroup per item) and 256"""
    from theatergen_amd import ops, rowchain
    B = B3
    c = _rc_case(B, N, T, dtype, seed=7 * N + T)
    wqp = rowchain.pack_xattn_q(c["wq"], None, c["gamma"], c["beta"], c["scale"])
    wop = rowchain.pack_xattn_out(c["wo"], c["bo"])
    kv = ops.rc_kv_pack(c["k"], c["vt"], c["ldt"], c["L"], c["kip"], c["vtip"], c["ldi"], T, B)
    run = lambda w: ops.rc_xattn(c["h"], wqp, kv, wop, N, 1e-5, T, ip_scale=w)
    l2, mx = rc_tols(dtype)
    what = f"rc_xattn N{N} T{T} {dtype}"
    vec = torch.tensor(SCALES, device=DEV)
    got = run(vec)
    check(got, c["ref"](vec), what + " per item", l2, mx)
    for b, s in enumerate(SCALES):
        one = run(torch.full((1,), s, device=DEV))
        check(one, c["ref"](s), what + f" scalar {s}", l2, mx)
        assert torch.equal(got[b * N:(b + 1) * N], one[b * N:(b + 1) * N]), f"{what}: item {b} of the per-item launch differs from the scalar launch with {s}"
    assert not torch.equal(got[N:2 * N], run(torch.full((1,), SCALES[2], device=DEV))[N:2 * N])
    old = run(torch.full((1,), 0.4, device=DEV))
    for count in (0, 1):
        with monkeypatch.context() as mp:
            _through_new_entry(mp, "tg_rc_xattn", count)
            assert torch.equal(run(torch.full((1,), 0.4, device=DEV)), old), f"{what}: tg_rc_xattn_ps(count {count}) != tg_rc_xattn"
    with pytest.raises(RuntimeError, match="2 elements"):
        run(torch.zeros(2, device=DEV))


# ---- tg_xq_attn --------------------------------------------------------------------------------------------------------------------------------
def _xq_parts(x, gamma, beta, wq, k, v, kip, vip, heads, scale, f):
    """test_round5_gpu.py::_xq_reference (f = float) / test_xq_d64_gpu.py::_xq_reference64 (f = double) with the image segment returned apart"""
    M, C = x.shape
    B = k.shape[0]
    N = M // B
    d = C // heads
    q = (F.layer_norm(f(x), (C,), f(gamma), f(beta), 1e-5) @ f(wq).t()).reshape(B, N, heads, d).permute(0, 2, 1, 3)
    hd = lambda t: f(t).reshape(B, t.shape[1], heads, d).permute(0, 2, 1, 3)
    o_text = torch.softmax(q @ hd(k).transpose(-1, -2) * scale, -1) @ hd(v)
    o_img = torch.softmax(q @ hd(kip).transpose(-1, -2) * scale, -1) @ hd(vip)

    def ref(w):
        w = torch.as_tensor(w, device=x.device).to(o_text.dtype).reshape(-1, 1, 1, 1)
        return (o_text + w * o_img).permute(0, 2, 1, 3).reshape(M, C)
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,d", [(640, 80), (1280, 160), (640, 64)])
@pytest.mark.parametrize("N", [128, 256])
def test_xq_attn_per_item_scale(dtype, C, d, N, monkeypatch):
    """all three head-dim instances; rows_per_batch 128 (tile t belongs to item t) and 256"""
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_ln_linear
    B, L, T = B3, 77, 4
    heads, M = C // d, B3 * N
    g = torch.Generator().manual_seed(C + d + N)
    t = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x = (t(M, C, sc=1.2) + 0.2).to(dtype).to(DEV)
    wq = t(C, C, sc=C ** -0.5).to(dtype).to(DEV)
    gamma, beta = (1 + 0.2 * t(C)).to(dtype).to(DEV), t(C, sc=0.1).to(dtype).to(DEV)
    k, v = t(B, L, C).to(dtype).to(DEV), t(B, L, C).to(dtype).to(DEV)
    kip, vip = t(B, T, C).to(dtype).to(DEV), t(B, T, C).to(dtype).to(DEV)
    ldt, ldi = 80, 8
    vt = torch.zeros(B, C, ldt, device=DEV, dtype=dtype); vt[:, :, :L] = v.transpose(1, 2)
    vtip = torch.zeros(B, C, ldi, device=DEV, dtype=dtype); vtip[:, :, :T] = vip.transpose(1, 2)
    scale = d ** -0.5
    wl, u, vv = pack_ln_linear(wq, None, gamma, beta, scale=scale * math.log2(math.e))
    blob = ops.xq_kv_pack(k.reshape(B * L, C), vt, ldt, L, kip.reshape(B * T, C), vtip, ldi, T, B, C, d)
    run = lambda w: ops.xq_attn(x, wl, u, vv, 1e-5, blob, d, N, L, T, ip_scale=w)
    ref = _xq_parts(x, gamma, beta, wq, k, v, kip, vip, heads, scale, (lambda a: a.double()) if d == 64 else (lambda a: a.float()))
    l2, mx = xq_tols(dtype)
    what = f"xq_attn C{C} d{d} N{N} {dtype}"
    vec = torch.tensor(SCALES, device=DEV)
    got = run(vec)
    check(got, ref(vec), what + " per item", l2, mx)
    for b, s in enumerate(SCALES):
        one = run(torch.full((1,), s, device=DEV))
        check(one, ref(s), what + f" scalar {s}", l2, mx)
        assert torch.equal(got[b * N:(b + 1) * N], one[b * N:(b + 1) * N]), f"{what}: item {b} of the per-item launch differs from the scalar launch with {s}"
    assert not torch.equal(got[N:2 * N], run(torch.full((1,), SCALES[2], device=DEV))[N:2 * N])
    old = run(torch.full((1,), 0.4, device=DEV))
    for count in (0, 1):
        with monkeypatch.context() as mp:
            _through_new_entry(mp, "tg_xq_attn", count)
            assert torch.equal(run(torch.full((1,), 0.4, device=DEV)), old), f"{what}: tg_xq_attn_ps(count {count}) != tg_xq_attn"
    with pytest.raises(RuntimeError, match="2 elements"):
        run(torch.zeros(2, device=DEV))


# ---- IPAttnProcessor on its three routes ------------------------------------------------------------------------------------------------------
def _ip_attn(C, heads, ctx, T, dtype, seed):
    from theatergen_amd import attention_processor as AP
    torch.manual_seed(seed)
    attn = AP.Attention(query_dim=C, cross_attention_dim=ctx, heads=heads, dim_head=C // heads)
    attn.set_processor(AP.IPAttnProcessor(hidden_size=C, cross_attention_dim=ctx, scale=0.4, num_tokens=T))
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.add_(0.2 * torch.randn(C))
        norm.bias.add_(0.1 * torch.randn(C))
    return attn.to(DEV, dtype), norm.to(DEV, dtype)


# route, C, heads, N: the smallest shapes the selectors take as they stand — the row chain from 8192 rows of 320 channels (N a multiple of 128), the fused
# to_q + attention launch from 4096 rows (head dim 80), the three launches below that
ROUTES = [("rc_xattn", 320, 8, 2816), ("xq_attn", 640, 8, 1408), ("attention", 640, 8, 128)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,C,heads,N", ROUTES)
def test_processor_routes_take_the_vector(dtype, route, C, heads, N, monkeypatch):
    from theatergen_amd import attention_processor as AP
    B, T, ctx = B3, 4, 64
    attn, norm = _ip_attn(C, heads, ctx, T, dtype, seed=C + N)
    proc = attn.processor
    g = torch.Generator().manual_seed(N)
    x = (torch.randn(B, N, C, generator=g) * 1.1 + 0.2).to(DEV, dtype)
    enc = (torch.randn(B, 77 + T, ctx, generator=g) * 0.5).to(DEV, dtype)
    calls = _spy(monkeypatch, ["rc_xattn", "xq_attn", "attention"])

    def call():
        if route == "rc_xattn":                                        # what BasicTransformerBlock.run does on the first level
            out = AP.fused_cross_block(attn, norm, x.reshape(B * N, C), B, N, enc, {})
            assert out is not None, "the row chain refused the shape"
            return out.reshape(B, N, C)
        return proc(attn, x, encoder_hidden_states=enc, _fused_residual=x.reshape(B * N, C), _fused_ln=(norm, None))
    proc.scale = SCALES
    assert proc.scale == tuple(SCALES)
    got = call()
    assert {k: v for k, v in calls.items() if v} == {route: [B]}, f"{route}: launches {calls}"
    for b, s in enumerate(SCALES):
        proc.scale = s
        assert proc.scale == s
        one = call()
        assert torch.equal(got[b], one[b]), f"{route} {dtype}: item {b} with the vector differs from the call with the number {s}"
    assert not torch.equal(got[1], one[1])
    assert calls[route] == [B] * (1 + B), f"a number after a vector fills the [B] buffer and keeps the per-item launch: {calls}"
    # a fresh processor in the number form launches with one float
    attn2, norm2 = _ip_attn(C, heads, ctx, T, dtype, seed=C + N)
    attn, norm, proc = attn2, norm2, attn2.processor
    proc.scale = SCALES[2]
    assert torch.equal(call(), one) and calls[route][-1] == 1
    # a vector of another length than the batch
    proc.scale = [0.1, 0.2]
    with pytest.raises(ValueError, match=r"2 per-batch-item values.*batch 3"):
        call()


def test_processor_host_constant_paths_refuse_a_vector():
    from theatergen_amd import backward
    B, T, ctx, C, N = 2, 4, 64, 320, 64
    attn, norm = _ip_attn(C, 8, ctx, T, torch.bfloat16, seed=5)
    proc = attn.processor
    x = torch.randn(B, N, C).to(DEV, torch.bfloat16)
    enc = torch.randn(B, 77 + T, ctx).to(DEV, torch.bfloat16)
    proc.scale = [0.9, 0.1]
    with pytest.raises(NotImplementedError, match="capture"):
        proc(attn, x, encoder_hidden_states=enc, save_attn_to_dict={}, attn_key=("down", 0, 0, 0))
    with pytest.raises(NotImplementedError, match="capture"):
        proc(attn, x, encoder_hidden_states=enc, return_attntion_probs=True)
    with pytest.raises(NotImplementedError, match="reverse pass"):
        backward.attention_input_grad(attn, proc, x.reshape(B * N, C), B, N, enc, torch.ones(B * N, C, device=DEV, dtype=torch.bfloat16), None)
    proc.scale = 0.9                                                   # a number again: both paths run
    out, probs = proc(attn, x, encoder_hidden_states=enc, return_attntion_probs=True)
    assert out.shape == (B, N, C) and probs.shape[-1] == 77
    assert backward.attention_input_grad(attn, proc, x.reshape(B * N, C), B, N, enc, torch.ones(B * N, C, device=DEV, dtype=torch.bfloat16), None) is not None


# ---- engine -------------------------------------------------------------------------------------------------------------------------------------
def _build(cfg, dtype, seed=0, T=4, scale=0.4):
    """test_hotpath_gpu.py::_build"""
    from theatergen_amd import weights as W
    from theatergen_amd.unet import UNet2DConditionModel
    sd = W.random_unet_state_dict(cfg, seed=seed)
    sd_r = {k: v.to(dtype).float() for k, v in sd.items()}             # the oracle sees the SAME (storage-rounded) weights as the device
    unet = UNet2DConditionModel.from_state_dict(cfg, sd, device=DEV, dtype=dtype, num_tokens=T, ip_scale=scale)
    return unet, sd_r


def test_engine_per_image_scale_tiny_plan():
    """tiny plan, n_img 2, 3 steps, scales [0, 0.4]: image i of the per-image run IS image i of the same engine run at the number scales[i]; each image
    also against the oracle loop run for it alone at batch 1; graph == eager; new values replay the same graph; number -> vector re-captures once"""
    from oracle import ddim as oddim
    from oracle import unet as ou
    from theatergen_amd import config
    from theatergen_amd.pipelines import DenoiseEngine
    dtype = torch.bfloat16
    cfg = config.tiny()
    unet, sd_r = _build(cfg, dtype)
    g = torch.Generator().manual_seed(8)
    n, steps, scales = 2, 3, [0.0, 0.4]
    lat = torch.randn(n, 4, 16, 16, generator=g)
    enc = torch.randn(2 * n, 81, cfg.cross_attention_dim, generator=g) * 0.5
    mk = lambda use_graph=True: DenoiseEngine(unet, None, n_img=n, height=128, width=128, num_inference_steps=steps, guidance_scale=7.5, enc_len=81,
                                              use_graph=use_graph)
    eng = mk()
    captures = []
    orig_capture = eng._capture
    eng._capture = lambda: (captures.append(1), orig_capture())[1]
    eng.set_conditioning(enc.to(DEV, dtype))
    # number form first (what every caller does today), then the vector: one re-capture, and the right result
    by_number = {}
    for s in scales:
        eng.set_ip_scale(s)
        by_number[s] = eng.run(lat).clone()
    assert len(captures) == 1, "changing the number must replay the captured step"
    graph_number = eng.graph
    eng.set_ip_scale(scales)
    hv = eng.run(lat).clone()
    assert len(captures) == 2 and eng.graph is not graph_number, "number form -> per-image form re-captures the step exactly once"
    assert not torch.equal(by_number[0.0][-1], by_number[0.4][-1])
    for i, s in enumerate(scales):
        assert torch.equal(hv[:, i], by_number[s][:, i]), f"image {i} of the per-image run differs from the run at the number {s}"
    # new VALUES replay the same CUDAGraph object
    graph_vec = eng.graph
    eng.set_ip_scale(scales[::-1])
    hr = eng.run(lat).clone()
    assert eng.graph is graph_vec and len(captures) == 2
    for i, s in enumerate(scales[::-1]):
        assert torch.equal(hr[:, i], by_number[s][:, i])
    # the per-step gating assigns plain numbers: on an engine in per-image form it replays the same graph and gives the number's result
    eng.set_ip_scale(scales)
    gated = eng.run(lat, before_step=lambda i: [setattr(p, "scale", 0.4) for p in eng._ip_processors()]).clone()
    assert eng.graph is graph_vec and len(captures) == 2 and torch.equal(gated, by_number[0.4])
    # eager engine == graph engine
    eng_e = mk(False)
    eng_e.set_conditioning(enc.to(DEV, dtype))
    eng_e.set_ip_scale(scales)
    assert torch.equal(eng_e.run(lat), hv), "graph replay is not bit-identical to eager launches in the per-image form"
    # the oracle loop, per image at batch 1 with its own number
    osch = oddim.DDIMSchedule()
    osch.set_timesteps(steps)
    for i, s in enumerate(scales):
        ref = lat[i:i + 1].clone()
        enc_i = enc[[i, n + i]].to(dtype).float()
        for t in osch.timesteps.tolist():
            npred = ou.unet_forward(cfg, sd_r, torch.cat([ref] * 2).to(dtype).float(), t, enc_i, ip_scale=s)
            ref = oddim.step_epilogue(osch, npred, t, ref, 7.5)
        close(hv[-1, i:i + 1], ref, net_tol(dtype), f"per-image engine, image {i} (scale {s}) vs its own oracle loop")
    with pytest.raises(ValueError, match="n_img = 2"):
        eng.set_ip_scale([0.1, 0.2, 0.3])


def test_vector_scale_assignment_is_fenced_against_engine_streams():
    """test_round5_gpu.py::test_ip_scale_assignment_is_fenced_against_engine_streams with VECTOR writes: per-image scales gated between the rounds of
    ``run_concurrent`` (two engines on their own streams, one UNet) give the bits of the same gating on a single stream"""
    from theatergen_amd import config
    from theatergen_amd.attention_processor import IPAttnProcessor
    from theatergen_amd.pipelines import DenoiseEngine
    dtype = torch.bfloat16
    cfg = config.tiny()
    unet, _ = _build(cfg, dtype)
    procs = [p for p in unet.attn_processors.values() if isinstance(p, IPAttnProcessor)]
    assert procs
    g = torch.Generator().manual_seed(41)
    steps = 6
    lats = [torch.randn(2, 4, 16, 16, generator=g) for _ in range(2)]
    encs = [torch.randn(4, 81, cfg.cross_attention_dim, generator=g) * 0.5 for _ in range(2)]
    engs = [DenoiseEngine(unet, None, n_img=2, height=128, width=128, num_inference_steps=steps, guidance_scale=7.5, enc_len=81) for _ in range(2)]
    for e, enc in zip(engs, encs):
        e.set_conditioning(enc.to(DEV, dtype))

    def gate(i):
        v = [0.0, 0.0] if (i / steps < 1 / 3 or (i + 1) / steps > 2 / 3) else [0.7, 0.2]
        for p in procs:
            p.scale = v + v
    engs[0].set_ip_scale([0.7, 0.2])
    seq = [e.run(lat, before_step=gate).clone() for e, lat in zip(engs, lats)]
    engs[0].set_ip_scale([0.7, 0.2])
    ungated = [e.run(lat).clone() for e, lat in zip(engs, lats)]
    assert not torch.equal(seq[0][-1], ungated[0][-1]), "the gating must change the result for the test to mean anything"
    for rep in range(3):
        par = [h.clone() for h in DenoiseEngine.run_concurrent(engs, lats, before_step=gate)]
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(seq[k], par[k]), f"gated concurrent replay differs from the gated single-stream run (engine {k}, repeat {rep})"


def test_engine_form_change_between_capture_and_replay():
    """a vector of another form or length assigned AFTER the capture, by a before_step hook or between two runs: the right result or a loud refusal,
    never a replay that reads a buffer the new values were not written to"""
    from theatergen_amd import config
    from theatergen_amd.attention_processor import IPAttnProcessor
    from theatergen_amd.pipelines import DenoiseEngine
    dtype = torch.bfloat16
    cfg = config.tiny()
    unet, _ = _build(cfg, dtype)
    procs = [p for p in unet.attn_processors.values() if isinstance(p, IPAttnProcessor)]
    g = torch.Generator().manual_seed(8)
    n, steps = 2, 3
    lat = torch.randn(n, 4, 16, 16, generator=g)
    enc = torch.randn(2 * n, 81, cfg.cross_attention_dim, generator=g) * 0.5
    eng = DenoiseEngine(unet, None, n_img=n, height=128, width=128, num_inference_steps=steps, guidance_scale=7.5, enc_len=81)
    eng.set_conditioning(enc.to(DEV, dtype))
    by_number = {}
    for s in (0.0, 0.4):
        eng.set_ip_scale(s)
        by_number[s] = eng.run(lat).clone()
    one = procs[0].scale_device(torch.device(DEV), 2 * n)
    assert one.numel() == 1

    def assign(v):
        for p in procs:
            p.scale = v
    # (1) a hook turns a step captured with a number into the per-image form: refused before the replay of that step
    with pytest.raises(RuntimeError, match="before_step hook changed"):
        eng.run(lat, before_step=lambda i: assign([0.0, 0.4, 0.0, 0.4]) if i == 1 else None)
    torch.cuda.synchronize()
    # (2) the same assignment BETWEEN two runs: one re-capture, the right images; the [1] buffer the first graph read is still there (poisoned, not freed)
    assert procs[0].scale_device(torch.device(DEV)) is not one and one.data_ptr() == procs[0]._scale_bufs[(torch.device(DEV), 1)].data_ptr()
    assert torch.isnan(one).all()
    hv = eng.run(lat).clone()
    for i, s in enumerate((0.0, 0.4)):
        assert torch.equal(hv[:, i], by_number[s][:, i])
    four = procs[0].scale_device(torch.device(DEV), 2 * n)
    graph_vec = eng.graph
    # (3) a hook assigns a vector of another length on the per-image engine: refused
    with pytest.raises((RuntimeError, ValueError), match="per-batch-item scales|before_step hook changed"):
        eng.run(lat, before_step=lambda i: assign([0.1] * 6) if i == 1 else None)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="6 per-batch-item scales"):
        eng.run(lat)                                                   # ... and so is a run that starts with it
    # (4) back to this engine's form: the same graph, the same buffer, the right images
    eng.set_ip_scale([0.4, 0.0])
    hr = eng.run(lat).clone()
    assert eng.graph is graph_vec and procs[0].scale_device(torch.device(DEV), 2 * n) is four
    for i, s in enumerate((0.4, 0.0)):
        assert torch.equal(hr[:, i], by_number[s][:, i])
    # (5) a hook that assigns VALUES of the captured form is what hooks are for
    gated = eng.run(lat, before_step=lambda i: assign([0.0, 0.4, 0.0, 0.4])).clone()
    assert torch.equal(gated, hv) and eng.graph is graph_vec


def test_graphed_input_grad_refuses_a_changed_scale_form():
    """the other owner of a captured graph: ``GraphedInputGrad`` bakes in the [1] buffer of every IP processor.  Per-batch-item values assigned after the
    capture: ``run`` refuses; ``latent_backward_guidance(graphed=True)`` does not hit its cache (and the re-capture refuses the vector); a number again:
    the old graph replays the bits it gave before — its buffer was never freed"""
    from tests.golden import gen_common as gc
    from theatergen_amd import config
    from theatergen_amd import guidance as G
    from theatergen_amd.attention_processor import IPAttnProcessor
    from theatergen_amd.backward import GraphedInputGrad, latent_backward_guidance
    from theatergen_amd.scheduler import DDIMScheduler
    dtype = torch.bfloat16
    cfg = config.tiny()
    unet, _ = _build(cfg, dtype)
    procs = [p for p in unet.attn_processors.values() if isinstance(p, IPAttnProcessor)]
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(1, 4, 32, 32, generator=g).to(DEV, dtype)
    enc = (torch.randn(1, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    keys = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
    boxes, pos = gc.GUIDANCE_BOXES[2], gc.GUIDANCE_POSITIONS[2]
    t = 741

    def loss_fn(sv):
        return G.compute_ca_lossv3(sv, boxes, pos, keys, return_grads=True, loss_scale=30.0, use_ratio_based_loss=True)
    gig = GraphedInputGrad(unet, lat, t, enc, loss_fn, keys, streams=3)
    loss0, grad0 = gig.run()
    torch.cuda.synchronize()
    loss0, grad0 = loss0.clone(), grad0.clone()
    assert torch.isfinite(grad0).all() and grad0.abs().max() > 0
    for p in procs:
        p.scale = [0.4, 0.0]                                           # e.g. a batched stage-1 run of two characters on the same UNet
    with pytest.raises(RuntimeError, match="form of an IPAttnProcessor.scale changed"):
        gig.run()
    sch = DDIMScheduler()
    sch.set_timesteps(50)
    kw = dict(loss_scale=30.0, loss_threshold=0.0, max_iter=1, guidance_attn_keys=keys, graphed=True, use_ratio_based_loss=True)
    for p in procs:
        p.scale = 0.4
    lat1, _ = latent_backward_guidance(None, sch, unet, enc, 0, boxes, pos, t, lat, 1e6, **kw)
    cached = next(iter(unet.__dict__["_graphed_input_grad"].values()))
    for p in procs:
        p.scale = [0.4, 0.0]
    with pytest.raises(NotImplementedError):                           # no cache hit: the re-capture meets the vector and says so
        latent_backward_guidance(None, sch, unet, enc, 0, boxes, pos, t, lat, 1e6, **kw)
    torch.cuda.synchronize()
    for p in procs:
        p.scale = 0.4                                                  # the number the graphs were captured with
    loss2, grad2 = gig.run()
    torch.cuda.synchronize()
    assert torch.equal(grad2, grad0) and loss2.item() == loss0.item(), "the first graph's [1] buffer must still be the processor's"
    lat2, _ = latent_backward_guidance(None, sch, unet, enc, 0, boxes, pos, t, lat, 1e6, **kw)
    assert torch.equal(lat1, lat2)
    unet.__dict__["_graphed_input_grad"].clear()
    assert cached is not None


# ---- the batched stage-1 function -------------------------------------------------------------------------------------------------------------
class _FakeTextPipe:
    """test_round6_gpu.py::_FakeTextPipe"""

    def __init__(self, unet, vae, ctx):
        from theatergen_amd.scheduler import DDIMScheduler
        self.unet, self.vae, self.ctx = unet, vae, ctx
        self.scheduler = DDIMScheduler()
        self.vae_scale_factor = 8
        self.controlnet = None
        self.prompts = []

    def encode_prompt(self, prompt, device=None, num_images_per_prompt=1, do_classifier_free_guidance=True, negative_prompt=None, **kw):
        self.prompts.append((prompt, negative_prompt))

        def emb(s):
            g = torch.Generator().manual_seed(sum(map(ord, s)) % 100003)
            return (torch.randn(1, 77, self.ctx, generator=g) * 0.5).to(device=self.unet.device, dtype=self.unet.dtype)
        return emb(prompt), emb(negative_prompt)


def _image_tokens_of(pil_image, ctx, dev, dtype):
    """test_round6_gpu.py::_image_tokens_of: tokens seeded by the image's pixels (cond) / fixed (uncond)"""
    seed = int(np.asarray(pil_image.convert("RGB").resize((8, 8))).astype(np.int64).sum() % 100003)
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, 4, ctx, generator=g) * 0.5).to(dev, dtype), (torch.randn(1, 4, ctx, generator=torch.Generator().manual_seed(5)) * 0.5).to(dev, dtype)


def _build_vae(cfg, dtype, seed=2):
    """test_hotpath_gpu.py::_build_vae"""
    from theatergen_amd import weights as W
    from theatergen_amd.vae import AutoencoderKL
    sd = W.random_vae_decoder_state_dict(cfg, seed=seed)
    sd_r = {k: v.to(dtype).float() for k, v in sd.items()}
    sd_r["post_quant_conv.weight"], sd_r["post_quant_conv.bias"] = sd["post_quant_conv.weight"], sd["post_quant_conv.bias"]  # fp32 on device too
    return AutoencoderKL.from_state_dict(cfg, sd, device=DEV, dtype=dtype), sd_r


def test_generate_characters_two_characters_one_run(tmp_path, monkeypatch):
    """one character with a database PNG (scale 0.4) and one first appearance (placeholder, scale 0) in ONE engine run: per character the latents of
    the oracle loop run for it alone; the PNG is written for the new character only"""
    from PIL import Image
    from oracle import ddim as oddim
    from oracle import unet as ou
    from theatergen_amd import config, pipelines
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.vae import tiny_vae_config
    dtype = torch.bfloat16
    cfg = config.tiny()
    unet, sd_r = _build(cfg, dtype)
    vae, _ = _build_vae(tiny_vae_config(), dtype)
    pipe = _FakeTextPipe(unet, vae, cfg.cross_attention_dim)
    ad = IPAdapter(pipe, None, None, DEV, num_tokens=4)
    monkeypatch.setattr(ad, "get_image_embeds", lambda pil_image=None, clip_image_embeds=None: _image_tokens_of(pil_image, cfg.cross_attention_dim, DEV, dtype))
    monkeypatch.chdir(tmp_path)
    Image.fromarray(np.full((32, 32, 3), 90, np.uint8)).save("model.png")
    db = str(tmp_path) + "/db_"
    Image.fromarray(np.random.default_rng(3).integers(0, 255, (32, 32, 3), dtype=np.uint8)).save(db + "7.png")
    before = open(db + "7.png", "rb").read()
    g = torch.Generator().manual_seed(31)
    steps = 4
    lat = torch.randn(2, 4, 16, 16, generator=g).to(dtype)
    runs = []
    orig_run = pipelines.DenoiseEngine.run
    monkeypatch.setattr(pipelines.DenoiseEngine, "run", lambda self, *a, **k: (runs.append(self.n_img), orig_run(self, *a, **k))[1])
    vectors = []
    orig_set = pipelines.DenoiseEngine.set_ip_scale
    monkeypatch.setattr(pipelines.DenoiseEngine, "set_ip_scale", lambda self, sc: (vectors.append(list(sc)), orig_set(self, sc))[1])
    captures = []
    orig_cap = pipelines.DenoiseEngine._capture
    monkeypatch.setattr(pipelines.DenoiseEngine, "_capture", lambda self: (captures.append(1), orig_cap(self))[1])
    out = pipelines.generate_characters("story", [11, 12], "1.5", ["a red fox", "a blue owl"], db, ad, lat.to(DEV), steps, [7, 9], guidance_scale=7.5,
                                        save_all_latents=True)
    assert runs == [2], "one engine run for the whole list"
    assert [p[0] for p in pipe.prompts] == ["full-body picture of a red fox", "full-body picture of a blue owl"]
    assert len(out) == 2 and all(len(o) == 3 for o in out)
    assert os.path.exists(db + "9.png"), "the first image of a new character is written to the database"
    assert open(db + "7.png", "rb").read() == before, "a known character's reference image is left alone"
    procs = pipelines.DenoiseEngine._ip_processors(next(iter(ad._tg_engines.values())))
    assert vectors == [[0.4, 0]], f"one set_ip_scale with the list of scales: {vectors}"
    assert all(p.scale == 0 and not isinstance(p.scale, tuple) for p in procs), "a NUMBER is left behind (the last character's), as by the reference's loop"

    def enc_of(prompt, pil):
        pos, neg = pipe.encode_prompt(prompt, negative_prompt=pipelines.SINGLE_OBJECT_NEGATIVE_PROMPT)
        img, unc = _image_tokens_of(pil, cfg.cross_attention_dim, DEV, dtype)
        return torch.cat([torch.cat([neg, unc], 1), torch.cat([pos, img], 1)], 0)
    osch = oddim.DDIMSchedule()
    osch.set_timesteps(steps)
    cases = [("full-body picture of a red fox", Image.open(db + "7.png"), 0.4),
             ("full-body picture of a blue owl", Image.open("model.png"), 0.0)]
    for i, (prompt, pil, s) in enumerate(cases):
        enc = enc_of(prompt, pil).float().cpu()
        ref, rows = lat[i:i + 1].float().clone(), [lat[i:i + 1].float().clone()]
        for t in osch.timesteps.tolist():
            npred = ou.unet_forward(cfg, sd_r, torch.cat([ref] * 2).to(dtype).float(), t, enc, ip_scale=s)
            ref = oddim.step_epilogue(osch, npred, t, ref, 7.5)
            rows.append(ref.clone())
        latents, image, latents_all = out[i]
        assert latents.shape == (1, 4, 16, 16) and latents.dtype == dtype and image.size == (128, 128)
        assert latents_all.shape == (steps + 1, 1, 4, 16, 16) and latents_all.device.type == "cpu" and latents_all.dtype == dtype
        close(latents, ref, net_tol(dtype), f"generate_characters: character {i} (scale {s}) vs the oracle loop for it alone")
        close(latents_all, torch.stack(rows), net_tol(dtype), f"generate_characters: latents_all of character {i}")
    assert np.array_equal(np.asarray(Image.open(db + "9.png")), np.asarray(out[1][1])), "the saved PNG is the returned image of the new character"
    # the second call finds both PNGs: every character at 0.4, the same engine and graph
    out2 = pipelines.generate_characters("story", [11, 12], "1.5", ["a red fox", "a blue owl"], db, ad, lat.to(DEV), steps, [7, 9])
    assert runs == [2, 2] and len(out2[0]) == 2 and vectors[-1] == [0.4, 0.4] and all(p.scale == 0.4 for p in procs)
    assert captures == [1], "the second call replays the step captured by the first"
