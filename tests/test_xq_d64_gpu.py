"""GPU: the head-dim-64 instance of the fused to_q + cross-attention launch (tg_xq_attn on 128 x 128 tiles, two heads of 64 per tile; SD-2.1 / SDXL,
opt-in with TG_XQ_D64=1) — the kernel against an fp64 restatement of its contract, the two processors routed through it against the oracle, the
shapes that must stay on the three-launch path, and a captured call replayed with another IP scale."""
import math
import types

import pytest
import torch

from tests.golden import gen_common as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


def op_tol(dtype):
    """the per-op bar of test_round5_gpu.test_inner_level_cross_attention_fused_vs_reference_golden: max, with rel-L2 at half of it"""
    return 1.5e-2 if dtype == torch.bfloat16 else 4e-3


def close(got, ref, dtype, what):
    from tests import parity_metrics as pm
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, f"{what}: {got.shape} vs {ref.shape}"
    m = pm.metrics(got, ref)
    print(f"{what}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e}")
    return pm.check(got, ref, what, op_tol(dtype) / 2, op_tol(dtype))


def _count(monkeypatch, names):
    """wrap ``theatergen_amd.ops.<name>`` so that a test can assert which launches ran"""
    from theatergen_amd import ops
    calls = {n: 0 for n in names}
    for n in names:
        orig = getattr(ops, n)

        def wrapper(*a, _o=orig, _n=n, **k):
            calls[_n] += 1
            return _o(*a, **k)
        monkeypatch.setattr(ops, n, wrapper)
    return calls


def _xq_reference64(x, gamma, beta, wq, k, v, kip, vip, heads, scale, ip_w):
    """fp64 restatement of norm2 -> to_q -> (decoupled) cross-attention of ip_adapter/attention_processor.py:445-529 (O before to_out) on the
    storage-dtype operands the kernel reads: no rounding of its own, no element left out"""
    import torch.nn.functional as F
    M, C = x.shape
    B = k.shape[0]
    N = M // B
    d = C // heads
    f = lambda t: t.double()
    q = (F.layer_norm(f(x), (C,), f(gamma), f(beta), 1e-5) @ f(wq).t()).reshape(B, N, heads, d).permute(0, 2, 1, 3)
    hd = lambda t: f(t).reshape(B, t.shape[1], heads, d).permute(0, 2, 1, 3)
    o = torch.softmax(q @ hd(k).transpose(-1, -2) * scale, -1) @ hd(v)
    if kip is not None:
        o = o + ip_w * torch.softmax(q @ hd(kip).transpose(-1, -2) * scale, -1) @ hd(vip)
    return o.permute(0, 2, 1, 3).reshape(M, C)


# (C, B, N, L, T, ip_w)
KERNEL_CASES = [
    (256, 2, 128, 77, 4, 0.4),       # smallest: two tile columns, one row tile per batch item (the blob's batch and tile indexing)
    (256, 3, 256, 96, 16, 1.0),      # every key slot live, odd batch
    (256, 2, 128, 8, 0, 0.0),        # two text key blocks fully masked, no image segment
    (640, 2, 256, 77, 16, 0.7),      # five tile columns (SDXL's width), three-stage instance
    (640, 8, 1024, 77, 4, 0.4),      # 320 tiles > 256: the two-stage instance
    (1280, 2, 128, 77, 4, 0.4),      # ten tile columns, K = 1280
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,B,N,L,T,ip_w", KERNEL_CASES)
def test_xq_attn_d64_vs_fp64_restatement(dtype, C, B, N, L, T, ip_w):
    """tg_xq_kv_pack + tg_xq_attn at head dim 64 against the fp64 restatement, with the bars of test_xq_attn_vs_fp32_reference (the same three
    storage-dtype roundings q, P, O; fewer terms per head); a second call gives the same bits; the IP scale is read from the device at run time."""
    from tests import parity_metrics as pm
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_ln_linear
    d = 64
    heads, M = C // d, B * N
    g = torch.Generator().manual_seed(C + B + N + L + T)
    t = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x = (t(M, C, sc=1.2) + 0.2).to(dtype).to(DEV)
    wq = t(C, C, sc=C ** -0.5).to(dtype).to(DEV)
    gamma, beta = (1 + 0.2 * t(C)).to(dtype).to(DEV), t(C, sc=0.1).to(dtype).to(DEV)
    k, v = t(B, L, C).to(dtype).to(DEV), t(B, L, C).to(dtype).to(DEV)
    kip, vip = (t(B, T, C).to(dtype).to(DEV), t(B, T, C).to(dtype).to(DEV)) if T else (None, None)
    ldt, ldi = 8 * ((L + 7) // 8), 8 * ((max(T, 1) + 7) // 8)
    vt = torch.zeros(B, C, ldt, device=DEV, dtype=dtype); vt[:, :, :L] = v.transpose(1, 2)
    vtip = None
    if T:
        vtip = torch.zeros(B, C, ldi, device=DEV, dtype=dtype); vtip[:, :, :T] = vip.transpose(1, 2)
    scale = d ** -0.5
    wl, u, vv = pack_ln_linear(wq, None, gamma, beta, scale=scale * math.log2(math.e))
    blob = ops.xq_kv_pack(k.reshape(B * L, C), vt, ldt, L, kip.reshape(B * T, C) if T else None, vtip, ldi, T, B, C, d)
    assert blob.numel() == B * (C // 128) * 60 * 1024
    w = torch.full((1,), ip_w, device=DEV)
    got = ops.xq_attn(x, wl, u, vv, 1e-5, blob, d, N, L, T, ip_scale=w if T else None)
    ref = _xq_reference64(x, gamma, beta, wq, k, v, kip, vip, heads, scale, ip_w)
    l2, mx = (4e-3, 1.2e-2) if dtype == torch.bfloat16 else (6e-4, 3e-3)
    what = f"xq_attn d64 C{C} B{B} N{N} L{L} T{T} w{ip_w} {dtype}"
    m = pm.metrics(got, ref)
    print(f"{what}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e}")
    pm.check(got, ref, what, l2, mx)
    assert torch.equal(got, ops.xq_attn(x, wl, u, vv, 1e-5, blob, d, N, L, T, ip_scale=w if T else None))
    if T:
        w.fill_(0.0)                                       # the same launch with another device-side scale (graph-replay contract)
        got0 = ops.xq_attn(x, wl, u, vv, 1e-5, blob, d, N, L, T, ip_scale=w)
        pm.check(got0, _xq_reference64(x, gamma, beta, wq, k, v, kip, vip, heads, scale, 0.0), what + " scale 0", l2, mx)


def _setup(C, heads, ctx, N, T, dtype, seed, ip=True, scale=0.6, B=2):
    """-> (attn on the device, norm on the device, x, enc on the device, fp32 CPU reference of the sub-block: the oracle's processor on torch's
    LayerNorm output)"""
    import torch.nn.functional as F
    from oracle import attention as oattn
    from theatergen_amd import attention_processor as AP
    g = torch.Generator().manual_seed(seed)
    w = gc.attn_weights(C, ctx, seed=seed + 1, with_ip=ip)
    nw, nb = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    x = torch.randn(B, N, C, generator=g) * 1.2 + 0.3
    enc = torch.randn(B, 77 + T, ctx, generator=g) * 0.5
    attn = AP.Attention(query_dim=C, cross_attention_dim=ctx, heads=heads, dim_head=C // heads)
    attn.load_state_dict({k: v for k, v in w.items() if "_ip" not in k})
    if ip:
        proc = AP.IPAttnProcessor(hidden_size=C, cross_attention_dim=ctx, scale=scale, num_tokens=T)
        proc.load_state_dict({"to_k_ip.weight": w["to_k_ip.weight"], "to_v_ip.weight": w["to_v_ip.weight"]})
        attn.set_processor(proc)
    attn = attn.to(DEV, dtype)
    norm = torch.nn.LayerNorm(C)
    norm.load_state_dict({"weight": nw, "bias": nb})
    xn = F.layer_norm(x, (C,), nw, nb, 1e-5)

    def ref(s=scale):
        return oattn.ip_attn_processor(w, heads, xn, enc, s, T) if ip else oattn.attn_processor(w, heads, xn, enc)
    return attn, norm.to(DEV, dtype), x.to(DEV, dtype), enc.to(DEV, dtype), ref


def _flag(monkeypatch, on=True):
    from theatergen_amd import attention_processor as AP
    monkeypatch.setattr(AP, "XQ_ENABLED", True)
    monkeypatch.setattr(AP, "XQ_D64_ENABLED", on)
    monkeypatch.setattr(AP, "XQ_D64_MIN_ROWS", 128)
    return AP


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,ctx,T", [(640, 10, 2048, 16), (1280, 20, 1024, 4)])
def test_ip_processor_routes_head_dim_64_through_the_fused_launch(dtype, C, heads, ctx, T, monkeypatch):
    """IPAttnProcessor called the way BasicTransformerBlock calls it (LayerNorm handed over for folding): one fused launch and no attention launch
    with the flag on, the three-launch path with it off; both against ONE oracle value."""
    AP = _flag(monkeypatch)
    attn, norm, x, enc, ref = _setup(C, heads, ctx, 256, T, dtype, seed=6400 + C + T)
    want = ref()
    calls = _count(monkeypatch, ["xq_attn", "attention"])
    got = attn.processor(attn, x, encoder_hidden_states=enc, _fused_ln=(norm, None))
    assert calls == {"xq_attn": 1, "attention": 0}, calls
    close(got, want, dtype, f"fused d64 IP cross-attention C{C} T{T} {dtype}")
    monkeypatch.setattr(AP, "XQ_D64_ENABLED", False)
    old = attn.processor(attn, x, encoder_hidden_states=enc, _fused_ln=(norm, None))
    assert calls == {"xq_attn": 1, "attention": 1}, calls
    close(old, want, dtype, f"three-launch d64 IP cross-attention C{C} T{T} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_processor_routes_head_dim_64_through_the_fused_launch(dtype, monkeypatch):
    """AttnProcessor, text-only cross-attention (T = 0), C = 640 = 10 heads x 64"""
    AP = _flag(monkeypatch)
    attn, norm, x, enc, ref = _setup(640, 10, 1024, 256, 0, dtype, seed=6464, ip=False)
    want = ref()
    calls = _count(monkeypatch, ["xq_attn", "attention"])
    got = attn.processor(attn, x, encoder_hidden_states=enc, _fused_ln=(norm, None))
    assert calls == {"xq_attn": 1, "attention": 0}, calls
    close(got, want, dtype, f"fused d64 text cross-attention {dtype}")
    monkeypatch.setattr(AP, "XQ_D64_ENABLED", False)
    old = attn.processor(attn, x, encoder_hidden_states=enc, _fused_ln=(norm, None))
    assert calls == {"xq_attn": 1, "attention": 1}, calls
    close(old, want, dtype, f"three-launch d64 text cross-attention {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,N", [(320, 5, 256), (640, 10, 192)])
def test_shapes_outside_the_tile_grid_stay_on_three_launches(dtype, C, heads, N, monkeypatch):
    """flag on: C = 320 (2.5 tile columns) and N = 192 (1.5 row tiles per batch item) keep the three-launch path and still match the oracle"""
    _flag(monkeypatch)
    attn, norm, x, enc, ref = _setup(C, heads, 1024, N, 4, dtype, seed=3200 + C + N)
    calls = _count(monkeypatch, ["xq_attn", "attention"])
    got = attn.processor(attn, x, encoder_hidden_states=enc, _fused_ln=(norm, None))
    assert calls == {"xq_attn": 0, "attention": 1}, calls
    close(got, ref(), dtype, f"three-launch d64 fallback C{C} N{N} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_captured_call_replays_with_the_scale_of_the_moment(dtype, monkeypatch):
    """one processor call through the fused launch captured in a graph; IPAdapter.set_scale between two replays: each replay gives the eager
    result of its scale (the kernel reads the scale from the device)"""
    from theatergen_amd.ip_adapter import IPAdapter
    _flag(monkeypatch)
    attn, norm, x, enc, _ = _setup(640, 10, 2048, 256, 16, dtype, seed=6416, scale=0.6)
    proc = attn.processor
    adapter = types.SimpleNamespace(pipe=types.SimpleNamespace(unet=types.SimpleNamespace(attn_processors={"attn2": proc})))
    calls = _count(monkeypatch, ["xq_attn", "attention"])
    call = lambda: proc(attn, x, encoder_hidden_states=enc, _fused_ln=(norm, None))
    eager = {}
    for s in (0.6, 0.15):
        IPAdapter.set_scale(adapter, s)
        eager[s] = call().clone()
    assert calls == {"xq_attn": 2, "attention": 0}, calls
    assert not torch.equal(eager[0.6], eager[0.15])
    IPAdapter.set_scale(adapter, 0.6)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    assert calls == {"xq_attn": 3, "attention": 0}, calls
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0.6])
    IPAdapter.set_scale(adapter, 0.15)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0.15])
