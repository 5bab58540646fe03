"""GPU: SAM's rel-pos attention (``tg_relpos_tables`` + ``tg_attention_relpos``) against fp64, and the encoder (``theatergen_amd/sam.py``) against
``transformers.SamVisionEncoder`` goldens (tests/golden/make_sam_golden.py).

Bounds, none taken from the code under test:
  * tables: |err| <= 2^-20 * sum_c |q_c r_c| per element (fp32 accumulation of exact products, the bound of the DPM sampler test);
  * attention: ``op_tol`` of tests/test_hotpath_gpu.py (the project's bound for tg_attention) AND rel-L2 <= 2 x the error of the parent's route on the
    same inputs — ``ops.attention(mask = the materialised fp32 [B, H, N, N] bias)`` — which rounds at the same two places;
  * encoder: ``close`` at 3e-2 bf16 / 6e-3 fp16 on the hidden state after the windowed layer, after the global layer, and on the neck output.
The fp64 references are computed once per (case, dtype) on the CPU with at most 16 threads.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import parity_metrics as pm
from tests.golden import make_sam_golden as G

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CASES = {"g64_b1_h2_d80": (64, 1, 2, 80), "g64_b2_h1_d64": (64, 2, 1, 64), "g14_b3_h2_d80": (14, 3, 2, 80), "g14_b2_h3_d64": (14, 2, 3, 64)}


def op_tol(dtype):
    return 1.5e-2 if dtype == torch.bfloat16 else 4e-3


def golden_tol(dtype):
    return 3e-2 if dtype == torch.bfloat16 else 6e-3


def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return float((got - ref).norm() / ref.norm())


def _record(rec):
    """TG_SAM_ERR_JSON=path: the measured errors go to that file too (scripts/sam_encoder_timing.py --errors turns them into the findings table)"""
    path = os.environ.get("TG_SAM_ERR_JSON")
    if path:
        import json
        recs = json.load(open(path)) if os.path.exists(path) else []
        with open(path, "w") as f:
            json.dump(recs + [rec], f, indent=1)


def _attn64(q, k, v, bias, scale):
    """fp64 softmax(scale q k^T + bias) v for [B, H, N, d] operands and a [B, H, N, N] bias."""
    s = scale * (q @ k.transpose(-1, -2)) + bias
    s -= s.amax(-1, keepdim=True)
    s.exp_()
    s /= s.sum(-1, keepdim=True)
    return s @ v


@functools.lru_cache(maxsize=None)
def case(cname, dname):
    """operands in the storage dtype (fused q | k rows, V^T per batch item, as the encoder lays them out) and the fp64 references"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    S, B, H, d = CASES[cname]
    dt = DTYPES[dname]
    N, D = S * S, H * d
    g = torch.Generator().manual_seed(1000 * S + 10 * d + B)
    qk = torch.randn(B * N, 2 * D, generator=g).to(dt)
    v = torch.randn(B, N, D, generator=g).to(dt)
    rph = (0.08 * torch.randn(2 * S - 1, d, generator=g)).to(dt)
    rpw = (0.08 * torch.randn(2 * S - 1, d, generator=g)).to(dt)
    q64 = qk[:, :D].double().reshape(B, N, H, d).permute(0, 2, 1, 3)                      # [B, H, N, d]
    k64 = qk[:, D:].double().reshape(B, N, H, d).permute(0, 2, 1, 3)
    v64 = v.double().reshape(B, N, H, d).permute(0, 2, 1, 3)
    idx = torch.arange(S)[:, None] - torch.arange(S)[None, :] + S - 1                      # [q coordinate, k coordinate]
    Rh, Rw = rph.double()[idx], rpw.double()[idx]                                          # [S, S, d]
    q5 = q64.reshape(B, H, S, S, d)
    bh = torch.einsum("bhyxc,ykc->bhyxk", q5, Rh).reshape(B, H, N, S)
    bw = torch.einsum("bhyxc,xkc->bhyxk", q5, Rw).reshape(B, H, N, S)
    mag_h = torch.einsum("bhyxc,ykc->bhyxk", q5.abs(), Rh.abs()).reshape(B, H, N, S)       # sum_c |q_c r_c|
    mag_w = torch.einsum("bhyxc,xkc->bhyxk", q5.abs(), Rw.abs()).reshape(B, H, N, S)
    bias = (bh[..., :, None] + bw[..., None, :]).reshape(B, H, N, N)                       # [.., kh, kw] -> key kh * S + kw
    scale = d ** -0.5
    ref = _attn64(q64, k64, v64, bias, scale)
    # what the reference would be with a table ignored or the key coordinates swapped (checked on the CPU before any launch)
    moved = {}
    for what, alt in (("Bh dropped", bw[..., None, :].expand(B, H, N, S, S)), ("Bw dropped", bh[..., :, None].expand(B, H, N, S, S)),
                      ("(kh, kw) transposed", bh[..., None, :] + bw[..., :, None])):
        moved[what] = rel_l2(_attn64(q64, k64, v64, alt.reshape(B, H, N, N), scale), ref)
    return dict(S=S, B=B, H=H, d=d, N=N, D=D, dt=dt, qk=qk, v=v, rph=rph, rpw=rpw, bh=bh, bw=bw, mag_h=mag_h, mag_w=mag_w, bias=bias,
                ref=ref.permute(0, 2, 1, 3).reshape(B * N, D), scale=scale, moved=moved)


def _device_operands(c):
    B, N, D = c["B"], c["N"], c["D"]
    ldt = (N + 7) // 8 * 8
    qk = c["qk"].cuda()
    vt = torch.full((B, D, ldt), float("nan"), dtype=c["dt"], device="cuda")               # columns >= N: never used as data
    vt[:, :, :N] = c["v"].cuda().transpose(1, 2)
    return qk, vt, ldt


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("cname", list(CASES))
def test_tables_against_fp64(cname, dname):
    from theatergen_amd import ops
    c = case(cname, dname)
    S, B, H, d, N, D = c["S"], c["B"], c["H"], c["d"], c["N"], c["D"]
    qk = c["qk"].cuda()
    bh = torch.full((B, H, N, S), float("nan"), device="cuda")
    bw = torch.full((B, H, N, S), float("nan"), device="cuda")
    ops.relpos_tables(qk, 2 * D, N * 2 * D, c["rph"].cuda(), c["rpw"].cuda(), B, H, d, S, out=(bh, bw))
    for name, got, ref, mag in (("Bh", bh, c["bh"], c["mag_h"]), ("Bw", bw, c["bw"], c["mag_w"])):
        got = got.double().cpu()
        assert torch.isfinite(got).all(), f"{name}: an element was not written"
        ratio = float(((got - ref).abs() / mag).max())
        print(f"relpos_tables {cname} {dname} {name}: max |err| / sum|q r| = {ratio:.3e} (bound 2^-20 = {2.0 ** -20:.3e})")
        assert ratio <= 2.0 ** -20


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("cname", list(CASES))
def test_attention_against_fp64_and_the_mask_route(cname, dname):
    from theatergen_amd import ops
    c = case(cname, dname)
    S, B, H, d, N, D, dt = c["S"], c["B"], c["H"], c["d"], c["N"], c["D"], c["dt"]
    tol = op_tol(dt)
    for what, mv in c["moved"].items():                                                    # CPU: the check can see a wrong table
        assert mv > 10 * tol / 2, f"{what} moves the fp64 reference by only {mv:.3e} rel-L2"
    qk, vt, ldt = _device_operands(c)
    bh32, bw32 = c["bh"].float().cuda().contiguous(), c["bw"].float().cuda().contiguous()
    out = torch.full((B * N, D), float("nan"), dtype=dt, device="cuda")
    ops.attention_relpos(qk, 2 * D, N * 2 * D, qk[:, D:], 2 * D, N * 2 * D, vt, ldt, D * ldt, B, H, d, S, c["scale"], bh32, bw32, out, D, N * D)
    mask = (bh32[..., :, None] + bw32[..., None, :]).reshape(B, H, N, N).contiguous()      # the parent's route: the bias as an [N, N] tensor
    vt0 = torch.nan_to_num(vt, nan=0.0)
    par = torch.empty((B * N, D), dtype=dt, device="cuda")
    ops.attention(qk, 2 * D, N * 2 * D, qk[:, D:], 2 * D, N * 2 * D, vt0, ldt, D * ldt, N, B, H, d, N, c["scale"], par, D, N * D, mask=mask)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), "an output element was not written"
    e_new, e_par = rel_l2(out, c["ref"]), rel_l2(par, c["ref"])
    m = pm.metrics(out, c["ref"])
    print(f"attention_relpos {cname} {dname}: rel-L2 {e_new:.3e} max {m['max_rel']:.3e} | mask route rel-L2 {e_par:.3e} | bound 2 x = {2 * e_par:.3e}, "
          f"op_tol {tol:.1e}; reference moves: {', '.join(f'{k} {v:.2f}' for k, v in c['moved'].items())}")
    _record(dict(kind="attention", case=f"{cname} {dname}", err_new=e_new, max_new=m["max_rel"], err_mask_route=e_par))
    pm.check(out, c["ref"], f"attention_relpos {cname} {dname}", tol / 2, tol)
    assert e_new <= 2 * e_par, f"rel-L2 {e_new:.3e} > 2 x the mask route's {e_par:.3e}"


def test_no_n_by_n_tensor_is_allocated():
    from theatergen_amd import ops
    S, H, d, dt = 64, 8, 80, torch.bfloat16
    N, D = S * S, H * d
    g = torch.Generator().manual_seed(5)
    qk = torch.randn(N, 2 * D, generator=g).to(dt).cuda()
    vt = torch.randn(1, D, N, generator=g).to(dt).cuda()
    rph, rpw = (0.08 * torch.randn(2, 2 * S - 1, d, generator=g)).to(dt).cuda()
    out = torch.empty((N, D), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    bh, bw = ops.relpos_tables(qk, 2 * D, N * 2 * D, rph.contiguous(), rpw.contiguous(), 1, H, d, S)
    ops.attention_relpos(qk, 2 * D, N * 2 * D, qk[:, D:], 2 * D, N * 2 * D, vt, N, D * N, 1, H, d, S, d ** -0.5, bh, bw, out, D, N * D)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak device memory across relpos_tables + attention_relpos at grid 64, 8 heads of 80: +{rise / 2 ** 20:.1f} MiB "
          f"(the [8, 4096, 4096] fp32 bias alone: 512 MiB)")
    _record(dict(kind="peak_memory", rise_mib=rise / 2 ** 20))
    assert torch.isfinite(out).all()
    assert rise < 512 * 2 ** 20


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden(tag):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"sam_vision_{tag}.npz"))
    v = G.VARIANTS[tag]
    w = G.make_weights(v["hidden"], v["seed"])
    assert np.allclose(G.weight_checksums(w), z["weight_checksums"], rtol=1e-12, atol=0), "make_weights no longer draws the golden's weights"
    return z, w, v


def _tiny_config(v):
    from theatergen_amd.sam import SamVisionConfig
    return SamVisionConfig(hidden_size=v["hidden"], num_hidden_layers=2, num_attention_heads=v["heads"], global_attn_indexes=[1],
                           mlp_dim=2 * v["hidden"], image_size=1024, patch_size=16, window_size=14, output_channels=32, layer_norm_eps=1e-6,
                           qkv_bias=True, use_abs_pos=True, use_rel_pos=True, num_channels=3)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("tag", ["d80", "d64"])
def test_encoder_against_the_transformers_golden(tag, dname):
    from theatergen_amd.sam import SamVisionEncoder
    z, w, v = golden(tag)
    dt = DTYPES[dname]
    enc = SamVisionEncoder.from_state_dict(_tiny_config(v), {k: torch.from_numpy(a) for k, a in w.items()}, device="cuda", dtype=dt)
    out, hs = enc(torch.from_numpy(G.golden_image()).cuda(), output_hidden_states=True)
    assert out.shape == (1, 32, 64, 64) and out.dtype == dt and len(hs) == 2
    rows = z["rows"].tolist()
    tol = golden_tol(dt)
    for name, got, ref in (("hidden0", hs[0][0, rows], z["hidden0"]), ("hidden1", hs[1][0, rows], z["hidden1"]), ("neck", out[0][:, rows], z["neck"])):
        m = pm.metrics(got.float().cpu(), torch.from_numpy(ref))
        print(f"sam encoder {tag} {dname} {name}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (tolerance {tol / 2:.1e} / {tol:.1e})")
    for name, got, ref in (("hidden0", hs[0][0, rows], z["hidden0"]), ("hidden1", hs[1][0, rows], z["hidden1"]), ("neck", out[0][:, rows], z["neck"])):
        pm.check(got.float().cpu(), torch.from_numpy(ref), f"sam encoder {tag} {dname} {name}", tol / 2, tol)


def test_state_dict_names():
    from theatergen_amd.sam import SamVisionEncoder
    _, w, v = golden("d64")
    sd = {k: torch.from_numpy(a) for k, a in w.items()}
    a = SamVisionEncoder.from_state_dict(_tiny_config(v), sd, device="cuda", dtype=torch.float16)
    full = {"vision_encoder." + k: t for k, t in sd.items()}
    full.update({"shared_image_embedding.positional_embedding": torch.zeros(2, 128), "mask_decoder.iou_token.weight": torch.zeros(1, 256),
                 "prompt_encoder.no_mask_embed.weight": torch.zeros(1, 256)})
    b = SamVisionEncoder.from_state_dict(_tiny_config(v), full, device="cuda", dtype=torch.float16)
    for (ka, pa), (kb, pb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb) and pa.is_cuda and pa.dtype == torch.float16
    assert set(a.state_dict()) == set(sd)
    missing = dict(sd)
    missing.pop("layers.0.attn.rel_pos_h")
    with pytest.raises(RuntimeError, match="rel_pos_h"):
        SamVisionEncoder.from_state_dict(_tiny_config(v), missing)
    extra = dict(sd)
    extra["layers.0.attn.rel_pos_d"] = torch.zeros(3)
    with pytest.raises(RuntimeError, match="rel_pos_d"):
        SamVisionEncoder.from_state_dict(_tiny_config(v), extra)
    with pytest.raises(RuntimeError, match="GPU only"):
        a(torch.zeros(1, 3, 1024, 1024))


def test_padded_window_layer_in_isolation():
    """One windowed layer on a 64 x 64 grid, d = 80, against an fp32 restatement (pad after layer_norm1, the padded tokens are real keys whose q, k, v
    are the projection bias).  Token (63, 63) sits in the corner window, 64 real positions and 132 padded ones: masking padded keys out would show there."""
    import torch.nn.functional as F
    from theatergen_amd.sam import SamVisionEncoder
    _, w, v = golden("d80")
    dt = torch.float16
    cfg = _tiny_config(v)
    enc = SamVisionEncoder.from_state_dict(cfg, {k: torch.from_numpy(a) for k, a in w.items()}, device="cuda", dtype=dt)
    D, H, S = 160, 2, 14
    d = D // H
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 64, D, generator=g).to(dt)
    got = enc.layers[0].run(x.reshape(4096, D).cuda(), 1, cfg, enc._window_maps(torch.device("cuda", torch.cuda.current_device())))
    p = {k[len("layers.0."):]: torch.from_numpy(a) for k, a in w.items() if k.startswith("layers.0.")}
    xf = x.float()
    y = F.layer_norm(xf, (D,), p["layer_norm1.weight"], p["layer_norm1.bias"], 1e-6)
    y = F.pad(y, (0, 0, 0, 6, 0, 6)).reshape(1, 5, S, 5, S, D).permute(0, 1, 3, 2, 4, 5).reshape(25, S * S, D)
    qkv = F.linear(y, p["attn.qkv.weight"], p["attn.qkv.bias"]).reshape(25, S * S, 3, H, d).permute(2, 0, 3, 1, 4)
    q, k, vv = qkv[0], qkv[1], qkv[2]                                                       # [25, H, 196, d]
    idx = torch.arange(S)[:, None] - torch.arange(S)[None, :] + S - 1
    q5 = q.reshape(25, H, S, S, d)
    bias = (torch.einsum("bhyxc,ykc->bhyxk", q5, p["attn.rel_pos_h"][idx])[..., :, None] +
            torch.einsum("bhyxc,xkc->bhyxk", q5, p["attn.rel_pos_w"][idx])[..., None, :]).reshape(25, H, S * S, S * S)
    o = torch.softmax(d ** -0.5 * (q @ k.transpose(-1, -2)) + bias, -1) @ vv
    o = o.permute(0, 2, 1, 3).reshape(1, 5, 5, S, S, D).permute(0, 1, 3, 2, 4, 5).reshape(1, 70, 70, D)[:, :64, :64]
    h = xf + F.linear(o, p["attn.proj.weight"], p["attn.proj.bias"])
    z = F.layer_norm(h, (D,), p["layer_norm2.weight"], p["layer_norm2.bias"], 1e-6)
    ref = h + F.linear(F.gelu(F.linear(z, p["mlp.lin1.weight"], p["mlp.lin1.bias"])), p["mlp.lin2.weight"], p["mlp.lin2.bias"])
    got = got.float().cpu().reshape(1, 64, 64, D)
    tol = golden_tol(dt)
    m = pm.check(got, ref, "sam windowed layer f16", tol / 2, tol)
    mc = pm.check(got[:, 56:, 56:], ref[:, 56:, 56:], "sam windowed layer f16, corner window", tol / 2, tol)
    print(f"windowed layer: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e}; corner window (64 real + 132 padded keys) rel-L2 {mc['rel_l2']:.3e}; "
          f"token (63, 63) |err| {float((got - ref)[0, 63, 63].abs().max()):.3e}")
    assert float((got - ref)[0, 63, 63].abs().max()) <= tol * float(ref.abs().max())
