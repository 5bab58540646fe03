"""GPU: the SDXL flow — the sigma step epilogue (tg_step_epilogue_sigma), the T2I-Adapter-XL kernels and forward, the UNet in T2I-Adapter mode,
and the 'xl' branches of the two stage functions, each against the fp32 restatements of tests/sdxl_flow_reference.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sdxl_flow_reference as R
from tests.test_kernels_gpu import DTYPES, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the step epilogue ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ancestral", [False, True])
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("fast", [False, True])
def test_step_epilogue_sigma_vs_restated_step(dtype, ancestral, frozen, fast):
    """CFG + Euler / Euler-ancestral update from the row the DEVICE counter selects, ancestral noise from the per-step table (storage dtype),
    frozen blend while step < frozen_steps, history rows, next model input x / sqrt(sigma_next^2 + 1) rounded once, counter advance"""
    from theatergen_amd import ops
    from theatergen_amd.schedule import get_fast_schedule
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    s = (EulerAncestralDiscreteScheduler if ancestral else EulerDiscreteScheduler)()
    s.set_timesteps(10)
    ts = get_fast_schedule(s.timesteps, 2, 2) if fast else s.timesteps
    n_steps = len(ts)
    coef = s.coef_table(ts).to(DEV)
    n, C, h, w = 2, 4, 8, 12
    g = torch.Generator().manual_seed(7 + ancestral + 2 * frozen + 4 * fast)
    lat = torch.randn(n, C, h, w, generator=g) * float(s.init_noise_sigma)
    noise = torch.randn(n_steps, n, C, h, w, generator=g).to(dtype)
    fz = torch.randn(n_steps + 1, n, C, h, w, generator=g)
    mask = (torch.rand(h, w, generator=g) > 0.5).float()
    frozen_steps = 2
    lat_d, idx = lat.to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    hist = torch.zeros(n_steps + 1, n, C, h, w, device=DEV)
    mi = torch.zeros(2 * n, C, h, w, dtype=dtype, device=DEV)
    ref = lat.clone()
    for i in range(3):
        npred = torch.randn(2 * n, C, h, w, generator=g)
        ops.step_epilogue_sigma(npred.to(DEV), lat_d, 7.5, coef, idx, noise=noise.to(DEV) if ancestral else None, frozen=fz.to(DEV) if frozen else None,
                                frozen_mask=mask.to(DEV) if frozen else None, frozen_steps=frozen_steps, history=hist, model_in=mi)
        u, c = npred.chunk(2)
        eps = u + 7.5 * (c - u)
        ref = R.euler_step(ref, eps, s.sigmas, i, ancestral, noise[i].float())          # step i: sigmas[i], sigmas[i + 1] of the FULL table
        if frozen and i < frozen_steps:
            ref = fz[i + 1] * mask + ref * (1 - mask)
        check(lat_d, ref, dtype, f"sigma epilogue step {i}")
        assert int(idx.item()) == i + 1, "the counter advances once per launch"
        same_hist = torch.equal(hist[i + 1], lat_d)
        want_mi = (lat_d / R.scale_div(s.sigmas, i + 1)).to(dtype)
        same_mi = torch.equal(mi[:n], want_mi) and torch.equal(mi[n:], want_mi)
        assert same_hist and same_mi, "history row + next model input (x / sqrt(sigma_next^2 + 1) as torch divides, one rounding, CFG-duplicated)"
    # Euler: the noise table and sigma_up are not read (no ancestral term)
    if not ancestral:
        lat2, idx2 = lat.to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        npred = torch.randn(2 * n, C, h, w, generator=g).to(DEV)
        ops.step_epilogue_sigma(npred, lat2, 7.5, coef, idx2, advance=False)
        lat3 = lat.to(DEV)
        ops.step_epilogue_sigma(npred, lat3, 7.5, coef, idx2, advance=False, noise=noise.to(DEV))
        assert int(idx2.item()) == 0 and torch.equal(lat2, lat3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scheduler_step_and_add_noise_drop_in(dtype):
    """``scheduler.step(noise_pred, t, latents, generator=g)`` / ``add_noise`` on the device vs the restatement; the ancestral step draws its noise
    from ``g`` like diffusers (same generator state -> same draw)"""
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 4, 16, 16, generator=g).to(dtype)
    eps = torch.randn(1, 4, 16, 16, generator=g).to(dtype)
    for cls, anc in ((EulerDiscreteScheduler, False), (EulerAncestralDiscreteScheduler, True)):
        s = cls()
        s.set_timesteps(20)
        gen = torch.Generator(DEV).manual_seed(9)
        out = s.step(eps.to(DEV), s.timesteps[3], x.to(DEV), generator=gen).prev_sample
        nz = torch.randn((1, 4, 16, 16), generator=torch.Generator(DEV).manual_seed(9), device=DEV, dtype=dtype).float().cpu()
        ref = R.euler_step(x.float(), eps.float(), s.sigmas, 3, anc, nz)
        assert out.dtype == dtype
        check(out, ref, dtype, f"{cls.__name__}.step")
        x0, nzz = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
        noisy = s.add_noise(x0.to(DEV, dtype), nzz.to(DEV, dtype), s.timesteps)
        want = x0.to(dtype).float()[None] + s.sigmas[:20].reshape(20, 1, 1, 1, 1) * nzz.to(dtype).float()[None]
        check(noisy.reshape(20, 1, 4, 16, 16), want, dtype, "add_noise")


# ---- T2I-Adapter kernels and forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 3, 1024, 1024, 16), (2, 3, 128, 96, 16), (2, 5, 12, 8, 2)])
def test_pixel_unshuffle_is_bit_exact(dtype, shape):
    from theatergen_amd import ops
    B, C, H, W, f = shape
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H + W)).to(dtype).to(DEV)
    got = ops.pixel_unshuffle(x, f)
    want = F.pixel_unshuffle(x, f).permute(0, 2, 3, 1).reshape(B * (H // f) * (W // f), C * f * f)
    same = torch.equal(got, want)
    assert same, "pixel-unshuffle only moves data"


@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_pool_and_scale_repeat_kernels(dtype):
    from theatergen_amd import ops
    g = torch.Generator().manual_seed(4)
    for (B, h, w, C) in [(2, 7, 5, 64), (1, 64, 64, 640)]:
        x = torch.randn(B * h * w, C, generator=g).to(dtype).to(DEV)
        same_relu = torch.equal(ops.relu(x), torch.clamp_min(x, 0))
        assert same_relu
        nchw = x.float().reshape(B, h, w, C).permute(0, 3, 1, 2)
        want = F.avg_pool2d(nchw, 2, 2, ceil_mode=True).permute(0, 2, 3, 1).reshape(-1, C)
        check(ops.avgpool2x2(x, B, h, w), want, dtype, f"avgpool2x2 ceil {h}x{w}")
        rep = ops.scale_repeat(x, 0.8, 2)
        same_rep = torch.equal(rep, torch.cat([x * 0.8] * 2))
        assert same_rep, "state * 0.8 then cat([state] * 2), rounded once like the reference's half-precision multiply"


def _build_t2i(channels, dtype, seed=5):
    from theatergen_amd import weights
    from theatergen_amd.t2i_adapter import T2IAdapter
    sd = weights.random_t2i_adapter_state_dict(seed=seed, channels=channels)
    sd_r = {k: v.to(dtype).float() for k, v in sd.items()}
    return T2IAdapter.from_state_dict(sd, device=DEV, dtype=dtype, channels=channels), sd_r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_t2i_adapter_xl_vs_restatement(dtype, size):
    """tiny: channels (64, 128, 256, 256) on a 128^2 image; full: the line-art adapter's (320, 640, 1280, 1280) on 1024^2, seeded random weights"""
    from tests.test_hotpath_gpu import close, net_tol
    channels, H = ((64, 128, 256, 256), 128) if size == "tiny" else ((320, 640, 1280, 1280), 1024)
    ad, sd_r = _build_t2i(channels, dtype)
    x = torch.rand(1, 3, H, H, generator=torch.Generator().manual_seed(H)).to(dtype)
    feats = ad(x.to(DEV))
    ref = R.t2i_adapter_forward(sd_r, x.float())
    shapes = [(1, channels[0], H // 16, H // 16), (1, channels[1], H // 16, H // 16), (1, channels[2], H // 32, H // 32), (1, channels[3], H // 32, H // 32)]
    assert [tuple(f.shape) for f in feats] == shapes and all(f.dtype == dtype for f in feats)
    for k, (f, r) in enumerate(zip(feats, ref)):
        close(f, r, net_tol(dtype), f"t2i adapter {size} feature {k}")
    tm = ad(x.to(DEV), token_major=True)
    for f, t in zip(feats, tm):
        same = torch.equal(f, t.t.reshape(t.b, t.h, t.w, t.c).permute(0, 3, 1, 2))
        assert same


# ---- the UNet in T2I-Adapter mode -------------------------------------------------------------------------------------------------------
def _feature_shapes(cfg, B, s):
    """the shape the adapter rules inject at: per down block (cross: its last pair's output; plain: after the block), then the mid block"""
    boc = cfg.block_out_channels
    shapes, h = [], s
    for i, bt in enumerate(cfg.down_block_types):
        if bt == "DownBlock2D" and i != len(boc) - 1:
            h = (h - 1) // 2 + 1
        shapes.append((B, boc[i], h, h))
        if bt != "DownBlock2D" and i != len(boc) - 1:
            h = (h - 1) // 2 + 1
    if len(shapes) < 4:
        shapes.append((B, boc[-1], h, h))
    return shapes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["xl", "sd15"])
def test_unet_adapter_mode_vs_restated_forward(dtype, variant):
    from tests.test_hotpath_gpu import _build, _tiny_inputs, close, net_tol
    from theatergen_amd import config
    from theatergen_amd.unet import _Act
    cfg = config.tiny(xl=True) if variant == "xl" else config.tiny()
    unet, sd_r = _build(cfg, dtype)
    x, enc, added = _tiny_inputs(cfg)
    shapes = _feature_shapes(cfg, 2, 16)
    g = torch.Generator().manual_seed(8)
    feats = [(torch.randn(s, generator=g) * 0.5).to(dtype) for s in shapes]
    addr = None if added is None else {k: v.to(dtype).float() if k == "text_embeds" else v for k, v in added.items()}
    addd = None if added is None else {k: v.to(DEV) for k, v in added.items()}
    ref = R.unet_forward_adapter(cfg, sd_r, x.to(dtype).float(), 981, enc.to(dtype).float(), [f.float() for f in feats], addr, ip_scale=0.4)
    fd = [f.to(DEV) for f in feats]
    out = unet(x.to(DEV, dtype), 981, enc.to(DEV, dtype), added_cond_kwargs=addd, down_block_additional_residuals=fd, out_dtype=torch.float32).sample
    close(out, ref, net_tol(dtype), f"unet adapter mode {variant}")
    assert [tuple(f.shape) for f in fd] == shapes, "the caller's list is not consumed"
    plain = unet(x.to(DEV, dtype), 981, enc.to(DEV, dtype), added_cond_kwargs=addd, out_dtype=torch.float32).sample
    assert (out - plain).abs().max() > 1e-2, "the features reach the output"
    # token-major features (what DenoiseEngine hands over): the same values, no transpose
    acts = [_Act(f.permute(0, 2, 3, 1).reshape(-1, f.shape[1]).contiguous(), f.shape[0], f.shape[2], f.shape[3], f.shape[1]) for f in fd]
    out_tm = unet(x.to(DEV, dtype), 981, enc.to(DEV, dtype), added_cond_kwargs=addd, down_block_additional_residuals=acts, out_dtype=torch.float32).sample
    same = torch.equal(out, out_tm)
    assert same
    with pytest.raises(ValueError):
        unet(x.to(DEV, dtype), 981, enc.to(DEV, dtype), added_cond_kwargs=addd, down_block_additional_residuals=[fd[1]] + fd[1:])


def test_unet_adapter_mode_full_sdxl_1024():
    """the full SDXL plan at 1024^2, CFG batch 2, the line-art adapter's feature shapes (320@64^2, 640@64^2, 1280@32^2, 1280@32^2), fp16"""
    import gc as _gc
    from tests.test_hotpath_gpu import _build, close, full_tol
    from theatergen_amd import config
    cfg = config.sdxl()
    dtype, T = torch.float16, 16
    unet, sd_r = _build(cfg, dtype, T=T)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 4, 128, 128, generator=g)
    enc = torch.randn(2, 77 + T, cfg.cross_attention_dim, generator=g) * 0.5
    added = {"text_embeds": torch.randn(2, 1280, generator=g), "time_ids": torch.tensor([[1024., 1024., 0., 0., 1024., 1024.]] * 2)}
    shapes = [(2, 320, 64, 64), (2, 640, 64, 64), (2, 1280, 32, 32), (2, 1280, 32, 32)]
    assert _feature_shapes(cfg, 2, 128) == shapes
    feats = [(torch.randn(s, generator=g) * 0.5).to(dtype) for s in shapes]
    out = unet(x.to(DEV, dtype), 621, enc.to(DEV, dtype), added_cond_kwargs={k: v.to(DEV) for k, v in added.items()},
               down_block_additional_residuals=[f.to(DEV) for f in feats], out_dtype=torch.float32).sample.cpu()
    del unet
    _gc.collect()
    torch.cuda.empty_cache()
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    addr = {"text_embeds": added["text_embeds"].to(dtype).float(), "time_ids": added["time_ids"]}
    ref = R.unet_forward_adapter(cfg, sd_r, x.to(dtype).float(), 621, enc.to(dtype).float(), [f.float() for f in feats], addr, ip_scale=0.4, num_tokens=T)
    close(out, ref, full_tol(dtype), "sdxl unet adapter mode full")


# ---- the engine: Euler-ancestral + adapter + frozen blend, graph replay vs eager ------------------------------------------------------
def test_engine_graph_replay_equals_eager_sdxl_flow():
    from tests.test_hotpath_gpu import _build
    from theatergen_amd import config
    from theatergen_amd.pipelines import DenoiseEngine
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler
    dtype = torch.bfloat16
    cfg = config.tiny(xl=True)
    unet, _ = _build(cfg, dtype)
    ad, _ = _build_t2i((64, 128, 256, 256), dtype)
    g = torch.Generator().manual_seed(21)
    enc = (torch.randn(2, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    added = {"text_embeds": torch.randn(2, 64, generator=g).to(DEV, dtype), "time_ids": torch.tensor([[128., 128., 0., 0., 128., 128.]] * 2, device=DEV)}
    feats = ad(torch.rand(1, 3, 128, 128, generator=g).to(DEV, dtype), token_major=True)
    lat = torch.randn(1, 4, 16, 16, generator=g) * 5
    noise = torch.randn(4, 1, 4, 16, 16, generator=g).to(DEV, dtype)
    frozen = torch.randn(5, 1, 4, 16, 16, generator=g).to(DEV)
    mask = (torch.rand(16, 16, generator=g) > 0.5).float().to(DEV)
    hs = []
    for use_graph in (True, False):
        eng = DenoiseEngine(unet, EulerAncestralDiscreteScheduler(), n_img=1, height=128, width=128, num_inference_steps=4, enc_len=81, use_graph=use_graph)
        eng.set_conditioning(enc, added)
        eng.set_adapter(feats, 0.8)
        eng.set_step_noise(noise)
        eng.set_frozen(frozen, mask, 2)
        hs.append(eng.run(lat).clone())
        if use_graph:
            assert eng.graph is not None
            again = eng.run(lat).clone()
            same_again = torch.equal(again, hs[0])
            assert same_again, "a second replay reproduces the first"
    same = torch.equal(hs[0], hs[1])
    assert same, "graph replay = eager, bit for bit"
    eng2 = DenoiseEngine(unet, EulerAncestralDiscreteScheduler(), n_img=1, height=128, width=128, num_inference_steps=4, enc_len=81)
    with pytest.raises(RuntimeError, match="set_step_noise"):
        eng2.run(lat)


# ---- the two stage functions, 'xl' ----------------------------------------------------------------------------------------------------
class _FakeXLPipe:
    """what the xl branches read from ``adapter.pipe`` / ``controlnetpipe``: ``encode_prompt`` -> 4-tuple (seeded by the prompt strings), ``vae``,
    ``scheduler``, ``unet``, ``vae_scale_factor`` (and ``adapter`` for stage 2)"""

    def __init__(self, unet, vae, scheduler, ctx, pooled=64, adapter=None):
        self.unet, self.vae, self.scheduler, self.ctx, self.pooled_dim, self.adapter = unet, vae, scheduler, ctx, pooled, adapter
        self.vae_scale_factor = 8
        self.controlnet = None
        self.prompts = []

    def emb(self, s):
        g = torch.Generator().manual_seed(sum(map(ord, s)) % 100003)
        return ((torch.randn(1, 77, self.ctx, generator=g) * 0.5).to(self.unet.device, self.unet.dtype),
                (torch.randn(1, self.pooled_dim, generator=g) * 0.5).to(self.unet.device, self.unet.dtype))

    def encode_prompt(self, prompt=None, device=None, num_images_per_prompt=1, do_classifier_free_guidance=True, negative_prompt=None, **kw):
        self.prompts.append((prompt, negative_prompt))
        (p, pp), (n, npool) = self.emb(prompt), self.emb(negative_prompt)
        return p, n, pp, npool


def _xl_setup(monkeypatch, tmp_path):
    from tests.test_hotpath_gpu import _build, _build_vae_full
    from tests.test_round6_gpu import _image_tokens_of
    from theatergen_amd import config
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.scheduler import EulerDiscreteScheduler
    from theatergen_amd.vae import tiny_vae_config
    dtype = torch.bfloat16
    cfg = config.tiny(xl=True)
    unet, sd_r = _build(cfg, dtype)
    vcfg = tiny_vae_config()
    vae, vsd = _build_vae_full(vcfg, dtype)
    pipe = _FakeXLPipe(unet, vae, EulerDiscreteScheduler(), cfg.cross_attention_dim)
    ad = IPAdapter(pipe, None, None, DEV, num_tokens=4)
    monkeypatch.setattr(ad, "get_image_embeds", lambda pil_image=None, clip_image_embeds=None: _image_tokens_of(pil_image, cfg.cross_attention_dim, DEV, dtype))
    monkeypatch.chdir(tmp_path)
    from PIL import Image
    Image.fromarray(np.full((32, 32, 3), 90, np.uint8)).save("model.png")
    return dtype, cfg, unet, sd_r, vcfg, vae, vsd, pipe, ad


def _added(pipe, prompt, negative, dtype, H=128):
    (_, pp), (_, npool) = pipe.emb(prompt), pipe.emb(negative)
    return {"text_embeds": torch.cat([npool, pp]).to(dtype).float().cpu(), "time_ids": torch.tensor([[H, H, 0., 0., H, H]] * 2)}


def test_generate_semantic_guidance_xl_vs_oracle_loop(tmp_path, monkeypatch):
    """stage 1, basever='xl' (models/pipelines.py:204-214, 255-366, 372-477): start latents from Generator(device).manual_seed(fg_seed_now) * init_noise_sigma
    (the caller's latents ignored), IP rows + pooled / time-id conditioning, Euler steps, the database PNG; a fast schedule walks the full sigma table"""
    from PIL import Image
    from oracle import unet as ou
    from oracle import vae as ov
    from tests.test_hotpath_gpu import close, net_tol
    from tests.test_round6_gpu import _image_tokens_of
    from theatergen_amd import pipelines
    from theatergen_amd.schedule import get_fast_schedule
    dtype, cfg, unet, sd_r, vcfg, vae, vsd, pipe, ad = _xl_setup(monkeypatch, tmp_path)
    db = str(tmp_path) + "/db_"
    steps, seed = 4, 77
    neg = pipelines.SINGLE_OBJECT_NEGATIVE_PROMPT

    def oracle(prompt, pil, scale, n=steps, fast=None):
        s = type(pipe.scheduler)()
        s.set_timesteps(n)
        ts = s.timesteps if fast is None else get_fast_schedule(s.timesteps, *fast)
        (p, _), (q, _) = pipe.emb(prompt), pipe.emb(neg)
        img, unc = _image_tokens_of(pil, cfg.cross_attention_dim, DEV, dtype)
        enc = torch.cat([torch.cat([q, unc], 1), torch.cat([p, img], 1)], 0).float().cpu()
        lat0 = torch.randn((1, 4, 16, 16), generator=torch.Generator(DEV).manual_seed(seed), device=DEV, dtype=dtype) * s.init_noise_sigma.to(DEV)
        ref, rows = lat0.float().cpu(), [lat0.float().cpu()]
        for i, t in enumerate(ts.tolist()):
            mi = (torch.cat([ref] * 2) / R.scale_div(s.sigmas, i)).to(dtype).float()
            npred = ou.unet_forward(cfg, sd_r, mi, t, enc, ip_scale=scale, added_cond_kwargs=_added(pipe, prompt, neg, dtype))
            u, c = npred.chunk(2)
            ref = R.euler_step(ref, u + 7.5 * (c - u), s.sigmas, i)
            rows.append(ref.clone())
        return ref, torch.stack(rows)

    kw = dict(guidance_scale=7.5, return_saved_cross_attn=True, return_box_vis=True, save_all_latents=True, obj_id=7)
    junk = torch.randn(1, 4, 8, 8).to(DEV)
    out = pipelines.generate_semantic_guidance("story", seed, "xl", "a red fox", db, 0, ad, None, junk, None, steps, None, None, None, **kw)
    assert len(out) == 5
    latents, image, saved, image2, latents_all = out
    assert latents.shape == (1, 4, 16, 16) and latents.dtype == dtype and image.size == (128, 128) and image2 is image and saved == [{}] * steps
    assert latents_all.shape == (steps + 1, 1, 4, 16, 16) and latents_all.device.type == "cpu"
    assert pipe.prompts[-1] == ("full-body picture of a red fox", neg)
    assert os.path.exists(db + "7.png"), "the first image of a character becomes its reference"
    ref, rows = oracle("full-body picture of a red fox", Image.open("model.png"), 0.0)
    close(latents, ref, net_tol(dtype), "stage 1 xl: final latents")
    close(latents_all, rows, net_tol(dtype), "stage 1 xl: latents_all")
    lat0 = torch.randn((1, 4, 16, 16), generator=torch.Generator(DEV).manual_seed(seed), device=DEV, dtype=dtype) * pipe.scheduler.init_noise_sigma.to(DEV)
    same0 = torch.equal(latents_all[0], lat0.cpu())
    assert same0, "latents_all[0] = prepare_latents(Generator(device).manual_seed(fg_seed_now)) * init_noise_sigma"
    dec = ov.decode(vcfg, vsd, latents.float().cpu())
    got_img = torch.from_numpy(np.asarray(image).astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    close(got_img, (dec / 2 + 0.5).clamp(0, 1), 8e-2, "stage 1 xl: decoded image")
    # the caller's latents are ignored: other latents, same result (the character now has a reference: scale 0.4)
    a = pipelines.generate_semantic_guidance("story", seed, "xl", "a red fox", db, 0, ad, None, junk, None, steps, None, None, None, **kw)
    b = pipelines.generate_semantic_guidance("story", seed, "xl", "a red fox", db, 0, ad, None, junk * 3 + 1, None, steps, None, None, None, **kw)
    same_ab = torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])
    assert same_ab
    ref2, _ = oracle("full-body picture of a red fox", Image.open(db + "7.png"), 0.4)
    close(a[0], ref2, net_tol(dtype), "stage 1 xl: reuse (scale 0.4)")
    # the fast schedule: 6 steps, first 2 kept, then every 2nd; sigmas by position in the replaced list
    out3 = pipelines.generate_semantic_guidance("story", seed, "xl", "a red fox", db, 0, ad, None, junk, None, 6, None, None, None,
                                                **{**kw, "fast_after_steps": 2, "fast_rate": 2})
    s6 = type(pipe.scheduler)()
    s6.set_timesteps(6)
    assert out3[4].shape[0] == len(get_fast_schedule(s6.timesteps, 2, 2)) + 1
    ref3, _ = oracle("full-body picture of a red fox", Image.open(db + "7.png"), 0.4, n=6, fast=(2, 2))
    close(out3[0], ref3, net_tol(dtype), "stage 1 xl: fast schedule")
    # refusals, before any encoding
    n_prompts = len(pipe.prompts)
    with pytest.raises(NotImplementedError, match="EulerDiscreteScheduler"):
        from theatergen_amd.scheduler import DDIMScheduler
        monkeypatch.setattr(pipe, "scheduler", DDIMScheduler())
        pipelines.generate_semantic_guidance("story", seed, "xl", "x", db, 0, ad, None, junk, None, steps, None, None, None, obj_id=7)
    assert len(pipe.prompts) == n_prompts


def test_final_image_generation_xl_vs_oracle_loop(tmp_path, monkeypatch):
    """stage 2, basever='xl' (models/pipelines.py:592-700, 733-857): generator A = posterior sample, re-noising noise (Euler add_noise: x0 + sigma noise),
    the unused background draw; generator B = start latents * init_noise_sigma, then one ancestral draw per step; T2I-Adapter features * 0.8 every step into
    controlnetpipe.unet (text rows only); frozen blend while index < frozen_steps; returns (latents, list of PIL)"""
    from PIL import Image
    from tests.test_hotpath_gpu import _build, close, net_tol
    from theatergen_amd import config, pipelines, weights
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler
    from theatergen_amd.unet import UNet2DConditionModel
    from oracle import vae as ov
    dtype, cfg, unet, sd_r, vcfg, vae, vsd, pipe, ad = _xl_setup(monkeypatch, tmp_path)
    sd2 = weights.random_unet_state_dict(cfg, seed=9, ip_adapter=False)
    sd2_r = {k: v.to(dtype).float() for k, v in sd2.items()}
    unet2 = UNet2DConditionModel.from_state_dict(cfg, sd2, device=DEV, dtype=dtype, ip_adapter=False)
    t2i, sd_t = _build_t2i((64, 128, 256, 256), dtype)
    cn = _FakeXLPipe(unet2, vae, EulerAncestralDiscreteScheduler(), cfg.cross_attention_dim, adapter=t2i)
    H = W = 128
    steps, frozen_steps, bg_seed = 4, 2, 11
    g = torch.Generator().manual_seed(43)
    pasted = Image.fromarray((torch.rand(H, W, 3, generator=g) * 255).to(torch.uint8).numpy())
    m512 = np.full((H, W), 255, np.uint8)
    m512[40:100, 24:80] = 0
    inp_mask = Image.fromarray(m512, mode="L")
    latents_all = torch.zeros(steps + 1, 1, 4, H // 8, W // 8, device=DEV)
    calls = []

    def processor(arr, detect_resolution=512, image_resolution=512):       # the line-art detector's place
        calls.append((arr.shape, detect_resolution, image_resolution))
        return Image.fromarray(255 - arr).resize((W // 2, H // 2))
    latents, images = pipelines.final_image_generation("xl", processor, cn, 1, "two foxes in a park", "lowres", "a park", [pasted], None, 0, H, W, bg_seed,
                                                       inp_mask, pasted, ad, None, latents_all, torch.ones(16, 16), None, None, steps, frozen_steps)
    assert calls == [((H, W, 3), 384, 1024)]
    assert isinstance(images, list) and len(images) == 1 and images[0].size == (W, H) and latents.shape == (1, 4, 16, 16) and latents.dtype == dtype
    assert cn.prompts[-1] == ("two foxes in a park", "lowres")
    # generator order
    gA = torch.Generator(DEV).manual_seed(bg_seed)
    n1, n2 = [torch.randn((1, 4, 16, 16), generator=gA, device=DEV, dtype=dtype) for _ in range(2)]
    gB = torch.Generator(DEV).manual_seed(bg_seed)
    ea = EulerAncestralDiscreteScheduler()
    ea.set_timesteps(steps)
    start = torch.randn((1, 4, 16, 16), generator=gB, device=DEV, dtype=dtype) * ea.init_noise_sigma.to(DEV)
    noises = [torch.randn((1, 4, 16, 16), generator=gB, device=DEV, dtype=dtype).float().cpu() for _ in range(steps)]
    same0 = torch.equal(latents_all[0], start.float())
    assert same0, "latents_all[0] = the start latents of the second bg_seed generator"
    img = (2.0 * torch.from_numpy(np.asarray(pasted).astype(np.float32) / 255.0)[None].permute(0, 3, 1, 2) - 1.0).to(dtype).float()
    mom = ov.encode_moments(vcfg, vsd, img)
    mean, logvar = mom[:, :4], mom[:, 4:].clamp(-30, 20)
    init = vcfg.scaling_factor * (mean + torch.exp(0.5 * logvar) * n1.float().cpu())
    want_rows = torch.stack([init + ea.sigmas[i] * n2.float().cpu() for i in range(steps)])
    close(latents_all[1:].cpu(), want_rows.reshape(steps, 1, 4, 16, 16), net_tol(dtype), "stage 2 xl: frozen rows = Euler add_noise at every timestep")
    # the loop, from the rows the function wrote
    ctrl = processor(np.array(pasted))
    x = torch.from_numpy(np.array(ctrl.resize((W, H), resample=Image.LANCZOS)).astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    feats = [torch.cat([f * 0.8] * 2) for f in R.t2i_adapter_forward(sd_t, x.to(dtype).float())]
    (p, _), (q, _) = cn.emb("two foxes in a park"), cn.emb("lowres")
    enc = torch.cat([q, p]).float().cpu()
    added = _added(cn, "two foxes in a park", "lowres", dtype)
    mask = torch.from_numpy(1 - (np.array(inp_mask.resize((16, 16)).convert("L")).astype(np.float32) / 255.0 > 0).astype(np.float32))
    frozen = latents_all.cpu()
    ref = frozen[0].clone()
    for i, t in enumerate(ea.timesteps.tolist()):
        mi = (torch.cat([ref] * 2) / R.scale_div(ea.sigmas, i)).to(dtype).float()
        npred = R.unet_forward_adapter(cfg, sd2_r, mi, t, enc, feats, added, cross_mode="plain")
        u, c = npred.chunk(2)
        ref = R.euler_step(ref, u + 7.5 * (c - u), ea.sigmas, i, True, noises[i])
        if i < frozen_steps:
            ref = frozen[i + 1] * mask + ref * (1 - mask)
    close(latents, ref, net_tol(dtype), "stage 2 xl: T2I-Adapter + UNet + Euler ancestral + frozen blend")
    dec = ov.decode(vcfg, vsd, latents.float().cpu())
    got = torch.from_numpy(np.asarray(images[0]).astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    close(got, (dec / 2 + 0.5).clamp(0, 1), 8e-2, "stage 2 xl: decoded image")
    # refusals up front
    n_prompts = len(cn.prompts)
    bad = _FakeXLPipe(unet2, vae, EulerAncestralDiscreteScheduler(), cfg.cross_attention_dim, adapter=object())
    with pytest.raises(NotImplementedError, match="adapter"):
        pipelines.final_image_generation("xl", processor, bad, 1, "p", "n", "b", [pasted], None, 0, H, W, bg_seed, inp_mask, pasted, ad, None, latents_all,
                                         None, None, None, steps, frozen_steps)
    bad = _FakeXLPipe(unet, vae, EulerAncestralDiscreteScheduler(), cfg.cross_attention_dim, adapter=t2i)
    bad.unet = _build(config.tiny(), dtype)[0]
    with pytest.raises(NotImplementedError, match="text_time"):
        pipelines.final_image_generation("xl", processor, bad, 1, "p", "n", "b", [pasted], None, 0, H, W, bg_seed, inp_mask, pasted, ad, None, latents_all,
                                         None, None, None, steps, frozen_steps)
    assert len(cn.prompts) == n_prompts and len(bad.prompts) == 0
