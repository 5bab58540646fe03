"""The uint8 <-> NCHW image-boundary kernels against the host expressions of the pipelines, bit for bit, and ``pipelines.generate_final_images`` (stage 2
for a list of turns in one engine run) against the oracle, per turn, at the bars of the single call's own test."""
import numpy as np
import pytest
import torch

from tests import image_boundary_reference as ibr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


# ---- tg_image_from_u8 ------------------------------------------------------------------------------------------------------------------------
# one pixel; odd sizes (h * w % 4 != 0: the one-pixel-per-thread kernel, image bases that are not 4-byte aligned); more than one image on the 4-pixel
# kernel; more than one wave; more than one block per image
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (3, 8, 8), (2, 16, 24), (1, 128, 128), (3, 7, 9)])
def test_image_from_u8_is_bit_equal_to_the_host_expression(shape):
    from theatergen_amd import ops
    batch, h, w = shape
    imgs = ibr.all_bytes_images(batch, h, w, seed=batch * 1000 + h * 10 + w)
    dev_imgs = torch.from_numpy(imgs).to(DEV)
    for dtype in OUT_DTYPES:
        for mode in (0, 1):
            for copies in (1, 2):
                got = ops.image_from_u8(dev_imgs, dtype, range_mode=mode, copies=copies)
                want = ibr.from_u8_host(imgs, dtype, mode, copies)
                assert got.shape == want.shape == (copies * batch, 3, h, w) and got.dtype == dtype
                same = torch.equal(got.cpu(), want)
                assert same, (f"tg_image_from_u8 {shape} {dtype} range_mode {mode} copies {copies}: "
                              f"{int((got.cpu() != want).sum())} of {want.numel()} elements differ from the host expression")


def test_image_kernels_on_bases_that_are_not_aligned():
    """a view one byte / one element into a buffer: the wrappers pass its address, the launcher must leave the 4-pixel kernel"""
    from theatergen_amd import ops
    imgs = ibr.all_bytes_images(3, 8, 8, seed=9)
    buf = torch.zeros(imgs.size + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(3, 8, 8, 3)
    view.copy_(torch.from_numpy(imgs))
    assert view.data_ptr() % 4 == 1
    for dtype in OUT_DTYPES:
        obuf = torch.zeros(3 * 3 * 64 + 1, dtype=dtype, device=DEV)
        out = ops.image_from_u8(view, dtype, range_mode=1, out=obuf[1:].view(3, 3, 8, 8))
        same = torch.equal(out.cpu(), ibr.from_u8_host(imgs, dtype, 1, 1))
        assert same and float(obuf[0]) == 0.0, dtype
        x = ibr.from_u8_host(imgs, dtype, 1, 1)
        xbuf = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
        xbuf[1:].copy_(x.reshape(-1))
        u8buf = torch.zeros(imgs.size + 2, dtype=torch.uint8, device=DEV)
        got = ops.image_to_u8(xbuf[1:].view(3, 3, 8, 8), out=u8buf[1:-1].view(3, 8, 8, 3))
        assert np.array_equal(got.cpu().numpy(), ibr.to_u8_host(x)) and int(u8buf[0]) == 0 and int(u8buf[-1]) == 0, dtype


# ---- tg_image_to_u8 --------------------------------------------------------------------------------------------------------------------------
def _edge_values():
    """every tie of the search, its two fp32 neighbours, +-0, +-1, +-inf, values outside [-1, 1]"""
    t = ibr.ties()
    assert len(t) >= 150
    x = np.array([v for _, v in t], np.float32)
    vals = np.concatenate([x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-2)),
                           np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1.5, -1.5, 3e38, -3e38, 1.0000001, -1.0000001, 1e-45, -1e-45, 0.9999999, -0.9999999],
                                    np.float32)])
    return vals.astype(np.float32)


# h * w % 4 != 0 (the issue's case: one pixel per thread) and h * w % 4 == 0 (four pixels per thread, 16-byte plane loads)
@pytest.mark.parametrize("hw", [(9, 13), (12, 10)])
def test_image_to_u8_fp32_ties_neighbours_and_edges(hw):
    from theatergen_amd import ops
    h, w = hw
    vals = _edge_values()
    total = 2 * 3 * h * w
    assert total >= vals.size + 7
    pool = np.random.default_rng(5).permutation(np.concatenate([vals, np.linspace(-1.2, 1.2, 7, dtype=np.float32)]))
    flat = np.resize(pool, total)                                              # shuffled, then cyclic: the ties land in all three channels of both images
    x = torch.from_numpy(flat.reshape(2, 3, h, w).copy())
    tie_bits = set(np.array([v for _, v in ibr.ties()], np.float32).view(np.uint32).tolist())
    for plane in flat.reshape(6, h * w):
        assert sum(b in tie_bits for b in plane.view(np.uint32).tolist()) >= 10
    got = ops.image_to_u8(x.to(DEV)).cpu().numpy()
    want = ibr.to_u8_host(x)
    assert got.shape == (2, h, w, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ (ties to even? one rounding of y * 255?)"
    # the reference itself tells the rounding modes apart on this input
    away = np.floor(ibr.to_u8_chain(flat) + np.float32(0.5))
    finite = np.isfinite(away)
    assert int((away[finite] != ibr.to_u8_host(x).transpose(0, 3, 1, 2).reshape(-1)[finite]).sum()) > 0


def _all_patterns(dtype, shape):
    """all 65 536 bit patterns of a 16-bit float type, NaNs replaced by 0, zero-padded to ``shape``"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype).clone()
    v[torch.isnan(v.float())] = 0
    n = int(np.prod(shape))
    assert n >= 65536
    return torch.cat([v, torch.zeros(n - 65536, dtype=dtype)]).reshape(shape)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(1, 3, 128, 171), (1, 3, 127, 173)])           # h * w % 4 == 0: four pixels per thread; odd: one pixel per thread
def test_image_to_u8_half_types_exhaustively(dtype, shape):
    from theatergen_amd import ops
    x = _all_patterns(dtype, shape)
    got = ops.image_to_u8(x.to(DEV)).cpu().numpy()
    want = ibr.to_u8_host(x)
    assert np.array_equal(got, want), f"{dtype} {shape}: {int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("dtype", OUT_DTYPES)
def test_image_to_u8_stores_zero_for_nan(dtype):
    """this project's convention (numpy's ``astype`` of NaN is undefined): NaN -> 0, on both kernels"""
    from theatergen_amd import ops
    for h, w in ((4, 4), (3, 3)):
        x = torch.full((1, 3, h, w), float("nan"), dtype=dtype)
        x[0, 1, 0, 0] = 1.0
        got = ops.image_to_u8(x.to(DEV)).cpu().numpy()
        want = np.zeros((1, h, w, 3), np.uint8)
        want[0, 0, 0, 1] = 255
        assert np.array_equal(got, want)


# ---- generate_final_images -------------------------------------------------------------------------------------------------------------------
def test_generate_final_images_two_turns_in_one_run_vs_oracle(tmp_path, monkeypatch):
    """Two turns with different pasted images, masks, prompts, character images and seeds through ONE engine run: per turn the draws of its own device
    generator, the frozen rows vs the oracle encoder, the ControlNet + UNet + frozen-mask loop vs the oracle loop of that turn alone, the image vs the oracle
    decode, the bytes vs the host expression; the host-side effects; a replay without re-capture; a one-turn list vs ``final_image_generation``."""
    from PIL import Image
    from oracle import controlnet as oc
    from oracle import ddim as oddim
    from oracle import unet as ou
    from oracle import vae as ov
    from tests.test_hotpath_gpu import _build, _build_controlnet, _build_vae_full, close, net_tol
    from tests.test_round6_gpu import _FakeTextPipe, _image_tokens_of
    from theatergen_amd import config, pipelines
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.vae import tiny_vae_config
    dtype = torch.bfloat16
    cfg = config.tiny()
    ctx = cfg.cross_attention_dim
    unet, sd_u = _build(cfg, dtype)
    net, sd_c = _build_controlnet(cfg, dtype)
    vcfg = tiny_vae_config()
    vae, vsd = _build_vae_full(vcfg, dtype)
    pipe = _FakeTextPipe(unet, vae, ctx)
    ad = IPAdapter(pipe, None, None, DEV, num_tokens=4)
    monkeypatch.setattr(ad, "get_image_embeds", lambda pil_image=None, clip_image_embeds=None: _image_tokens_of(pil_image, ctx, DEV, dtype))
    cnpipe = type("CNPipe", (), {"controlnet": net})()
    H = W = 128
    n, steps, frozen_steps = 2, 4, 3
    seeds = [11, 23]
    g = torch.Generator().manual_seed(43)

    def turn_inputs():
        pasted = [Image.fromarray((torch.rand(H, W, 3, generator=g) * 255).to(torch.uint8).numpy()) for _ in range(n)]
        texts = [(torch.randn(2, 77, ctx, generator=g) * 0.5).to(DEV, dtype) for _ in range(n)]
        return pasted, texts
    pasted, texts = turn_inputs()
    boxes = [(slice(40, 100), slice(24, 80)), (slice(8, 60), slice(56, 120))]
    masks = []
    for ys, xs in boxes:
        m = np.full((H, W), 255, np.uint8)
        m[ys, xs] = 0
        masks.append(Image.fromarray(m, mode="L"))
    chars = [Image.fromarray(np.full((32, 32, 3), 140, np.uint8)), Image.fromarray(np.full((32, 32, 3), 60, np.uint8))]
    prompts, negs = ["two foxes in a park", "a fox and an owl at night"], ["lowres", "blurry, lowres"]
    lat_all = [torch.zeros(steps + 1, 1, 4, H // 8, W // 8, device=DEV) for _ in range(n)]
    calls = []

    def processor(arr):                                       # the lineart detector's place: ndarray in, PIL out
        calls.append(arr.copy())
        return Image.fromarray(255 - arr)

    def run(pasted, texts, lat_all):
        return pipelines.generate_final_images("1.5", processor, cnpipe, prompts, negs, [[c] for c in chars], H, W, seeds, masks, pasted, ad, lat_all,
                                               [(t, t[:1], t[1:]) for t in texts], steps, frozen_steps, guidance_scale=7.5)
    assert "_tg_engines" not in ad.__dict__
    out = run(pasted, texts, lat_all)
    # ---- host-side effects
    assert len(out) == n and len(calls) == n and all(np.array_equal(c, np.asarray(p)) for c, p in zip(calls, pasted))
    assert pipe.prompts == list(zip(prompts, negs)), "encode_prompt once per turn, with that turn's strings, in order"
    assert float(unet.attn_processors[[k for k in unet.attn_processors if "attn2" in k][0]].scale) == pytest.approx(0.1)
    assert len(ad._tg_engines) == 1, "one engine for the whole batch of turns"
    eng = next(iter(ad._tg_engines.values()))
    assert eng.n_img == n and eng.graph is not None
    osch = oddim.DDIMSchedule()
    osch.set_timesteps(steps)
    stacked = torch.cat([o[0] for o in out])
    assert stacked.shape == (n, 4, 16, 16) and stacked.dtype == dtype
    # the bytes: the host expression on the decode of the returned latents, stacked in the same order (deterministic kernels: exact)
    want_u8 = ibr.to_u8_host(vae.decode(1 / 0.18215 * stacked).sample)
    for i in range(n):
        latents, images = out[i]
        assert images.shape == (1, H, W, 3) and images.dtype == np.uint8 and latents.shape == (1, 4, 16, 16)
        assert np.array_equal(images, want_u8[i:i + 1]), f"turn {i}: returned bytes != host expression of the decoded latents"
        # the turn's own device generator, in the reference's order (:625-632): posterior noise, re-noising noise, background latents
        g2 = torch.Generator(DEV).manual_seed(seeds[i])
        n1 = torch.randn((1, 4, 16, 16), generator=g2, device=DEV, dtype=dtype)
        n2 = torch.randn((1, 4, 16, 16), generator=g2, device=DEV, dtype=dtype)
        bg = torch.randn((1, 4, 16, 16), generator=g2, device=DEV, dtype=dtype)
        same = torch.equal(lat_all[i][0], bg.float())
        assert same, f"turn {i}: latents_all[0] = the third draw of its bg_seed generator"
        img = (2.0 * torch.from_numpy(np.asarray(pasted[i]).astype(np.float32) / 255.0)[None].permute(0, 3, 1, 2) - 1.0).to(dtype).float()
        mom = ov.encode_moments(vcfg, vsd, img)
        mean, logvar = mom[:, :4], mom[:, 4:].clamp(-30, 20)
        init = vcfg.scaling_factor * (mean + torch.exp(0.5 * logvar) * n1.float().cpu())
        want_rows = torch.stack([osch.add_noise(init, n2.float().cpu(), t) for t in osch.timesteps.tolist()])
        close(lat_all[i][1:].cpu(), want_rows.reshape(steps, 1, 4, 16, 16), net_tol(dtype), f"turn {i}: frozen rows = VAE-encoded pasted image re-noised at every timestep")
        # the loop of this turn alone, started from the rows the function wrote
        mask = torch.from_numpy(1 - (np.array(masks[i].resize((16, 16)).convert("L")).astype(np.float32) / 255.0 > 0).astype(np.float32))
        probe = _FakeTextPipe(unet, vae, ctx)
        pos, neg = probe.encode_prompt(prompts[i], negative_prompt=negs[i])
        tok, unc = _image_tokens_of(chars[i], ctx, DEV, dtype)
        ip_rows = torch.cat([torch.cat([neg, unc], 1), torch.cat([pos, tok], 1)], 0)
        cond = torch.from_numpy(np.asarray(Image.fromarray(255 - np.asarray(pasted[i])).resize((W, H), resample=Image.LANCZOS)).astype(np.float32) / 255.0)
        cond = torch.cat([cond.permute(2, 0, 1)[None]] * 2).to(dtype).float()
        frozen = lat_all[i].cpu()
        ref = frozen[0].clone()
        for s, t in enumerate(osch.timesteps.tolist()):
            mi = torch.cat([ref] * 2).to(dtype).float()
            rd, rm = oc.controlnet_forward(cfg, sd_c, mi, t, texts[i].float().cpu(), cond, 1.0, cross_mode="cn")
            rd = [d.to(dtype).float() for d in rd]
            npred = ou.unet_forward(cfg, sd_u, mi, t, ip_rows.float().cpu(), ip_scale=0.1, down_block_additional_residuals=rd,
                                    mid_block_additional_residual=rm.to(dtype).float())
            ref = oddim.step_epilogue(osch, npred, t, ref, 7.5, frozen[s + 1] if s < frozen_steps else None, mask)
        close(latents, ref, net_tol(dtype), f"turn {i}: ControlNet + UNet + frozen-mask loop")
        dec = ov.decode(vcfg, vsd, latents.float().cpu(), scaling_factor=0.18215)
        close(torch.from_numpy(images.astype(np.float32) / 255.0).permute(0, 3, 1, 2), (dec / 2 + 0.5).clamp(0, 1), 8e-2, f"turn {i}: decoded image")
    differs = not torch.equal(out[0][0], out[1][0])
    assert differs
    # ---- a second call with other images replays the captured step
    graph = eng.graph
    pasted2, texts2 = turn_inputs()
    lat_all2 = [torch.zeros_like(t) for t in lat_all]
    out2 = run(pasted2, texts2, lat_all2)
    assert len(ad._tg_engines) == 1 and eng.graph is graph, "same geometry: no new engine, no re-capture"
    changed = not torch.equal(out2[0][0], out[0][0])
    assert changed
    same = torch.equal(lat_all2[0][0], lat_all[0][0])
    assert same, "the same seeds draw the same background noise"
    # ---- a one-turn list vs the single call on the same inputs
    la_b, la_s = torch.zeros_like(lat_all[1]), torch.zeros_like(lat_all[1])
    one = pipelines.generate_final_images("1.5", processor, cnpipe, prompts[1:], negs[1:], [[chars[1]]], H, W, seeds[1:], masks[1:], pasted[1:], ad, [la_b],
                                          [(texts[1], texts[1][:1], texts[1][1:])], steps, frozen_steps, guidance_scale=7.5)
    lat_s, img_s = pipelines.final_image_generation("1.5", processor, cnpipe, 1, prompts[1], negs[1], "bg", [chars[1]], None, 0, H, W, seeds[1], masks[1], pasted[1],
                                                    ad, None, la_s, torch.ones(16, 16), None, (texts[1], texts[1][:1], texts[1][1:]), steps, frozen_steps,
                                                    guidance_scale=7.5)
    assert len(one) == 1 and one[0][1].shape == img_s.shape
    same = torch.equal(la_b[0], la_s[0]) and torch.equal(la_b[0], lat_all[1][0])
    assert same, "one turn: the same row-0 draw as the single call, and as the same turn inside the batch of two"
    close(la_b, la_s, net_tol(dtype), "one turn: latents_all vs final_image_generation")
    close(one[0][0], lat_s, net_tol(dtype), "one turn: latents vs final_image_generation")
    with pytest.raises(TypeError, match="ControlNetModel"):
        pipelines.generate_final_images("1.5", processor, type("P", (), {"controlnet": object()})(), prompts, negs, [[c] for c in chars], H, W, seeds, masks, pasted,
                                        ad, lat_all, [(t, t[:1], t[1:]) for t in texts], steps, frozen_steps)
