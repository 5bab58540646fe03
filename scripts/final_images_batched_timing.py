"""Stage 2 for four turns: four ``final_image_generation`` calls (arm A) against one ``generate_final_images`` (arm B), and the two image-boundary
kernels alone (profiles/final_images_batched_findings.md).  SD-1.5 plan, ControlNet, full VAE, weights drawn from seeds, 512 x 512, 50 DDIM steps.

    python scripts/final_images_batched_timing.py [--rounds 5] [--steps 50] [--out FILE]

Same process, both engines captured and warmed before timing, the arms alternate; a host clock around calls that end in their device-to-host copy of
the images.  The kernels: device events around ``inner`` back-to-back launches at [4, 512, 512, 3], bytes moved over the median time, against the
achievable HBM rate.  Needs a GPU.  Prints one JSON record; ``--out FILE`` also writes it there."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
HBM_TBS = 6.29          # measured float4-copy rate of the chip (8.0 spec): the roof a bandwidth-bound kernel is read against
N_TURNS, H, W, T = 4, 512, 512, 4


class _TextPipe:
    """what the two functions read from ``adapter.pipe``: seeded stand-in for the text encoder, the VAE, the scheduler"""

    def __init__(self, unet, vae, ctx):
        from theatergen_amd.scheduler import DDIMScheduler
        self.unet, self.vae, self.ctx = unet, vae, ctx
        self.scheduler = DDIMScheduler()
        self.vae_scale_factor = 8
        self.controlnet = None

    def encode_prompt(self, prompt, device=None, num_images_per_prompt=1, do_classifier_free_guidance=True, negative_prompt=None, **kw):
        def emb(s):
            g = torch.Generator().manual_seed(sum(map(ord, s)) % 100003)
            return (torch.randn(1, 77, self.ctx, generator=g) * 0.5).to(device=self.unet.device, dtype=self.unet.dtype)
        return emb(prompt), emb(negative_prompt)


def _image_tokens(pil_image, ctx, dtype):
    seed = int(np.asarray(pil_image.convert("RGB").resize((8, 8))).astype(np.int64).sum() % 100003)
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(1, T, ctx, generator=g) * 0.5).to(DEV, dtype),
            (torch.randn(1, T, ctx, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV, dtype))


def _spread(v):
    return {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2), "n": len(v)}


def stage2(rounds, steps):
    from PIL import Image
    from theatergen_amd import config, pipelines, weights
    from theatergen_amd.controlnet import ControlNetModel
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.unet import UNet2DConditionModel
    from theatergen_amd.vae import AutoencoderKL, sd_vae_config
    dtype = torch.bfloat16
    cfg = config.sd15()
    ctx = cfg.cross_attention_dim
    unet = UNet2DConditionModel.from_state_dict(cfg, weights.random_unet_state_dict(cfg, seed=0, device=DEV), device=DEV, dtype=dtype, num_tokens=T, ip_scale=0.1)
    net = ControlNetModel.from_state_dict(cfg, weights.random_controlnet_state_dict(cfg, seed=1), device=DEV, dtype=dtype, num_tokens=T)
    vcfg = sd_vae_config()
    vae = AutoencoderKL.from_state_dict(vcfg, weights.random_vae_state_dict(vcfg, seed=2), device=DEV, dtype=dtype)
    ad = IPAdapter(_TextPipe(unet, vae, ctx), None, None, DEV, num_tokens=T)
    ad.get_image_embeds = lambda pil_image=None, clip_image_embeds=None: _image_tokens(pil_image, ctx, dtype)
    cnpipe = type("CNPipe", (), {"controlnet": net})()
    g = torch.Generator().manual_seed(7)
    pasted = [Image.fromarray((torch.rand(H, W, 3, generator=g) * 255).to(torch.uint8).numpy()) for _ in range(N_TURNS)]
    masks = []
    for i in range(N_TURNS):
        m = np.full((H, W), 255, np.uint8)
        m[64 + 32 * i:320 + 32 * i, 96:352] = 0
        masks.append(Image.fromarray(m, mode="L"))
    chars = [Image.fromarray(np.full((64, 64, 3), 40 + 50 * i, np.uint8)) for i in range(N_TURNS)]
    texts = [(torch.randn(2, 77, ctx, generator=g) * 0.5).to(DEV, dtype) for _ in range(N_TURNS)]
    embs = [(t, t[:1], t[1:]) for t in texts]
    prompts, negs, seeds = [f"turn {i}: two foxes in a park" for i in range(N_TURNS)], ["lowres"] * N_TURNS, [11 + i for i in range(N_TURNS)]
    processor = lambda arr: Image.fromarray(255 - arr)
    frozen_steps = steps // 2
    lat_a = [torch.zeros(steps + 1, 1, 4, H // 8, W // 8, device=DEV) for _ in range(N_TURNS)]
    lat_b = [torch.zeros_like(t) for t in lat_a]

    def arm_a():
        return [pipelines.final_image_generation("1.5", processor, cnpipe, 1, prompts[i], negs[i], "bg", [chars[i]], None, 0, H, W, seeds[i], masks[i], pasted[i],
                                                 ad, None, lat_a[i], None, None, embs[i], steps, frozen_steps) for i in range(N_TURNS)]

    def arm_b():
        return pipelines.generate_final_images("1.5", processor, cnpipe, prompts, negs, [[c] for c in chars], H, W, seeds, masks, pasted, ad, lat_b, embs,
                                               steps, frozen_steps)
    arms = [("A: four final_image_generation calls", arm_a), ("B: one generate_final_images", arm_b)]
    finals = {}
    for name, fn in arms:                                                       # capture, then one warm replay of everything the timed calls touch
        fn()
        finals[name] = fn()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for r in range(rounds):
        for name, fn in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                                # ends in the device-to-host copy of its images
            times[name].append((time.perf_counter() - t0) * 1000.0)
    la = torch.cat([o[0] for o in finals[arms[0][0]]]).float()
    lb = torch.cat([o[0] for o in finals[arms[1][0]]]).float()
    ia = np.concatenate([o[1] for o in finals[arms[0][0]]]).astype(np.int32)
    ib = np.concatenate([o[1] for o in finals[arms[1][0]]]).astype(np.int32)
    rec = {name: _spread(v) for name, v in times.items()}
    a, b = rec[arms[0][0]]["median_ms"], rec[arms[1][0]]["median_ms"]
    rec["A_over_B"] = round(a / b, 3)
    rec["images_per_s"] = {"A": round(N_TURNS * 1000.0 / a, 2), "B": round(N_TURNS * 1000.0 / b, 2)}
    rec["B_vs_A_outputs"] = {"latents_rel_l2": float(((lb - la).norm() / la.norm()).item()), "row0_draws_equal": all(torch.equal(x[0], y[0]) for x, y in zip(lat_a, lat_b)),
                             "image_bytes_mean_abs_diff": float(np.abs(ia - ib).mean()), "image_bytes_max_abs_diff": int(np.abs(ia - ib).max())}
    rec["config"] = f"SD-1.5 plan + ControlNet + SD VAE, bf16, {N_TURNS} turns, {H}x{W}, {steps} DDIM steps, frozen_steps {frozen_steps}, rounds {rounds}"
    return rec


def kernels(inner=50, rounds=9):
    from theatergen_amd import ops
    g = torch.Generator().manual_seed(3)
    u8 = (torch.rand(N_TURNS, H, W, 3, generator=g) * 255).to(torch.uint8).to(DEV)
    px = N_TURNS * H * W * 3
    rec = {}
    cases = []
    for dtype, size in ((torch.bfloat16, 2), (torch.float32, 4)):
        name = str(dtype).replace("torch.", "")
        out1 = torch.empty((N_TURNS, 3, H, W), dtype=dtype, device=DEV)
        out2 = torch.empty((2 * N_TURNS, 3, H, W), dtype=dtype, device=DEV)
        x = ops.image_from_u8(u8, dtype, range_mode=1)
        o8 = torch.empty_like(u8)
        cases.append((f"tg_image_from_u8 range_mode 1 copies 1 -> {name}", lambda d=dtype, o=out1: ops.image_from_u8(u8, d, 1, 1, out=o), px + px * size))
        cases.append((f"tg_image_from_u8 range_mode 0 copies 2 -> {name}", lambda d=dtype, o=out2: ops.image_from_u8(u8, d, 0, 2, out=o), px + 2 * px * size))
        cases.append((f"tg_image_to_u8 {name} ->", lambda x=x, o=o8: ops.image_to_u8(x, out=o), px * size + px))
    for _, fn, _ in cases:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    # two clocks per case: `inner` launches issued from Python between two events (what a caller's loop sees: the wrapper's launch cadence), and the same
    # `inner` launches captured once into a graph and replayed between two events (the kernels back to back, no host in between)
    graphs = {}
    for name, fn, _ in cases:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(inner):
                fn()
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    eager = {name: [] for name, _, _ in cases}
    graph = {name: [] for name, _, _ in cases}
    for r in range(rounds):
        for name, fn, _ in (cases if r % 2 == 0 else cases[::-1]):
            for dest, work in ((eager, lambda: [fn() for _ in range(inner)]), (graph, graphs[name].replay)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                work()
                e1.record()
                e1.synchronize()
                dest[name].append(e0.elapsed_time(e1) * 1000.0 / inner)
    for name, _, nbytes in cases:
        med = statistics.median(graph[name])
        rec[name] = {"graph_median_us": round(med, 2), "graph_min_us": round(min(graph[name]), 2), "graph_max_us": round(max(graph[name]), 2),
                     "eager_median_us": round(statistics.median(eager[name]), 2), "bytes_moved": nbytes,
                     "GB_per_s": round(nbytes / med / 1e3, 1), "share_of_hbm_6.29_TB_s": round(nbytes / med / 1e6 / HBM_TBS, 3)}
    rec["note"] = (f"[{N_TURNS}, {H}, {W}, 3]; per launch, {inner} launches between two events; graph = captured once and replayed (kernel + the boundary to "
                   "the next one), eager = issued from Python; GB_per_s and the share are bytes_moved over graph_median_us; the same tensors (3-19 MB) are "
                   "reused by every launch, so they can be served from the 256 MiB Infinity Cache")
    return rec


if __name__ == "__main__":
    argv = sys.argv[1:]

    def opt(flag, default):
        if flag in argv:
            i = argv.index(flag)
            v = argv[i + 1]
            del argv[i:i + 2]
            return v
        return default
    dest, rounds, steps = opt("--out", None), int(opt("--rounds", 5)), int(opt("--steps", 50))
    if not torch.cuda.is_available():
        raise SystemExit("final_images_batched_timing.py needs a GPU: a timing taken without one says nothing")
    out = {}
    with torch.no_grad():
        out["image kernels"] = kernels()
        print(json.dumps(out["image kernels"], indent=1), flush=True)
        out["stage 2, four turns"] = stage2(max(5, rounds), steps)
    print(json.dumps(out, indent=1))
    if dest:
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "w") as f:
            json.dump(out, f, indent=1)
