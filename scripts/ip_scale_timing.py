"""Timings of the per-image IP scale (profiles/ip_scale_per_image_findings.md), same process, alternating arms, medians.

    python scripts/ip_scale_timing.py 1     # the three launches, one float against one float per batch item, at the flagship shapes
    python scripts/ip_scale_timing.py 3     # eight characters, four at scale 0 and four at 0.4: one n_img = 8 engine / two n_img = 4 engines / run_concurrent

Prints one JSON record; ``--out FILE`` also writes it there."""
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
out = {}


def time_forms(name, launch, scalar, vector, inner=20, rounds=15):
    """launch(scale tensor): `inner` back-to-back launches between two events; the two forms alternate; median us per launch"""
    for w in (scalar, vector):
        for _ in range(5):
            launch(w)
    torch.cuda.synchronize()
    res = {"scalar": [], "per_item": []}
    for r in range(rounds):
        for key, w in (("scalar", scalar), ("per_item", vector)) if r % 2 == 0 else (("per_item", vector), ("scalar", scalar)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                launch(w)
            e1.record()
            e1.synchronize()
            res[key].append(e0.elapsed_time(e1) * 1000.0 / inner)
    rec = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in res.items()}
    rec["per_item_over_scalar"] = round(rec["per_item"]["median_us"] / rec["scalar"]["median_us"], 4)
    out[name] = rec
    print(name, json.dumps(rec), flush=True)


def part1():
    from theatergen_amd import ops, rowchain
    from theatergen_amd.weights_pack import pack_ln_linear
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(1)
    t = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype).to(DEV)
    B, L, T = 16, 77, 4
    vec = torch.tensor([0.0, 0.4] * 8, device=DEV)
    one = torch.full((1,), 0.4, device=DEV)
    # level-0 row chain, 16 x 4096 rows
    N, C = 4096, 320
    h = t(B * N, C, sc=1.2)
    wqp = rowchain.pack_xattn_q(t(C, C, sc=C ** -0.5), None, t(C) * 0 + 1, t(C, sc=0.1), 40 ** -0.5)
    wop = rowchain.pack_xattn_out(t(C, C, sc=C ** -0.5), t(C, sc=0.1))
    vt = torch.zeros(B, C, 80, device=DEV, dtype=dtype); vt[:, :, :L] = t(B, C, L)
    vti = torch.zeros(B, C, 8, device=DEV, dtype=dtype); vti[:, :, :T] = t(B, C, T)
    kv = ops.rc_kv_pack(t(B * L, C), vt, 80, L, t(B * T, C), vti, 8, T, B)
    o = torch.empty_like(h)
    time_forms("rc_xattn 16x4096x320 T4", lambda w: ops.rc_xattn(h, wqp, kv, wop, N, 1e-5, T, ip_scale=w, out=o), one, vec)
    # fused to_q + attention, 16 x 1024 x 640 (d 80) and 16 x 256 x 1280 (d 160)
    for N, C, d in ((1024, 640, 80), (256, 1280, 160)):
        x = t(B * N, C, sc=1.2)
        wl, u, vv = pack_ln_linear(t(C, C, sc=C ** -0.5), None, t(C) * 0 + 1, t(C, sc=0.1), scale=d ** -0.5 * math.log2(math.e))
        vt = torch.zeros(B, C, 80, device=DEV, dtype=dtype); vt[:, :, :L] = t(B, C, L)
        vti = torch.zeros(B, C, 8, device=DEV, dtype=dtype); vti[:, :, :T] = t(B, C, T)
        blob = ops.xq_kv_pack(t(B * L, C), vt, 80, L, t(B * T, C), vti, 8, T, B, C, d)
        o2 = torch.empty_like(x)
        time_forms(f"xq_attn 16x{N}x{C} d{d} T4", lambda w: ops.xq_attn(x, wl, u, vv, 1e-5, blob, d, N, L, T, ip_scale=w, out=o2), one, vec)
    # attention_kernel d 40, 77 + 4 keys, 16 x 4096 queries
    N, heads, d = 4096, 8, 40
    C = heads * d
    q, k0, k1 = t(B, N, C), t(B, L, C), t(B, T, C)
    vt0 = torch.zeros(B, C, 80, device=DEV, dtype=dtype); vt0[:, :, :L] = t(B, C, L)
    vt1 = torch.zeros(B, C, 8, device=DEV, dtype=dtype); vt1[:, :, :T] = t(B, C, T)
    o3 = torch.empty_like(q)
    time_forms("attention d40 16x4096 len0 77 len1 4",
               lambda w: ops.attention(q, C, N * C, k0, C, L * C, vt0, 80, C * 80, L, B, heads, d, N, d ** -0.5, o3, C, N * C,
                                       k1=k1, k1_ld=C, k1_bs=T * C, vt1=vt1, vt1_ld=8, vt1_bs=C * 8, len1=T, w1_dev=w), one, vec)


def part3():
    import bench
    from theatergen_amd import story
    from theatergen_amd.pipelines import DenoiseEngine
    dtype, T, steps = torch.bfloat16, 4, 50
    cfg, _, unet, adapter = bench.build_model("sd15", dtype, DEV, num_tokens=T)
    _, _, unet2, _ = bench.build_model("sd15", dtype, DEV, num_tokens=T)         # the concurrent arm needs a second scale = a second UNet today
    ctx = cfg.cross_attention_dim
    scales = [0.0] * 4 + [0.4] * 4
    jobs = story.story_jobs(0, ip_scales=scales)
    shared = story.shared_conditioning(ctx, T, dtype, DEV)
    char_ids = sorted({j.char_id for j in jobs})
    img_tok = story.character_image_tokens(char_ids, ctx, T, dtype, DEV)
    cidx = {c: i for i, c in enumerate(char_ids)}
    enc = story.job_conditioning(jobs, shared, img_tok, cidx, ctx, dtype, DEV)
    lat = story.job_latents(jobs, adapter)
    mk = lambda u, n: DenoiseEngine(u, None, n_img=n, height=512, width=512, num_inference_steps=steps, guidance_scale=7.5, enc_len=77 + T)
    e8, e4 = mk(unet, 8), [mk(unet, 4), mk(unet, 4)]
    c4 = [mk(unet, 4), mk(unet2, 4)]
    halves = [list(range(k * 4, k * 4 + 4)) + list(range(8 + k * 4, 8 + k * 4 + 4)) for k in range(2)]

    def arm_vector():
        e8.set_ip_scale(story.job_ip_scales(jobs))
        e8.set_conditioning(enc)
        return e8.run(lat)[-1].clone()

    def arm_sequential():
        outs = []
        for k, e in enumerate(e4):
            e.set_ip_scale(scales[4 * k])
            e.set_conditioning(enc[halves[k]])
            outs.append(e.run(lat[4 * k:4 * k + 4])[-1].clone())
        return torch.cat(outs)

    def arm_concurrent():
        for k, e in enumerate(c4):
            e.set_ip_scale(scales[4 * k])
            e.set_conditioning(enc[halves[k]])
        hs = DenoiseEngine.run_concurrent(c4, [lat[:4], lat[4:]])
        return torch.cat([h[-1] for h in hs]).clone()
    arms = [("one n_img=8 engine, per-image scales", arm_vector), ("two n_img=4 engines, one after the other", arm_sequential),
            ("run_concurrent of two n_img=4 engines (second UNet copy)", arm_concurrent)]
    finals = {}
    for name, fn in arms:                                               # warm-up: capture
        finals[name] = fn()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for r in range(5):
        order = arms if r % 2 == 0 else arms[::-1]
        for name, fn in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1000.0)
    ref = finals[arms[1][0]].float()
    rec = {}
    for name, _ in arms:
        v = times[name]
        rec[name] = {"median_ms_per_50_step_story": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                     "rel_l2_vs_sequential": float(((finals[name].float() - ref).norm() / ref.norm()).item())}
        print(name, json.dumps(rec[name]), flush=True)
    out["eight characters (4 at scale 0, 4 at 0.4), 512x512, 50 DDIM steps, bf16"] = rec


if __name__ == "__main__":
    argv = sys.argv[1:]
    dest = None
    if "--out" in argv:
        i = argv.index("--out")
        dest = argv[i + 1]
        del argv[i:i + 2]
    which = argv or ["1", "3"]
    with torch.no_grad():
        if "1" in which:
            part1()
        if "3" in which:
            part3()
    print(json.dumps(out, indent=1))
    if dest:
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "w") as f:
            json.dump(out, f, indent=1)
