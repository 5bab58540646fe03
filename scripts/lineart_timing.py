"""The lineart annotator at 512 x 512, batch 1 and 4 (profiles/lineart_findings.md):

  (a) the native forward alone (``theatergen_amd.lineart.LineartGenerator``), issued from Python and as one captured graph replayed;
  (b) the same network as plain ``torch.nn`` (tests/lineart_reference.py), eager on the device, fp32 and the storage dtype;
  (c) that restatement in fp32 on the host at 16 threads: the arm the reference's construction runs (it never moves the annotator off the CPU);
  (d) ``generate_final_images`` for four turns with the native detector in "pt" mode against the same call with arm (b, storage dtype) as ``processor``.

    python scripts/lineart_timing.py [--rounds 9] [--steps 50] [--skip-stage2] [--out profiles/lineart_timing.json]

Same process, the arms alternate, medians.  Device events around launches; a host clock around the host arm and around the stage-2 calls, which end in
their device-to-host copy.  Needs a GPU.  Seeded weights (the test suite's), a seeded image: the timings do not depend on the values."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
DEV = "cuda:0"
H = W = 512
DTYPE = torch.bfloat16


def _spread(v, unit="ms"):
    return {f"median_{unit}": round(statistics.median(v), 3), f"min_{unit}": round(min(v), 3), f"max_{unit}": round(max(v), 3), "n": len(v)}


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _count_calls(model, x):
    """C-ABI calls of one forward by wrapper, and the kernel launches they make (tg_lineart_instnorm is three; a K-split tg_gemm adds its reduce)"""
    from theatergen_amd import ops
    names = ("gemm", "conv_up2", "lineart_instnorm", "lineart_conv7_in", "lineart_conv7_out")
    counts, saved = {n: 0 for n in names}, {n: getattr(ops, n) for n in names}
    splits = []

    def wrap(n):
        def f(*a, **kw):
            counts[n] += 1
            if n == "gemm":
                splits.append(saved[n](*a, **dict(kw, plan_only=True))[2])
            return saved[n](*a, **kw)
        return f
    for n in names:
        setattr(ops, n, wrap(n))
    try:
        model(x)
    finally:
        for n in names:
            setattr(ops, n, saved[n])
    launches = counts["gemm"] + sum(1 for s in splits if s > 1) + counts["conv_up2"] + 3 * counts["lineart_instnorm"] + counts["lineart_conv7_in"] + \
        counts["lineart_conv7_out"]
    return {"c_abi_calls": counts, "gemm_k_splits": sorted(set(splits)), "kernel_launches": launches}


def forward_arms(rounds, out):
    from tests import lineart_reference as LR
    from theatergen_amd.lineart import LineartGenerator
    seeded = LR.seeded_generator()
    native = LineartGenerator()
    native.load_state_dict(seeded.state_dict())
    native = native.to(device=DEV, dtype=DTYPE).eval()
    ref_dev32 = LR.rounded_copy(seeded, DTYPE, torch.float32).to(DEV)
    ref_dev16 = LR.rounded_copy(seeded, DTYPE, DTYPE).to(DEV)
    ref_host = LR.rounded_copy(seeded, DTYPE, torch.float32)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for B in (1, 4):
        imgs = [LR.sample_image(s, H, W) for s in range(B)]
        x = torch.cat([LR.preprocess(i) for i in imgs])
        xd16, xd32 = x.to(DEV, DTYPE), x.to(DEV)
        rec = {"native": _count_calls(native, xd16)}
        arms = [("a: native forward, issued from Python", lambda: native(xd16)),
                ("b: torch.nn restatement on the device, fp32", lambda: ref_dev32(xd32)),
                ("b: torch.nn restatement on the device, bf16", lambda: ref_dev16(xd16))]
        with torch.no_grad():
            for _, fn in arms:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in arms}
            for r in range(rounds):
                for name, fn in (arms if r % 2 == 0 else arms[::-1]):
                    times[name].append(_event_ms(fn))
            for name, v in times.items():
                rec[name] = _spread(v)
            host = []
            ref_host(x)
            for _ in range(3):
                t0 = time.perf_counter()
                ref_host(x)
                host.append((time.perf_counter() - t0) * 1000.0)
            rec[f"c: torch.nn restatement on the host, fp32, {torch.get_num_threads()} threads"] = _spread(host)
        out[f"forward, batch {B}, {H}x{W}, bf16"] = rec
        print(json.dumps({f"batch {B}": rec}, indent=1), flush=True)
    # last: the native forward as one captured graph (the kernels back to back, no host in between)
    for B in (1, 4):
        xd16 = torch.cat([LR.preprocess(LR.sample_image(s, H, W)) for s in range(B)]).to(DEV, DTYPE)
        key = f"forward, batch {B}, {H}x{W}, bf16"
        try:
            with torch.no_grad():
                native(xd16)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    native(xd16)
                gr.replay()
                torch.cuda.synchronize()
                out[key]["a: native forward, captured graph replayed"] = _spread([_event_ms(gr.replay) for _ in range(rounds)])
        except Exception as e:                                                   # recorded, not hidden: the eager arm above stands on its own
            out[key]["a: native forward, captured graph replayed"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            break


def stage2(rounds, steps, out):
    import final_images_batched_timing as F2
    from PIL import Image
    from tests import lineart_reference as LR
    from theatergen_amd import config, pipelines, weights
    from theatergen_amd.controlnet import ControlNetModel
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.lineart import LineartDetector, LineartGenerator
    from theatergen_amd.unet import UNet2DConditionModel
    from theatergen_amd.vae import AutoencoderKL, sd_vae_config
    N, T = F2.N_TURNS, F2.T
    cfg = config.sd15()
    ctx = cfg.cross_attention_dim
    unet = UNet2DConditionModel.from_state_dict(cfg, weights.random_unet_state_dict(cfg, seed=0, device=DEV), device=DEV, dtype=DTYPE, num_tokens=T, ip_scale=0.1)
    net = ControlNetModel.from_state_dict(cfg, weights.random_controlnet_state_dict(cfg, seed=1), device=DEV, dtype=DTYPE, num_tokens=T)
    vcfg = sd_vae_config()
    vae = AutoencoderKL.from_state_dict(vcfg, weights.random_vae_state_dict(vcfg, seed=2), device=DEV, dtype=DTYPE)
    ad = IPAdapter(F2._TextPipe(unet, vae, ctx), None, None, DEV, num_tokens=T)
    ad.get_image_embeds = lambda pil_image=None, clip_image_embeds=None: F2._image_tokens(pil_image, ctx, DTYPE)
    cnpipe = type("CNPipe", (), {"controlnet": net})()
    pasted = [Image.fromarray(LR.sample_image(20 + i, H, W)) for i in range(N)]
    masks = []
    for i in range(N):
        m = np.full((H, W), 255, np.uint8)
        m[64 + 32 * i:320 + 32 * i, 96:352] = 0
        masks.append(Image.fromarray(m, mode="L"))
    chars = [Image.fromarray(np.full((64, 64, 3), 40 + 50 * i, np.uint8)) for i in range(N)]
    g = torch.Generator().manual_seed(7)
    texts = [(torch.randn(2, 77, ctx, generator=g) * 0.5).to(DEV, DTYPE) for _ in range(N)]
    embs = [(t, t[:1], t[1:]) for t in texts]
    prompts, negs, seeds = [f"turn {i}: two foxes in a park" for i in range(N)], ["lowres"] * N, [11 + i for i in range(N)]
    frozen_steps = steps // 2
    lat = [torch.zeros(steps + 1, 1, 4, H // 8, W // 8, device=DEV) for _ in range(N)]
    seeded = LR.seeded_generator()
    native = LineartGenerator()
    native.load_state_dict(seeded.state_dict())
    det = LineartDetector(native.to(device=DEV, dtype=DTYPE).eval(), output_type="pt")
    ref_dev = LR.rounded_copy(seeded, DTYPE, DTYPE).to(DEV)

    def torch_processor(arr):                                                    # arm (b) as the reference's processor: ndarray in, PIL image out
        return Image.fromarray(LR.byte_map(LR.run(ref_dev, LR.preprocess(arr).to(DTYPE))[0]))

    def run(processor):
        return pipelines.generate_final_images("1.5", processor, cnpipe, prompts, negs, [[c] for c in chars], H, W, seeds, masks, pasted, ad, lat, embs,
                                               steps, frozen_steps)
    arms = [("d: generate_final_images, native detector in pt mode", lambda: run(det)),
            ("d: generate_final_images, torch.nn restatement (device, bf16) as processor", lambda: run(torch_processor)),
            ("d: generate_final_images, stub processor (255 - image), for scale", lambda: run(lambda arr: Image.fromarray(255 - arr)))]
    for _, fn in arms:
        fn()
        fn()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for r in range(rounds):
        for name, fn in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1000.0)
    rec = {name: _spread(v) for name, v in times.items()}
    rec["config"] = f"SD-1.5 plan + ControlNet + SD VAE, bf16, {N} turns, {H}x{W}, {steps} DDIM steps, frozen_steps {frozen_steps}, rounds {rounds}"
    out["stage 2, four turns"] = rec


if __name__ == "__main__":
    argv = sys.argv[1:]

    def opt(flag, default):
        if flag in argv:
            i = argv.index(flag)
            v = argv[i + 1]
            del argv[i:i + 2]
            return v
        return default
    dest, rounds, steps = opt("--out", os.path.join(ROOT, "profiles", "lineart_timing.json")), int(opt("--rounds", 9)), int(opt("--steps", 50))
    if not torch.cuda.is_available():
        raise SystemExit("lineart_timing.py needs a GPU: a timing taken without one says nothing")
    out = {}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        with open(dest, "w") as f:
            json.dump(out, f, indent=1)
    if "--skip-stage2" not in argv:
        with torch.no_grad():
            stage2(max(5, rounds // 2), steps, out)
        print(json.dumps(out, indent=1), flush=True)
        save()
    forward_arms(rounds, out)
    save()
    print(json.dumps(out, indent=1))
