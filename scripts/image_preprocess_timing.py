"""Timing of the device image preprocessing (profiles/image_preprocess_findings.md), bf16, batch 1 and 4, 512 x 512 uint8 images.

Same process, arms alternating, medians and quartiles; wall clock around work that ends in a device synchronisation (the host processor is host work).
  preprocess        host: ``hf_processor(images)["pixel_values"].to(device, dtype)``; device: ``DeviceImageProcessor`` on the same PIL images (uint8
                    upload) and on a uint8 tensor already on the device — SAM (-> 1024 x 1024), GroundingDINO (-> 800 x 800), CLIP (-> 224 x 224, bicubic)
  sam               ``sam_refine_attn`` (batch 1) / ``sam_refine_characters`` (batch 4) on the device route, ViT-H-sized synthetic encoder: the caller's
                    ``SamProcessor`` (the parent route) against ``DeviceSamProcessor``
  detect            ``detect`` (batch 1) / ``detect_many`` (batch 4) through ``GroundingDinoDetector`` (GroundingDINO-T-sized synthetic weights, caption
                    cached): the host image processor (the parent route) against ``DeviceGroundingDinoProcessor``
  kernel            ``tg_image_resample_u8`` per launch from HIP events around ``--launches`` launches, against its algorithmic bytes (source read +
                    destination write) at the achievable HBM rate

    python scripts/image_preprocess_timing.py --out profiles/image_preprocess_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_ACHIEVABLE = 6.3e12            # bytes / s, the float4-copy rate of the MI355X
TEXT_IDS = [101, 2235, 3899, 1012, 2417, 4937, 1012, 102]


def stats(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1], "quartiles": [v[len(v) // 4], v[(3 * len(v)) // 4]]}


def alternate(arms, reps, warmup):
    """{name: stats of ms}: one call of every arm per round, in turn, each ending in a device synchronisation"""
    import torch
    times = {k: [] for k in arms}
    for i in range(warmup + reps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in times.items()}


def verdict(out, new, parent):
    """the condition of the findings: faster than the parent arm by more than the larger interquartile spread of the two"""
    iqr = max(out[k]["quartiles"][1] - out[k]["quartiles"][0] for k in (new, parent))
    gain = out[parent]["median"] - out[new]["median"]
    return {"gain_ms": gain, "larger_interquartile_spread_ms": iqr, "faster_by_more_than_the_spread": bool(gain > iqr)}


class Tokenizer:
    """the caption's ids on the host, as the caller's tokenizer delivers them (the tokenizer is not part of this work)"""

    def __call__(self, text, return_tensors="pt", **kw):
        import torch
        n = len(text) if isinstance(text, (list, tuple)) else 1
        ids = torch.tensor([TEXT_IDS] * n)
        return {"input_ids": ids, "attention_mask": torch.ones_like(ids), "token_type_ids": torch.zeros_like(ids)}


class HostDinoProcessor:
    def __init__(self, image_processor, tokenizer):
        self.image_processor, self.tokenizer = image_processor, tokenizer

    def __call__(self, images, text, return_tensors="pt", **kw):
        out = dict(self.image_processor(images=images, return_tensors=return_tensors))
        out.update(self.tokenizer(text, return_tensors=return_tensors, **kw))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-models", action="store_true", help="preprocessing and kernel only")
    a = ap.parse_args()
    import numpy as np
    import torch
    import transformers
    from PIL import Image
    from transformers import CLIPImageProcessor, GroundingDinoImageProcessor, SamImageProcessor, SamProcessor
    from theatergen_amd import ops, preprocess as P
    if not torch.cuda.is_available():
        raise SystemExit("image_preprocess_timing: no GPU (a timing without one says nothing)")
    dev, dt = "cuda", torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "reps": a.reps, "warmup": a.warmup, "transformers": transformers.__version__,
           "pillow": Image.__version__, "preprocess": {}, "kernel": {}, "end_to_end": {}}
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (512, 512, 3)).astype(np.uint8) for _ in range(4)]
    pil = [Image.fromarray(im) for im in images]
    on_device = torch.from_numpy(np.stack(images)).to(dev)
    hfs = {"sam": SamImageProcessor(), "grounding_dino": GroundingDinoImageProcessor(), "clip": CLIPImageProcessor()}

    # ---- the preprocessing alone
    for name, hf in hfs.items():
        dp = P.DeviceImageProcessor.from_hf(hf, dt, dev)
        for B in (1, 4):
            want = hf(images=pil[:B], return_tensors="pt")["pixel_values"].to(dt)
            got = dp(images=pil[:B])["pixel_values"]
            assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), f"{name} batch {B}: pixel_values differ from the processor's"
            out = alternate({"host_processor_plus_copy": lambda: hf(images=pil[:B], return_tensors="pt")["pixel_values"].to(dev, dt),
                             "device_from_pil": lambda: dp(images=pil[:B]),
                             "device_from_device_u8": lambda: dp(images=on_device[:B])}, a.reps, a.warmup)
            out["device_from_pil_vs_host"] = verdict(out, "device_from_pil", "host_processor_plus_copy")
            out["bytes_over_the_bus"] = {"host": int(want.numel()) * 4, "device_from_pil": B * 512 * 512 * 3}
            res["preprocess"][f"{name}_batch{B}"] = out
            print(name, B, json.dumps(out), flush=True)

    # ---- the kernel per launch
    for name, hf in hfs.items():
        dp = P.DeviceImageProcessor.from_hf(hf, dt, dev)
        (rh, rw), (oy, ox), (oh, ow) = dp.window(512, 512)
        hp, wp = dp.pad if dp.pad is not None else (oh, ow)
        pv, ph = P.device_plan(512, rh, dp.resample, dp.device), P.device_plan(512, rw, dp.resample, dp.device)
        for B in (1, 4):
            src = on_device[:B].contiguous()
            dst = torch.empty((B, 3, hp, wp), dtype=dt, device=dev)
            run = lambda: ops.image_resample_u8(src, pv, ph, dp.lut(), dt, window=(oy, ox, oh, ow), out=dst)        # noqa: E731
            for _ in range(5):
                run()
            samples = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    run()
                e1.record()
                torch.cuda.synchronize()
                samples.append(e0.elapsed_time(e1) * 1e3 / a.launches)
            nbytes = src.numel() + dst.numel() * dst.element_size()
            floor_us = nbytes / HBM_ACHIEVABLE * 1e6
            us = statistics.median(samples)
            res["kernel"][f"{name}_batch{B}"] = {"us_per_launch": stats(samples), "launches_per_sample": a.launches, "route": P.resample_route(pv[0], oy, oh)[0],
                                                 "algorithmic_bytes": nbytes, "byte_bound_us_at_6.3_TB_s": floor_us, "times_the_byte_bound": us / floor_us,
                                                 "note": "back-to-back launches on one stream: includes the launch gap between dependent kernels"}
            print("kernel", name, B, json.dumps(res["kernel"][f"{name}_batch{B}"]), flush=True)

    if not a.skip_models:
        from theatergen_amd import sam as S
        from theatergen_amd.detector import GroundingDinoDetector, detect, detect_many
        from theatergen_amd.sam import SamVisionEncoder, sam_vit_h_config
        from theatergen_amd.sam_decoder import SamModel, sam_decoder_config
        # ---- SAM end to end: ViT-H-sized synthetic encoder, the device decoder
        torch.manual_seed(0)
        hf_sam = transformers.SamModel(transformers.SamConfig(vision_config=dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, mlp_dim=32,
                                                                                 global_attn_indexes=[0]))).eval()
        sd = {k: v for k, v in hf_sam.state_dict().items() if not k.startswith("vision_encoder.")}
        model = SamModel.from_state_dict(None, sd, device=dev, dtype=dt, decoder_config=sam_decoder_config(64))
        enc = SamVisionEncoder(sam_vit_h_config())
        for p in enc.parameters():
            p.data.normal_(0, 0.02)
        for n, p in enc.named_parameters():
            if "layer_norm" in n and n.endswith(".weight"):
                p.data.fill_(1.0)
        enc = enc.to(dev, dt)
        proc = SamProcessor(image_processor=hfs["sam"])
        parent = {"sam_model": model, "sam_processor": proc, "sam_encoder": enc}
        device = {"sam_model": model, "sam_processor": P.DeviceSamProcessor(proc, dt, dev), "sam_encoder": enc}
        boxes = [[[100.0 + 10 * i, 120.0, 400.0, 420.0 - 10 * i]] for i in range(4)]
        args = (None, None, False, None, None, None, None, 0.85, 0.2, False)
        ra, rb = S.sam_refine_characters(pil, boxes, parent, 512, 512, 0.85, 0.2), S.sam_refine_characters(pil, boxes, device, 512, 512, 0.85, 0.2)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for k in range(4) for x, y in zip(ra[k], rb[k])), "the two routes' results differ"
        for B, arms in ((1, {"parent_route": lambda: S.sam_refine_attn(boxes[0], 0, pil[0], None, parent, 512, 512, *args),
                             "device_processor": lambda: S.sam_refine_attn(boxes[0], 0, pil[0], None, device, 512, 512, *args)}),
                        (4, {"parent_route": lambda: S.sam_refine_characters(pil, boxes, parent, 512, 512, 0.85, 0.2),
                             "device_processor": lambda: S.sam_refine_characters(pil, boxes, device, 512, 512, 0.85, 0.2)})):
            out = alternate(arms, a.reps, a.warmup)
            out["verdict"] = verdict(out, "device_processor", "parent_route")
            res["end_to_end"][f"sam_refine_batch{B}"] = out
            print("sam", B, json.dumps(out), flush=True)
        del enc, model, parent, device
        torch.cuda.empty_cache()

        # ---- detect end to end: GroundingDINO-T-sized synthetic weights, caption cached
        from grounding_dino_decoder_timing import config
        from transformers import GroundingDinoForObjectDetection
        torch.manual_seed(0)
        base = GroundingDinoForObjectDetection(config()).eval().float().to(dev)
        detector = GroundingDinoDetector.from_hf(base, dt)
        del base
        host = HostDinoProcessor(hfs["grounding_dino"], Tokenizer())
        gd_parent = {"model": detector, "processor": host}
        gd_device = {"model": detector, "processor": P.DeviceGroundingDinoProcessor(host, dt, dev)}
        wa, wb = detect_many(gd_parent, ["cat"] * 4, pil), detect_many(gd_device, ["cat"] * 4, pil)
        assert all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(wa, wb)), "the two routes' boxes differ"
        for B, arms in ((1, {"parent_route": lambda: detect(gd_parent, "cat", pil[0]), "device_processor": lambda: detect(gd_device, "cat", pil[0])}),
                        (4, {"parent_route": lambda: detect_many(gd_parent, ["cat"] * 4, pil),
                             "device_processor": lambda: detect_many(gd_device, ["cat"] * 4, pil)})):
            out = alternate(arms, a.reps, a.warmup)
            out["verdict"] = verdict(out, "device_processor", "parent_route")
            res["end_to_end"][f"detect_batch{B}"] = out
            print("detect", B, json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(a.out)


if __name__ == "__main__":
    main()
