"""Timings of the Segment-Anything step with the prompt encoder, mask decoder and mask post-processing on the device (profiles/sam_decoder_findings.md).

One GPU, one process, the arms of a comparison alternate, medians of ``--reps`` rounds after ``--warmup``.  ViT-H-sized synthetic weights (random, bf16), a
512 x 512 image, one box.  Writes one JSON (``--out``):

  decoder_post     the decoder run + the two ``ops.sam_mask_post`` launches of one character (image embeddings given), HIP events; the number of ``ops.*`` launches
                   in it; the summed time of its three tokens -> image attention launches (7 queries against 4096 keys) and their share
  refine_attn      ``sam_refine_attn`` end to end, wall clock with a device synchronisation: the device route against the parent route (the same encoder, then
                   ``transformers``' prompt encoder + mask decoder on the device and host post-processing) when transformers can be imported, and the processor
                   call alone (host)
  refine_characters  ``sam_refine_characters`` for 4 characters against four ``sam_refine_attn`` calls
  errors           the records tests/test_sam_decoder_gpu.py wrote through TG_SAM_ERR_JSON (``--errors path``), copied in

    python scripts/sam_decoder_timing.py --out profiles/sam_decoder_timing.json [--errors path] [--reps 15] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps, warmup, sync=True):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def _alternate(arms, reps, warmup):
    """{name: median ms}: one call of every arm per round, in turn"""
    times = {k: [] for k in arms}
    for i in range(warmup + reps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sam_decoder_timing.json")
    ap.add_argument("--errors", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from theatergen_amd import ops, sam as S
    from theatergen_amd.sam import SamVisionEncoder, sam_vit_h_config
    from theatergen_amd.sam_decoder import SamModel, sam_decoder_config
    dev, dt = "cuda", torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "reps": a.reps, "warmup": a.warmup}
    torch.manual_seed(0)

    # ---- models: one set of decoder weights for both routes
    try:
        import transformers
        from transformers import SamConfig, SamImageProcessorPil, SamProcessor
        hf = transformers.SamModel(SamConfig(vision_config=dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, mlp_dim=32, global_attn_indexes=[0]))).eval()
        sd = {k: v for k, v in hf.state_dict().items() if not k.startswith("vision_encoder.")}
        proc = SamProcessor(image_processor=SamImageProcessorPil())
        res["transformers"] = transformers.__version__
    except Exception as e:                                      # no transformers here: the device route alone, with a stand-in processor
        hf, proc = None, None
        res["transformers"] = f"not importable ({type(e).__name__}): the parent route is not timed"
        m0 = SamModel(None, sam_decoder_config(64), with_vision=False)
        sd = {k: 0.02 * torch.randn_like(v) + (1.0 if "layer_norm" in k and k.endswith(".weight") else 0.0) for k, v in m0.state_dict().items()}
    model = SamModel.from_state_dict(None, sd, device=dev, dtype=dt, decoder_config=sam_decoder_config(64))
    enc = SamVisionEncoder(sam_vit_h_config())
    for p in enc.parameters():
        p.data.normal_(0, 0.02)
    for n, p in enc.named_parameters():
        if "layer_norm" in n and n.endswith(".weight"):
            p.data.fill_(1.0)
    enc = enc.to(dev, dt)
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (512, 512, 3)).astype(np.uint8) for _ in range(4)]
    boxes = [[[100.0 + 10 * i, 120.0, 400.0, 420.0 - 10 * i]] for i in range(4)]
    if proc is None:
        class _Proc:
            def __call__(self, ims, return_tensors="pt", **kw):
                ims = ims if isinstance(ims, list) else [ims]
                pv = torch.stack([torch.from_numpy(np.ascontiguousarray(im)).permute(2, 0, 1).float().div(255).repeat_interleave(2, 1).repeat_interleave(2, 2) for im in ims])
                return {"pixel_values": pv, "original_sizes": torch.tensor([im.shape[:2] for im in ims]), "reshaped_input_sizes": torch.tensor([(1024, 1024)] * len(ims))}
        proc = _Proc()
        res["processor"] = "stand-in (nearest x2), not the PIL resize"
    md = {"sam_model": model, "sam_processor": proc, "sam_encoder": enc}
    from PIL import Image
    pil = [Image.fromarray(im) for im in images] if hf is not None else images

    # ---- decoder + post-processing of one character
    with torch.no_grad():
        emb = enc(proc(pil[0], return_tensors="pt")["pixel_values"].to(dev))
    bx = np.array([[[200.0, 240.0, 800.0, 840.0]]])
    counts, attn_ev = {}, []
    launchers = [n for n in ("gemm", "attention", "layernorm", "add", "relu", "transpose", "sam_posenc", "sam_mask_head", "sam_mask_post")]
    orig = {n: getattr(ops, n) for n in launchers}

    def counted(n):
        def f(*args, **kw):
            counts[n] = counts.get(n, 0) + 1
            if n == "attention" and args[13] <= 16 and args[9] >= 1024:                                  # n_q (tokens) against len0 (image keys)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = orig[n](*args, **kw)
                e1.record()
                attn_ev.append((e0, e1))
                return r
            return orig[n](*args, **kw)
        return f

    def decode_post():
        out = model(image_embeddings=emb, input_boxes=bx)
        for shape in ((64, 64), (512, 512)):
            ops.sam_mask_post(out.pred_masks[0], 1024, (1024, 1024), (512, 512), shape)

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    with torch.no_grad():
        for _ in range(a.warmup):
            decode_post()
        dev_ms = statistics.median(timed_events(decode_post) for _ in range(a.reps))
        wall_ms = _median_ms(decode_post, a.reps, 1)
        for n in launchers:
            setattr(ops, n, counted(n))
        try:
            shares = []
            for i in range(a.reps):
                counts.clear()
                attn_ev.clear()
                total = timed_events(decode_post)
                shares.append((sum(e0.elapsed_time(e1) for e0, e1 in attn_ev), total, len(attn_ev)))
        finally:
            for n in launchers:
                setattr(ops, n, orig[n])
    t2i = statistics.median(s[0] for s in shares)
    res["decoder_post"] = {"device_ms": dev_ms, "wall_ms_with_sync": wall_ms, "ops_launches": dict(counts), "ops_launches_total": sum(counts.values()),
                           "token_to_image_attention_launches": shares[0][2], "token_to_image_attention_ms": t2i,
                           "token_to_image_attention_share_of_device_ms": t2i / statistics.median(s[1] for s in shares)}
    print(json.dumps(res["decoder_post"]), flush=True)

    # ---- sam_refine_attn end to end
    args = (None, None, False, None, None, None, None, 0.85, 0.2, False)
    arms = {"device_route": lambda: S.sam_refine_attn([boxes[0]], 0, pil[0], None, md, 512, 512, *args)}
    if hf is not None:
        md_parent = {"sam_model": hf.to(dev, dt), "sam_processor": proc, "sam_encoder": enc}
        arms["parent_route"] = lambda: S.sam_refine_attn([boxes[0]], 0, pil[0], None, md_parent, 512, 512, *args)       # the processor's nesting: image, box
    res["refine_attn_ms"] = _alternate(arms, a.reps, a.warmup)
    res["refine_attn_ms"]["processor_call_host"] = _median_ms(lambda: proc(pil[0], return_tensors="pt"), a.reps, 1, sync=False)
    res["refine_attn_ms"]["encoder_batch1"] = _median_ms(lambda: enc(torch.zeros(1, 3, 1024, 1024, device=dev)), a.reps, 1)
    print(json.dumps(res["refine_attn_ms"]), flush=True)

    # ---- four characters
    res["refine_characters_ms"] = _alternate({
        "characters_batch4": lambda: S.sam_refine_characters(pil, boxes, md, 512, 512, 0.85, 0.2),
        "four_single_calls": lambda: [S.sam_refine_attn(boxes[i], 0, pil[i], None, md, 512, 512, *args) for i in range(4)]}, max(a.reps // 2, 3), 2)
    print(json.dumps(res["refine_characters_ms"]), flush=True)
    if a.errors and os.path.exists(a.errors):
        res["errors"] = json.load(open(a.errors))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
