"""Timing of GroundingDINO's vision front (profiles/grounding_dino_vision_findings.md): Swin-T-sized synthetic weights, bf16, 800 x 800.

Arms, same process, alternating, medians: A = transformers' own ``backbone`` + ``input_proj_vision`` on the device, B = ``GroundingDinoVisionFront``.
Also: the front's calls into the native library (kernel launches are counted by scripts/grounding_dino_vision_counters.py), ``tg_attention_swin`` per stage (HIP events around each launch) with its algorithmic bytes (q + k + v + out), and the
split of arm A's whole detector forward (``--detector``, fp32) into backbone / text encoder / encoder / decoder by forward hooks.

    python scripts/grounding_dino_vision_timing.py --out profiles/grounding_dino_vision_timing.json [--detector]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def swin_t_config(full=False):
    from transformers import GroundingDinoConfig
    kw = dict(backbone_config=dict(model_type="swin", embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, out_indices=[2, 3, 4]),
              d_model=256, num_feature_levels=4, disable_custom_kernels=True)
    if not full:
        kw.update(encoder_layers=1, decoder_layers=2, text_config=dict(model_type="bert", hidden_size=64, num_hidden_layers=1, num_attention_heads=2,
                                                                        intermediate_size=128, vocab_size=1000))
    return GroundingDinoConfig(**kw)


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--detector", action="store_true", help="also split arm A's whole detector forward (BERT-base-sized text encoder, 6 + 6 layers)")
    args = ap.parse_args()
    from transformers import GroundingDinoForObjectDetection
    from theatergen_amd import ops
    from theatergen_amd.grounding_dino import GroundingDinoVisionFront
    dt = torch.bfloat16
    torch.manual_seed(0)
    model = GroundingDinoForObjectDetection(swin_t_config(args.detector)).eval().to(device="cuda", dtype=dt)
    core = model.model
    front = GroundingDinoVisionFront.from_state_dict(model.config, model.state_dict(), "cuda", dt)
    res = {"dtype": "bf16", "image": 800, "rounds": args.rounds, "batches": {}}

    def arm_a(pv, mask):
        with torch.no_grad():
            feats, _ = core.backbone(pv, mask)
            out = [core.input_proj_vision[i](f) for i, (f, _) in enumerate(feats)]
            out.append(core.input_proj_vision[3](feats[-1][0]))
        return out

    def arm_b(pv, mask):
        feats, _ = front(pv, mask)
        return front.project(feats)

    for B in (1, 4):
        pv = torch.randn(B, 3, 800, 800, device="cuda", dtype=dt)
        mask = torch.ones(B, 800, 800, dtype=torch.long, device="cuda")
        for _ in range(2):
            arm_a(pv, mask), arm_b(pv, mask)
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta += timed(lambda: arm_a(pv, mask), 1)
            tb += timed(lambda: arm_b(pv, mask), 1)
        # tg_attention_swin per stage: events around each launch of one forward
        recs, orig = [], ops.attention_swin

        def wrapped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig(*a, **k)
            e1.record()
            recs.append((a[13], a[14], a[15], a[16], e0, e1))
            return r
        ops.attention_swin = wrapped
        try:
            for _ in range(3):
                recs.clear()
                arm_b(pv, mask)
                torch.cuda.synchronize()
        finally:
            ops.attention_swin = orig
        front.op_calls = 0
        arm_b(pv, mask)
        stages = {}
        for batch, heads, H, W, e0, e1 in recs:
            s = stages.setdefault(f"{H}x{W}_h{heads}", {"launches": 0, "ms": 0.0, "alg_bytes_per_launch": 4 * batch * H * W * heads * 32 * 2})
            s["launches"] += 1
            s["ms"] += e0.elapsed_time(e1)
        for s in stages.values():
            s["gb_per_s"] = s["alg_bytes_per_launch"] * s["launches"] / (s["ms"] * 1e-3) / 1e9
        res["batches"][str(B)] = {"arm_a_ms": {"median": statistics.median(ta), "min": min(ta)}, "arm_b_ms": {"median": statistics.median(tb), "min": min(tb)},
                                  "front_native_op_calls": front.op_calls, "attention_swin": stages}
        print(f"batch {B}: A {statistics.median(ta):.2f} ms  B {statistics.median(tb):.2f} ms  native op calls {front.op_calls}", flush=True)
        for k, s in stages.items():
            print(f"   attention_swin {k}: {s['launches']} launches {s['ms']:.3f} ms, {s['gb_per_s']:.0f} GB/s algorithmic", flush=True)
    if args.detector:
        # fp32: transformers' deformable attention (grid_sample with fp32 sampling locations) does not run in bf16 / fp16 on the device
        model = model.float()
        res["detector_dtype"] = "fp32"
        pv = torch.randn(1, 3, 800, 800, device="cuda")
        ids = torch.randint(5, 900, (1, 8), device="cuda")
        kw = dict(pixel_values=pv, pixel_mask=torch.ones(1, 800, 800, dtype=torch.long, device="cuda"), input_ids=ids, attention_mask=torch.ones_like(ids),
                  token_type_ids=torch.zeros_like(ids))
        parts = {"backbone": core.backbone, "text_encoder": core.text_backbone, "encoder": core.encoder, "decoder": core.decoder}
        ev = {k: [] for k in parts}
        hooks = []
        for k, m in parts.items():
            def pre(_m, _a, _kw=None, k=k):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev[k].append([e, None])

            def post(_m, _a, _o, k=k):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev[k][-1][1] = e
            hooks += [m.register_forward_pre_hook(pre), m.register_forward_hook(post)]
        with torch.no_grad():
            for _ in range(2):
                model(**kw)
            for v in ev.values():
                v.clear()
            total = timed(lambda: model(**kw), args.rounds)
        for h in hooks:
            h.remove()
        res["detector_arm_a"] = {"total_ms_median": statistics.median(total),
                                 **{k + "_ms_median": statistics.median([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}}
        print("detector (arm A):", json.dumps(res["detector_arm_a"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
