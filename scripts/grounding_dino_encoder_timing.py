"""Timing of GroundingDINO's fusion / deformable encoder (profiles/grounding_dino_encoder_findings.md): GroundingDINO-T-sized synthetic weights
(d 256, 8 heads, ffn 2048, 6 layers), 800 x 800 (levels 100^2 + 50^2 + 25^2 + 13^2 = 13 294 tokens), 8 text tokens, batch 1 and 4.

Arms, same process, alternating, medians: A = transformers' own ``GroundingDinoEncoder`` in fp32 on the device (what runs without ``attach``; its
deformable attention does not run in half precision), B = ``GroundingDinoFusionEncoder`` in bf16.  Also, from HIP events around each call of one forward:
``tg_msdeform_attn`` per launch and the two fusion-attention launches.

    python scripts/grounding_dino_encoder_timing.py --out profiles/grounding_dino_encoder_timing.json
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/grounding_dino_encoder_timing.py --trace-forwards 4     (a run of its own)
    python scripts/grounding_dino_encoder_timing.py --count-trace DIR          (no GPU: kernel launches per forward from that trace)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = 6
SHAPES = [(100, 100), (50, 50), (25, 25), (13, 13)]


def config():
    from transformers import GroundingDinoConfig
    return GroundingDinoConfig(
        backbone_config=dict(model_type="swin", embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, out_indices=[2, 3, 4]),
        d_model=256, num_feature_levels=4, encoder_layers=LAYERS, encoder_attention_heads=8, encoder_ffn_dim=2048, encoder_n_points=4,
        disable_custom_kernels=True,
        text_config=dict(model_type="bert", hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128, vocab_size=1000))


def build():
    """(transformers encoder fp32 on the device, device encoder bf16); sampling and layer-scale weights drawn non-trivially (transformers initialises
    them to zero / 1e-4: every query would sample its own neighbourhood only)"""
    import torch
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoEncoder
    from theatergen_amd.grounding_dino_encoder import GroundingDinoFusionEncoder
    torch.manual_seed(0)
    enc = GroundingDinoEncoder(config()).eval().float()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if name.endswith("sampling_offsets.weight") or name.endswith("attention_weights.weight"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif name.endswith("_param"):
                p.copy_(0.1 + 0.02 * torch.randn(p.shape, generator=g))
    enc = enc.to("cuda")
    ours = GroundingDinoFusionEncoder.from_state_dict(enc.config, {"encoder." + k: v for k, v in enc.state_dict().items()}, "cuda", torch.bfloat16)
    return enc, ours


def inputs(B, text_len=8):
    import torch
    g = torch.Generator().manual_seed(2 + B)
    Nv = sum(h * w for h, w in SHAPES)
    spatial = torch.tensor(SHAPES, dtype=torch.long, device="cuda")
    return dict(vision_features=torch.randn(B, Nv, 256, generator=g).cuda(), vision_attention_mask=torch.zeros(B, Nv, dtype=torch.bool, device="cuda"),
                vision_position_embedding=(0.5 * torch.randn(B, Nv, 256, generator=g)).cuda(), spatial_shapes=spatial, spatial_shapes_list=list(SHAPES),
                level_start_index=torch.cat((spatial.new_zeros((1,)), spatial.prod(1).cumsum(0)[:-1])),
                valid_ratios=torch.ones(B, len(SHAPES), 2, device="cuda"), text_features=torch.randn(B, text_len, 256, generator=g).cuda(),
                text_attention_mask=torch.zeros(B, text_len, dtype=torch.bool, device="cuda"), text_position_embedding=None,
                text_self_attention_masks=~torch.eye(text_len, dtype=torch.bool, device="cuda")[None].repeat(B, 1, 1),
                text_position_ids=torch.zeros(B, text_len, dtype=torch.long, device="cuda"))


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def count_trace(directory):
    """kernel launches per forward from a rocprofv3 kernel trace of ``--trace-forwards N``: the rows from the first ``msdeform_attn_kernel`` launch of the
    second forward up to the first of the last forward span N - 2 whole forwards"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    ms = [i for i, n in enumerate(names) if "msdeform_attn_kernel" in n]
    forwards = len(ms) // LAYERS
    if forwards < 3 or len(ms) % LAYERS:
        raise SystemExit(f"{len(ms)} msdeform launches: not a whole number (>= 3) of {LAYERS}-layer forwards")
    span = names[ms[LAYERS]:ms[LAYERS * (forwards - 1)]]
    per = len(span) / (forwards - 2)
    native = sum(1 for n in span if "_GLOBAL__N_1" in n or "tg_" in n) / (forwards - 2)
    print(json.dumps({"forwards_in_trace": forwards, "kernel_launches_per_forward": per, "of_them_native_library_kernels": native}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--trace-forwards", type=int, default=0, help="only run N forwards of arm B at batch 1 (under rocprofv3 --kernel-trace)")
    ap.add_argument("--count-trace", default="", help="directory of that trace: print the launches per forward (no GPU)")
    args = ap.parse_args()
    if args.count_trace:
        return count_trace(args.count_trace)
    import torch
    from theatergen_amd import ops
    enc, ours = build()
    if args.trace_forwards:
        kw = inputs(1)
        for _ in range(args.trace_forwards):
            ours(**kw)
        torch.cuda.synchronize()
        return
    res = {"arm_a": "transformers GroundingDinoEncoder fp32", "arm_b": "GroundingDinoFusionEncoder bf16", "image": 800, "text_tokens": 8, "layers": LAYERS,
           "rounds": args.rounds, "batches": {}}
    for B in (1, 4):
        kw = inputs(B)

        def arm_a():
            with torch.no_grad():
                return enc(**kw, return_dict=True)

        def arm_b():
            return ours(**kw)
        for _ in range(2):
            arm_a(), arm_b()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        # per-launch times of the new kernels: events around each call of three forwards (the last is kept)
        recs = {"msdeform_attn": [], "attention_wide": []}
        orig = {k: getattr(ops, k) for k in recs}

        def wrap(k):
            def f(*a, **kk):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = orig[k](*a, **kk)
                e1.record()
                recs[k].append((a[13] if k == "attention_wide" else None, e0, e1))
                return r
            return f
        for k in recs:
            setattr(ops, k, wrap(k))
        try:
            for _ in range(3):
                for v in recs.values():
                    v.clear()
                arm_b()
                torch.cuda.synchronize()
        finally:
            for k in recs:
                setattr(ops, k, orig[k])
        msd = [a.elapsed_time(b) for _, a, b in recs["msdeform_attn"]]
        v2t = [a.elapsed_time(b) for n_q, a, b in recs["attention_wide"] if n_q > 64]
        t2v = [a.elapsed_time(b) for n_q, a, b in recs["attention_wide"] if n_q <= 64]
        # the same with the library's key-split planner (at most 8 splits) for the text -> vision attention
        ours.fusion_key_splits = 0
        for k in recs:
            setattr(ops, k, wrap(k))
        try:
            for _ in range(3):
                recs["attention_wide"].clear()
                arm_b()
                torch.cuda.synchronize()
        finally:
            for k in recs:
                setattr(ops, k, orig[k])
            ours.fusion_key_splits = None
        t2v_planner = [a.elapsed_time(b) for n_q, a, b in recs["attention_wide"] if n_q <= 64]
        ours.op_calls = 0
        arm_b()
        Nv = sum(h * w for h, w in SHAPES)
        gather_bytes = B * Nv * 8 * 64 * 64                      # taps x 64 bytes per (query, head), every tap counted (no reuse)
        res["batches"][str(B)] = {
            "arm_a_ms": {"median": statistics.median(ta), "min": min(ta)}, "arm_b_ms": {"median": statistics.median(tb), "min": min(tb)},
            "native_op_calls": ours.op_calls,
            "msdeform_attn_ms_per_launch": {"median": statistics.median(msd), "min": min(msd), "launches": len(msd),
                                            "tap_gb_per_s_at_median": gather_bytes / (statistics.median(msd) * 1e-3) / 1e9},
            "fusion_vision_to_text_ms": {"median": statistics.median(v2t), "launches": len(v2t)},
            "fusion_text_to_vision_ms": {"median": statistics.median(t2v), "launches": len(t2v), "includes": "partial + combine launch",
                                         "key_splits": ours._text_to_vision_splits(B, 8, (Nv + 7) // 8 * 8),
                                         "median_with_the_library_planner": statistics.median(t2v_planner)}}
        print(f"batch {B}:", json.dumps(res["batches"][str(B)]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
