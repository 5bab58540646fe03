"""Timing of GroundingDINO's detector forward with the decoder head on the device (profiles/grounding_dino_decoder_findings.md): GroundingDINO-T-sized
synthetic weights (Swin-T, d 256, 8 heads, 6 + 6 layers, 900 queries, BERT-base-sized text backbone), 800 x 800, 8 text tokens, batch 1 and 4.

Arms, same process, alternating, medians:
  parent    the route before the decoder head existed: vision front + fusion encoder attached (bf16), the rest ``transformers`` in fp32
  attached  that route plus ``GroundingDinoDecoderHead.attach`` (``transformers`` keeps its query selection and heads)
  cold      ``GroundingDinoDetector`` with its caption cache emptied before every forward (BERT runs)
  warm      ``GroundingDinoDetector`` with the caption cached (no BERT run)
Also: the decoder head alone (``GroundingDinoDecoderHead.forward`` on fixed encoder outputs), its query selection alone, and from HIP events around each
call of one detector forward the per-launch times of ``tg_dino_contrastive``, ``tg_dino_box_update`` and ``tg_msdeform_attn`` with ``ref_dim`` 4 (four warmed forwards pooled), with the
torch expressions the two new kernels replace timed on the same operands.

    python scripts/grounding_dino_decoder_timing.py --out profiles/grounding_dino_decoder_timing.json
"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE, TEXT_IDS = 800, [101, 2235, 3899, 1012, 2417, 4937, 1012, 102]


def config():
    from transformers import GroundingDinoConfig
    return GroundingDinoConfig(
        backbone_config=dict(model_type="swin", embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, out_indices=[2, 3, 4]),
        d_model=256, num_feature_levels=4, encoder_layers=6, decoder_layers=6, encoder_attention_heads=8, decoder_attention_heads=8,
        encoder_ffn_dim=2048, decoder_ffn_dim=2048, encoder_n_points=4, decoder_n_points=4, num_queries=900, max_text_len=256,
        disable_custom_kernels=True,
        text_config=dict(model_type="bert", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=30522))


def build():
    """(parent-route model, that plus the attached decoder, the detector): weights ``transformers`` initialises to zero / 1e-4 are drawn non-trivially"""
    import torch
    from transformers import GroundingDinoForObjectDetection
    from theatergen_amd.detector import GroundingDinoDetector
    from theatergen_amd.grounding_dino import GroundingDinoVisionFront
    from theatergen_amd.grounding_dino_decoder import GroundingDinoDecoderHead
    from theatergen_amd.grounding_dino_encoder import GroundingDinoFusionEncoder
    torch.manual_seed(0)
    base = GroundingDinoForObjectDetection(config()).eval().float()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in base.named_parameters():
            if name.endswith("sampling_offsets.weight") or name.endswith("attention_weights.weight") or "bbox_embed" in name and ".layers.2." in name:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif name.endswith("_param"):
                p.copy_(0.1 + 0.02 * torch.randn(p.shape, generator=g))
    base = base.to("cuda")
    dt = torch.bfloat16
    detector = GroundingDinoDetector.from_hf(base, dt)
    sd, cfg = base.state_dict(), base.config
    models = []
    for with_decoder in (False, True):
        m = copy.deepcopy(base)
        GroundingDinoVisionFront.from_state_dict(cfg, sd, "cuda", dt).attach(m)
        GroundingDinoFusionEncoder.from_state_dict(cfg, sd, "cuda", dt).attach(m)
        if with_decoder:
            GroundingDinoDecoderHead.from_state_dict(cfg, sd, "cuda", dt).attach(m)
        models.append(m)
    del base
    return models[0], models[1], detector


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1], "quartiles": [v[len(v) // 4], v[(3 * len(v)) // 4]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    import torch
    from theatergen_amd import ops
    parent, attached, detector = build()
    head = detector.head
    res = {"image": IMAGE, "text_tokens": len(TEXT_IDS), "queries": 900, "dtype": "bf16", "rounds": args.rounds,
           "arms": {"parent": "front + encoder attached, the rest transformers fp32", "attached": "parent + decoder attached",
                    "cold": "GroundingDinoDetector, caption cache emptied", "warm": "GroundingDinoDetector, caption cached"}, "batches": {}}
    for B in (1, 4):
        gen = torch.Generator().manual_seed(2 + B)
        pv = torch.randn(B, 3, IMAGE, IMAGE, generator=gen).cuda()
        ids = torch.tensor([TEXT_IDS] * B)
        cpu_kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids))
        dev_kw = {k: v.cuda() for k, v in cpu_kw.items()}
        pm = torch.ones(B, IMAGE, IMAGE, dtype=torch.long, device="cuda")

        def hf(model):
            with torch.no_grad():
                return model(pixel_values=pv, pixel_mask=pm, **dev_kw)

        def cold():
            detector._captions.clear()
            return detector(pixel_values=pv, pixel_mask=pm, **cpu_kw)

        def warm():
            return detector(pixel_values=pv, pixel_mask=pm, **cpu_kw)
        arms = {"parent": lambda: hf(parent), "attached": lambda: hf(attached), "cold": cold, "warm": warm}
        for _ in range(2):
            for f in arms.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, f in arms.items():
                times[k].append(timed(f))

        # the decoder head alone, and its query selection alone, on fixed encoder outputs
        shapes = [(100, 100), (50, 50), (25, 25), (13, 13)]
        Nv = sum(h * w for h, w in shapes)
        mem = torch.randn(B, Nv, 256, generator=gen).to(torch.bfloat16).cuda()
        text = torch.randn(B, len(TEXT_IDS), 256, generator=gen).to(torch.bfloat16).cuda()
        valid = torch.ones(B, Nv, dtype=torch.bool, device="cuda")
        tmask = torch.ones(B, len(TEXT_IDS), dtype=torch.bool, device="cuda")
        vr = torch.ones(B, 4, 2, device="cuda")
        mem2 = mem.reshape(B * Nv, 256)

        def head_alone():
            return head(mem, valid, text, tmask, shapes, vr)

        def select_alone():
            with torch.no_grad():
                return head.select(mem2, valid, text, tmask, shapes, vr, B, Nv)
        for _ in range(2):
            head_alone(), select_alone()
        t_head = [timed(head_alone) for _ in range(args.rounds)]
        t_sel = [timed(select_alone) for _ in range(args.rounds)]
        head.op_calls = 0
        head_alone()
        head_calls = head.op_calls

        # per-launch times: events around each call of five detector forwards; the first (cold) one is dropped, the samples of the other four are pooled
        recs = {"dino_contrastive": [], "dino_box_update": [], "msdeform_attn": []}
        orig = {k: getattr(ops, k) for k in recs}

        def wrap(k):
            def f(*a, **kk):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = orig[k](*a, **kk)
                e1.record()
                tag = {"dino_contrastive": lambda: "row_max" if kk.get("row_max") else "logits", "dino_box_update": lambda: "box" if a[4] else "proposal",
                       "msdeform_attn": lambda: int(a[8].shape[-1])}[k]()
                recs[k].append((tag, e0, e1))
                return r
            return f
        for k in recs:
            setattr(ops, k, wrap(k))
        try:
            for i in range(5):
                if i == 1:
                    for v in recs.values():
                        v.clear()
                warm()
                torch.cuda.synchronize()
        finally:
            for k in recs:
                setattr(ops, k, orig[k])
        per = lambda k, tag: [a.elapsed_time(b) for t, a, b in recs[k] if t == tag]                 # noqa: E731

        # the torch expressions the two kernels replace, on the same operands (fp32, as transformers runs them behind an fp32 model)
        from transformers.models.grounding_dino.modeling_grounding_dino import encode_sinusoidal_position_embedding
        oq, t32 = torch.randn(B, Nv, 256, device="cuda"), text.float()

        def torch_scores():
            out = (oq @ t32.transpose(-1, -2)).masked_fill(~tmask[:, None, :], float("-inf"))
            new = torch.full((*out.shape[:-1], 256), float("-inf"), device="cuda")
            new[..., :out.shape[-1]] = out
            return new.max(-1)[0]
        hq, w3, b3 = torch.randn(B * 900, 256, device="cuda"), torch.randn(4, 256, device="cuda") * 0.05, torch.zeros(4, device="cuda")
        prior = torch.rand(B, 900, 4, device="cuda")

        def torch_box():
            ref = ((hq @ w3.T + b3).view(B, 900, 4) + torch.special.logit(prior, eps=1e-5)).sigmoid()
            lev = ref[:, :, None] * torch.cat([vr, vr], -1)[:, None]
            return encode_sinusoidal_position_embedding(lev[:, :, 0, :], num_pos_feats=128)
        for _ in range(2):
            torch_scores(), torch_box()
        t_ts = [timed(torch_scores) for _ in range(args.rounds)]
        t_tb = [timed(torch_box) for _ in range(args.rounds)]

        out = {k + "_ms": stats(v) for k, v in times.items()}
        spread = max(s["quartiles"][1] - s["quartiles"][0] for s in out.values())
        out.update({
            "interquartile_spread_ms_largest_arm": spread,
            "detector_warm_beats_parent_by_ms": out["parent_ms"]["median"] - out["warm_ms"]["median"],
            "detector_cold_beats_parent_by_ms": out["parent_ms"]["median"] - out["cold_ms"]["median"],
            "decoder_head_alone_ms": stats(t_head), "query_selection_alone_ms": stats(t_sel), "decoder_head_native_op_calls": head_calls,
            "dino_contrastive_row_max_ms_per_launch": stats(per("dino_contrastive", "row_max")),
            "dino_contrastive_logits_ms_per_launch": stats(per("dino_contrastive", "logits")),
            "torch_fp32_scores_expression_ms": stats(t_ts),
            "dino_box_update_ms_per_launch": dict(stats(per("dino_box_update", "box") + per("dino_box_update", "proposal")),
                                                  launches_per_forward=len(recs["dino_box_update"]) // 4),
            "torch_fp32_box_expression_ms": stats(t_tb),
            "msdeform_attn_ref_dim_4_ms_per_launch": dict(stats(per("msdeform_attn", 4)), launches_per_forward=len(per("msdeform_attn", 4)) // 4)})
        res["batches"][str(B)] = out
        print(f"batch {B}:", json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
