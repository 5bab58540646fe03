"""SAM image encoder on the device: what the rel-pos flash attention and the whole encoder cost (bf16).

One process, HIP events, arms timed ALTERNATELY for ``--rounds`` rounds after warm-up, medians with [min, max] reported.

  (a) ``relpos_tables`` + ``attention_relpos`` against the parent commit's route for the same layer — the bias materialised as an fp32
      [B, heads, N, N] tensor and handed to ``ops.attention(mask=...)`` — at grid 64 x 16 heads x d 80 (a ViT-H global layer, one image) and at
      grid 14 x 25 windows (a windowed layer).  The mask route is timed twice: the attention launch alone (mask already in memory) and with the
      broadcast add that builds the mask from the two tables, which a caller without the new kernel pays per layer.  Peak device memory of each arm.
  (b) a ViT-H forward at batch 1 and 4 with device-drawn weights, and the share of each kernel family (HIP events around every ops call of one extra
      forward; "other" = torch indexing of the window gather / scatter, the unfold and allocations).
  (c) ``transformers.SamVisionEncoder`` (sdpa) with the same weights and dtype on the same device, if transformers imports there; else "not measured".

    python scripts/sam_encoder_timing.py [--rounds 7] [--out profiles/sam_encoder_timing.json] [--md profiles/sam_encoder_findings.md] [--errors FILE.json]

``--errors``: the per-case records tests/test_sam_gpu.py writes with ``TG_SAM_ERR_JSON`` set; they become the error table of ``--md``.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from theatergen_amd import ops  # noqa: E402
from theatergen_amd import sam as S  # noqa: E402

DEV = "cuda:0"
DTYPE = torch.bfloat16


def timed_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(routes, rounds, inner):
    for fn in routes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed_ms(fn, inner))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in t.items()}


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def attention_shape(label, grid, items, heads, d, rounds, inner, g):
    N, D = grid * grid, heads * d
    ldt = (N + 7) // 8 * 8
    qk = torch.randn(items * N, 2 * D, generator=g).to(DTYPE).to(DEV)
    vt = torch.zeros(items, D, ldt, dtype=DTYPE, device=DEV)
    vt[:, :, :N] = torch.randn(items, D, N, generator=g).to(DTYPE).to(DEV)
    rph = (0.08 * torch.randn(2 * grid - 1, d, generator=g)).to(DTYPE).to(DEV)
    rpw = (0.08 * torch.randn(2 * grid - 1, d, generator=g)).to(DTYPE).to(DEV)
    o_new = torch.empty(items * N, D, dtype=DTYPE, device=DEV)
    o_old = torch.empty(items * N, D, dtype=DTYPE, device=DEV)
    bh = torch.empty(items, heads, N, grid, device=DEV)
    bw = torch.empty(items, heads, N, grid, device=DEV)
    scale = d ** -0.5
    args = (qk, 2 * D, N * 2 * D, qk[:, D:], 2 * D, N * 2 * D, vt, ldt, D * ldt)

    def tables():
        ops.relpos_tables(qk, 2 * D, N * 2 * D, rph, rpw, items, heads, d, grid, out=(bh, bw))

    def new_attn():
        ops.attention_relpos(*args, items, heads, d, grid, scale, bh, bw, o_new, D, N * D)

    def new():
        tables()
        new_attn()

    def build_mask():
        return (bh.view(items, heads, N, grid, 1) + bw.view(items, heads, N, 1, grid)).reshape(items, heads, N, N)

    def old_attn(mask):
        ops.attention(*args, N, items, heads, d, N, scale, o_old, D, N * D, mask=mask)

    def old():
        tables()
        old_attn(build_mask())

    tables()
    mask = build_mask()
    r = alternate({"new_tables": tables, "new_attention": new_attn, "new_total": new, "mask_attention_only": lambda: old_attn(mask),
                   "mask_total": old}, rounds, inner)
    del mask
    r["peak_mib_new"] = peak_mib(new)
    r["peak_mib_mask"] = peak_mib(old)
    r["rel_l2_new_vs_mask"] = float((o_new.double() - o_old.double()).norm() / o_old.double().norm())
    flops = 4.0 * items * heads * N * N * d
    r.update(label=label, grid=grid, items=items, heads=heads, head_dim=d, inner=inner, algorithmic_flops=flops,
             tflops_new_attention=flops / (r["new_attention"]["median_ms"] * 1e-3) / 1e12,
             tflops_mask_attention=flops / (r["mask_attention_only"]["median_ms"] * 1e-3) / 1e12,
             mask_bytes=items * heads * N * N * 4, table_bytes=2 * items * heads * N * grid * 4)
    return r


FAMILIES = {"gemm": "GEMM (patch, qkv, proj, lin1, lin2, neck 1x1, neck 3x3)", "layernorm": "LayerNorm", "relpos_tables": "relpos_tables",
            "attention_relpos": "attention_relpos", "transpose": "transpose"}


def family_shares(enc, x):
    """HIP events around every ops call of one forward -> ({family: ms}, total ms); nested calls (linear / conv3x3 -> gemm) are timed at ``gemm``"""
    recs, saved = [], {}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def wrap(name, fn):
        def f(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            recs.append((name, e0, e1))
            return out
        return f
    for name in FAMILIES:
        saved[name] = getattr(ops, name)
        setattr(ops, name, wrap(name, saved[name]))
    try:
        t0.record()
        enc(x)
        t1.record()
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    fam = {k: 0.0 for k in FAMILIES}
    for name, e0, e1 in recs:
        fam[name] += e0.elapsed_time(e1)
    total = t0.elapsed_time(t1)
    fam["other"] = max(total - sum(fam.values()), 0.0)
    return fam, total


def device_weights(enc, g):
    """every parameter drawn on the device: N(0, 0.02), LayerNorm weights 1 + that"""
    with torch.no_grad():
        for name, p in enc.named_parameters():
            p.copy_(torch.randn(p.shape, device=p.device, dtype=torch.float32, generator=g) * 0.02 + (1.0 if "layer_norm" in name and name.endswith("weight") else 0.0))


def encoder_part(rounds, res):
    cfg = S.sam_vit_h_config()
    enc = S.SamVisionEncoder(cfg).to(device=DEV, dtype=DTYPE)
    gd = torch.Generator(device=DEV).manual_seed(1)
    device_weights(enc, gd)
    hf = None
    try:
        import transformers
        from transformers import SamVisionConfig
        from transformers.models.sam.modeling_sam import SamVisionEncoder as HF
        with torch.device(DEV):
            hf = HF(SamVisionConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                                    mlp_dim=cfg.mlp_dim, global_attn_indexes=cfg.global_attn_indexes, attn_implementation="sdpa")).eval().to(DTYPE)
        hf.load_state_dict(enc.state_dict())
        res["transformers"] = {"version": transformers.__version__, "attn_implementation": "sdpa"}
    except Exception as e:                                            # noqa: BLE001 - arm (c) is optional, (a) and (b) are not
        res["transformers"] = {"not_measured": repr(e)[:300]}
    res["encoder"] = []
    for B in (1, 4):
        x = torch.randn(B, 3, 1024, 1024, device=DEV, generator=gd)
        routes = {"ours": lambda: enc(x)}
        if hf is not None:
            routes["transformers_sdpa"] = lambda: hf(pixel_values=x.to(DTYPE)).last_hidden_state
        r = alternate(routes, rounds, 1)
        fam, total = family_shares(enc, x)
        r.update(batch=B, families_ms=fam, families_total_ms=total, peak_mib_ours=peak_mib(lambda: enc(x)))
        if hf is not None:
            a, b = enc(x).double(), hf(pixel_values=x.to(DTYPE)).last_hidden_state.double()
            r["rel_l2_ours_vs_transformers"] = float((a - b).norm() / b.norm())
            r["peak_mib_transformers"] = peak_mib(lambda: hf(pixel_values=x.to(DTYPE)))
            r["transformers_over_ours"] = r["transformers_sdpa"]["median_ms"] / r["ours"]["median_ms"]
        res["encoder"].append(r)
        print(json.dumps(r), flush=True)


def fmt(t):
    return f"{t['median_ms']:.3f} [{t['min_ms']:.3f}, {t['max_ms']:.3f}]"


def markdown(res, errors):
    L = ["# SAM image encoder on the device: what was measured", "",
         f"Device: {res['device']}; library built from `{res['commit']}` or later; bf16; {res['rounds']} alternating rounds per shape, HIP events around eager calls",
         "(`scripts/sam_encoder_timing.py`).  Times are median ms [min, max] over the rounds.", "",
         "## (a) The attention of one layer: separable bias in the kernel against the materialised fp32 mask", "",
         "`new` = `relpos_tables` + `attention_relpos`.  `mask` = the parent commit's route: the same two tables, a broadcast add into an fp32 [B, heads, N, N]",
         "tensor, `ops.attention(mask=...)`; `mask, attention only` times that launch with the mask already in memory.", "",
         "| shape | tables | new attention | new total | mask, attention only | mask total | mask total / new total | new attention TFLOP/s | peak MiB new | peak MiB mask |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for s in res["attention"]:
        L.append(f"| {s['label']} | {fmt(s['new_tables'])} | {fmt(s['new_attention'])} | {fmt(s['new_total'])} | {fmt(s['mask_attention_only'])} | {fmt(s['mask_total'])} | "
                 f"{s['mask_total']['median_ms'] / s['new_total']['median_ms']:.2f} | {s['tflops_new_attention']:.1f} | {s['peak_mib_new']:.1f} | {s['peak_mib_mask']:.1f} |")
    L += ["", "TFLOP/s is over the algorithmic 4 B h N^2 d (padding of d = 80 to 96 rows and of 196 keys to 256 not counted).  Outputs of the two routes on these",
          "inputs differ by rel-L2 " + ", ".join(f"{s['rel_l2_new_vs_mask']:.1e}" for s in res["attention"]) + " (both round P and O once; the fp32 sums differ in order).", ""]
    L += ["The two tables are caller buffers allocated outside the measured window (" + ", ".join(f"{s['table_bytes'] / 2 ** 20:.0f}" for s in res["attention"]) +
          " MiB per shape, in `ops.workspace` when the encoder runs), so `peak MiB new` counts only what the two launches allocate themselves.  The mask route's",
          "attention launch streams the fp32 mask once: " + ", ".join(f"{s['mask_bytes'] / (s['mask_attention_only']['median_ms'] * 1e-3) / 1e12:.2f}" for s in res["attention"]) +
          " TB/s of mask bytes alone per shape, which is what bounds it.", ""]
    L += ["## (b) ViT-H forward (32 layers x 1280 channels x 16 heads of 80, 1024 x 1024 input, device-drawn weights)", "",
          "| batch | ours | " + ("transformers sdpa | transformers / ours | ours vs transformers rel-L2 | " if "version" in res["transformers"] else "") +
          "peak MiB ours |" + (" peak MiB transformers |" if "version" in res["transformers"] else ""), "|---|---|" + ("---|---|---|" if "version" in res["transformers"] else "") + "---|" +
          ("---|" if "version" in res["transformers"] else "")]
    for r in res["encoder"]:
        row = f"| {r['batch']} | {fmt(r['ours'])} | "
        if "transformers_sdpa" in r:
            row += f"{fmt(r['transformers_sdpa'])} | {r['transformers_over_ours']:.2f} | {r['rel_l2_ours_vs_transformers']:.2e} | "
        row += f"{r['peak_mib_ours']:.0f} |"
        if "peak_mib_transformers" in r:
            row += f" {r['peak_mib_transformers']:.0f} |"
        L.append(row)
    L += ["", "Share per kernel family (one extra forward with HIP events around every `ops` call; `other` = torch indexing for the window gather / scatter, the",
          "unfold, allocations and launch gaps):", "", "| batch | " + " | ".join(list(FAMILIES) + ["other"]) + " | total ms |", "|---|" + "---|" * (len(FAMILIES) + 2)]
    for r in res["encoder"]:
        f, tot = r["families_ms"], r["families_total_ms"]
        L.append(f"| {r['batch']} | " + " | ".join(f"{f[k]:.2f} ms ({100 * f[k] / tot:.0f} %)" for k in list(FAMILIES) + ["other"]) + f" | {tot:.2f} |")
    L += ["", "## (c) transformers on the same device", ""]
    if "version" in res["transformers"]:
        L.append(f"`transformers` {res['transformers']['version']} imported on the GPU machine; its `SamVisionEncoder` (sdpa, bf16, same weights) is the `transformers sdpa` column above.")
    else:
        L.append(f"NOT MEASURED: `transformers` did not import or build on the GPU machine (`{res['transformers']['not_measured']}`).")
    if errors:
        L += ["", "## Error against fp64 (tests/test_sam_gpu.py)", "",
              "rel-L2 of `attention_relpos` and of the mask route on the same stored inputs and the same fp32 tables; the test asserts `new <= 2 x mask route`",
              "and the project's `op_tol` (max 1.5e-2 bf16 / 4e-3 fp16, rel-L2 half of it).", "", "| case | new rel-L2 | new max | mask route rel-L2 |", "|---|---|---|---|"]
        for e in errors:
            if e.get("kind") == "attention":
                L.append(f"| {e['case']} | {e['err_new']:.3e} | {e['max_new']:.3e} | {e['err_mask_route']:.3e} |")
        for e in errors:
            if e.get("kind") == "peak_memory":
                L += ["", f"Peak device memory across `relpos_tables` + `attention_relpos` at grid 64, 8 heads of 80: +{e['rise_mib']:.1f} MiB (the fp32 bias alone would be 512 MiB)."]
    L += ["", "## Still estimates", "",
          "The encoder's 2.6 TMAC (5-6 TFLOP) per image is an analytic count (parameters x tokens plus 4 N^2 d for the global layers).  The share of the SAM step in a character's generation time was not measured here: it needs the",
          "caller's prompt encoder, mask decoder and processor in the loop, which this script does not run."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--errors", default=None)
    ap.add_argument("--skip-encoder", action="store_true")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("sam_encoder_timing.py: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("sam_encoder_timing.py: needs the GPU (a CPU run measures nothing)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    except OSError:
        commit = ""
    info = os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json")
    if not commit and os.path.exists(info):
        commit = json.load(open(info)).get("commit", "")
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "dtype": "bfloat16", "unit": "ms per call", "attention": []}
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for label, grid, items, heads, d, inner in (("grid 64, 1 image x 16 heads x d 80", 64, 1, 16, 80, 5), ("grid 14, 25 windows x 16 heads x d 80", 14, 25, 16, 80, 20),
                                                    ("grid 64, 4 images x 16 heads x d 80", 64, 4, 16, 80, 2), ("grid 64, 1 image x 12 heads x d 64", 64, 1, 12, 64, 5)):
            r = attention_shape(label, grid, items, heads, d, args.rounds, inner, g)
            res["attention"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
        if not args.skip_encoder:
            encoder_part(args.rounds, res)
    errors = json.load(open(args.errors)) if args.errors and os.path.exists(args.errors) else []
    res["errors_vs_fp64"] = errors
    for path, text in ((args.out, lambda: json.dumps(res, indent=1)), (args.md, lambda: markdown(res, errors))):       # --md needs the encoder part
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text())


if __name__ == "__main__":
    main()
