"""Cross-attention sub-block at head dim 64 (SD-2.1 / SDXL): the fused norm2 + to_q + attention launch (tg_xq_attn on 128 x 128 tiles,
attention_processor.XQ_D64_ENABLED on) against the three-launch path (LayerNorm-folded to_q GEMM, attention kernel, to_out; switch off).

One process, HIP events around graph replays.  Per shape one ``IPAttnProcessor`` call the way BasicTransformerBlock makes it (the LayerNorm handed
over for folding, the conditioning registered so that its K / V^T projections and fragments are step-invariant, as under DenoiseEngine) is captured
once per route, ``--inner`` calls per graph; after a warm-up of both graphs they are replayed ALTERNATELY (off, on, off, on, ...), so both see the
same clocks and the same neighbours; median and spread of the rounds are printed.  Both routes end in the same to_out GEMM.

Shapes: SDXL at 1024^2, CFG batch 2 (8192 x 640 and 2048 x 1280, 16 image tokens, fp16), SD-2.1 at 768^2 (4608 x 640, 4 image tokens, bf16), batch 16
of the SDXL levels, and a sweep over the row count per width for the XQ_D64_MIN_ROWS default.

    python scripts/xq_d64_timing.py [--rounds 9] [--inner 20] [--out FILE.json]
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

from theatergen_amd import attention_processor as AP  # noqa: E402

DEV = "cuda:0"
# (label, C, ctx, B, N, T, dtype)
SHAPES = [
    ("sdxl 64^2 b2", 640, 2048, 2, 4096, 16, torch.float16),
    ("sdxl 32^2 b2", 1280, 2048, 2, 1024, 16, torch.float16),
    ("sd21-768 48^2 b2", 640, 1024, 2, 2304, 4, torch.bfloat16),
    ("sdxl 64^2 b16", 640, 2048, 16, 4096, 16, torch.float16),
    ("sdxl 32^2 b16", 1280, 2048, 16, 1024, 16, torch.float16),
]
SWEEP_ROWS = [256, 512, 1024, 2048, 4096, 8192, 16384]        # B = 2, N = rows / 2 (whole 128-token tiles per batch item)


def build(C, ctx, B, N, T, dtype, g):
    heads = C // 64
    attn = AP.Attention(query_dim=C, cross_attention_dim=ctx, heads=heads, dim_head=64)
    proc = AP.IPAttnProcessor(hidden_size=C, cross_attention_dim=ctx, scale=0.4, num_tokens=T)
    attn.set_processor(proc)
    attn = attn.to(DEV, dtype)
    norm = torch.nn.LayerNorm(C).to(DEV, dtype)
    x = (torch.randn(B, N, C, generator=g) * 1.2 + 0.3).to(DEV, dtype)
    enc = (torch.randn(B, 77 + T, ctx, generator=g) * 0.5).to(DEV, dtype)
    proc.register_static(attn, enc)
    return lambda: proc(attn, x, encoder_hidden_states=enc, _fused_ln=(norm, None))


def capture(fn, fused, inner):
    """-> (graph of ``inner`` calls on the chosen route, its last output, C-ABI calls of one call)"""
    from theatergen_amd import _lib
    AP.XQ_D64_ENABLED = fused
    n, orig = [0], _lib.check

    def counted(rc):
        n[0] += 1
        return orig(rc)
    fn()                                                          # eager first: weight packs and fragment blobs are made outside the capture
    _lib.check = counted
    try:
        fn()
    finally:
        _lib.check = orig
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            out = fn()
    return graph, out, n[0]


def replay_us(graph, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def measure(fn, rounds, inner):
    graphs = {"off": capture(fn, False, inner), "on": capture(fn, True, inner)}
    AP.XQ_D64_ENABLED = False
    for _ in range(2):
        for k in ("off", "on"):
            graphs[k][0].replay()
    torch.cuda.synchronize()
    t = {"off": [], "on": []}
    for _ in range(rounds):
        for k in ("off", "on"):
            t[k].append(replay_us(graphs[k][0], inner))
    r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "abi_calls": graphs[k][2]} for k, v in t.items()}
    r["off_over_on"] = r["off"]["median_us"] / r["on"]["median_us"]
    a, b = graphs["off"][1].double(), graphs["on"][1].double()
    r["rel_l2_on_vs_off"] = float((a - b).norm() / a.norm())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    assert AP.XQ_ENABLED, "TG_XQ=0 switches every fused launch off"
    AP.XQ_D64_MIN_ROWS = 128                                      # the threshold is what this script measures
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    except OSError:
        commit = ""
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner, "unit": "us per sub-block call",
           "shapes": [], "sweep": []}
    g = torch.Generator().manual_seed(0)

    def line(tag, r):
        print(f"{tag:34s} three-launch {r['off']['median_us']:8.1f} us [{r['off']['min_us']:.1f}, {r['off']['max_us']:.1f}]   fused {r['on']['median_us']:8.1f} us "
              f"[{r['on']['min_us']:.1f}, {r['on']['max_us']:.1f}]   off/on {r['off_over_on']:.3f}   C-ABI calls {r['off']['abi_calls']} -> {r['on']['abi_calls']}   "
              f"|on - off| / |off| = {r['rel_l2_on_vs_off']:.1e}", flush=True)

    with torch.no_grad():
        for label, C, ctx, B, N, T, dtype in SHAPES:
            r = measure(build(C, ctx, B, N, T, dtype, g), args.rounds, args.inner)
            r.update(label=label, C=C, ctx=ctx, batch=B, n=N, rows=B * N, ip_tokens=T, dtype=str(dtype).split(".")[-1], tiles=(B * N // 128) * (C // 128))
            res["shapes"].append(r)
            line(f"{label} {B * N} x {C} {r['dtype']}", r)
        if not args.no_sweep:
            for C in (640, 1280):
                for rows in SWEEP_ROWS:
                    r = measure(build(C, 2048, 2, rows // 2, 16, torch.float16, g), args.rounds, args.inner)
                    r.update(C=C, rows=rows, batch=2, n=rows // 2, ip_tokens=16, dtype="float16", tiles=(rows // 128) * (C // 128))
                    res["sweep"].append(r)
                    line(f"sweep {rows} x {C} float16", r)
            # smallest measured row count from which on the fused launch is never slower, per width; the default takes the larger
            res["min_rows_not_slower"] = {}
            for C in (640, 1280):
                rs = [r for r in res["sweep"] if r["C"] == C]
                ok = None
                for r in reversed(rs):
                    if r["off_over_on"] < 1.0:
                        break
                    ok = r["rows"]
                res["min_rows_not_slower"][str(C)] = ok
            print("smallest row count from which the fused launch is not slower:", res["min_rows_not_slower"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
