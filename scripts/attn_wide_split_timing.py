"""Key-split execution of the wide-head flash attention (``tg_attention_wide_split``; ``VAEAttention.flash_split`` / ``TG_VAE_FLASH_SPLIT=1``) against the
two routes of the parent commit: the materialised route (switches off) and the unsplit flash route (``flash=True``).

Written like scripts/attn_wide_timing.py: one process, HIP events around ``inner`` eager calls, every route warmed up and then timed ALTERNATELY
(materialised, flash, flash + split, materialised, ...) for ``--rounds`` rounds, so all see the same clocks and the same neighbours; median, min and max
of the rounds are reported.  Per block shape the attention launches are also timed alone on the route's own operand layout: the unsplit launch against
the partial + combine pair at the planner's S (where it is > 1), and at B = 1, N = 4096 a sweep of forced S = 2, 4, 8.

Shapes (bf16): one attention block at C = 512 with B = 1, 2, 8 at N = 4096 (512 x 512 images) and B = 1 at N = 16384 (1024 x 1024), the block at
C = 256, B = 1, N = 4096, and the full ``decode`` of the SD VAE at 512 x 512 and 1024 x 1024 (seeded random weights).

    python scripts/attn_wide_split_timing.py [--rounds 7] [--out profiles/attn_wide_split_timing.json] [--md profiles/attn_wide_split_findings.md]

The one condition the findings state: wherever the planner answers S > 1 on a timed shape, the median of the pair must not exceed the unsplit launch's
median by more than the min-max spread seen over the rounds of that shape (both arms).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from theatergen_amd import _lib, ops  # noqa: E402
from theatergen_amd import weights as W  # noqa: E402
from theatergen_amd.unet import _Act  # noqa: E402
from theatergen_amd.vae import AutoencoderKL, VAEAttention, sd_vae_config  # noqa: E402

DEV = "cuda:0"
DTYPE = torch.bfloat16
# (label, C, B, side of the token map, inner calls per timing, forced-S sweep)
BLOCKS = [("block B=1 N=4096", 512, 1, 64, 20, (2, 4, 8)), ("block B=2 N=4096", 512, 2, 64, 10, ()), ("block B=8 N=4096", 512, 8, 64, 4, ()),
          ("block B=1 N=16384", 512, 1, 128, 3, ()), ("block C=256 B=1 N=4096", 256, 1, 64, 20, ())]
DECODES = [("decode 512x512", 64, 3), ("decode 1024x1024", 128, 1)]
ROUTES = {"materialised": (False, None), "flash": (True, False), "flash+split": (True, True)}


def timed_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(routes, rounds, inner):
    """routes: {name: fn}; -> {name: {median_ms, min_ms, max_ms}} from ``rounds`` alternating timings after two warm-up calls each"""
    for fn in routes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed_ms(fn, inner))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in t.items()}


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def planner(C_, B, N, requested=0):
    d = _lib.AttnDesc()
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.len0 = 0, B, 1, C_, N, N
    d.q = d.k0 = d.vt0 = d.out = 16                                   # sizes only: the two queries never read through a pointer
    d.q_ld, d.q_bs, d.k0_ld, d.k0_bs, d.vt0_ld, d.vt0_bs = 2 * C_, N * 2 * C_, 2 * C_, N * 2 * C_, N, C_ * N
    d.out_ld, d.out_bs, d.scale = C_, N * C_, C_ ** -0.5
    S = _lib.lib().tg_attention_wide_splits(C.byref(d), requested)
    if S < 0:
        _lib.check(S)
    return S, int(_lib.lib().tg_attention_wide_workspace_bytes(C.byref(d), S))


def block_shape(C_, B, side, rounds, inner, sweep, g):
    N = side * side
    m = {k: VAEAttention(C_, flash=f, flash_split=fs) for k, (f, fs) in ROUTES.items()}
    for mod in m.values():
        mod.load_state_dict(m["materialised"].state_dict())
        mod.requires_grad_(False).to(DEV, DTYPE)
    x = torch.randn(B * N, C_, generator=g).to(DTYPE).to(DEV)
    r = alternate({k: (lambda mod=mod: mod.run(_Act(x, B, side, side, C_))) for k, mod in m.items()}, rounds, inner)
    y = {k: mod.run(_Act(x, B, side, side, C_)).t for k, mod in m.items()}
    S, ws_bytes = planner(C_, B, N)
    r.update(planner_splits=S, workspace_bytes=ws_bytes, workgroups_unsplit=B * ((N + 127) // 128) * (C_ // 256),
             rel_l2_flash_vs_materialised=rel_l2(y["flash"], y["materialised"]), rel_l2_split_vs_flash=rel_l2(y["flash+split"], y["flash"]))
    # the attention launches alone, on the route's own operand layout
    qk = torch.randn(B * N, 2 * C_, generator=g).to(DTYPE).to(DEV)
    vt = torch.randn(B, C_, N, generator=g).to(DTYPE).to(DEV)
    o = torch.empty(B * N, C_, dtype=DTYPE, device=DEV)

    def launch(ks):
        return lambda: ops.attention_wide(qk, 2 * C_, N * 2 * C_, qk[:, C_:], 2 * C_, N * 2 * C_, vt, N, C_ * N, N, B, 1, C_, N, C_ ** -0.5, o, C_, N * C_,
                                          key_splits=ks)
    arms = {"unsplit": launch(None)}
    if S > 1:
        arms[f"S={S} (planner)"] = launch(0)
    for s in sweep:
        if s != S:
            arms[f"S={s}"] = launch(s)
    k = alternate(arms, rounds, inner)
    flops = 4.0 * B * N * N * C_
    launch(None)()
    base = o.clone()
    for name, v in k.items():
        v["tflops"] = flops / (v["median_ms"] * 1e-3) / 1e12
        if name != "unsplit":
            s = int(name.split("=")[1].split()[0])
            v["workspace_bytes"] = planner(C_, B, N, s)[1]
            launch(s)()
            v["rel_l2_vs_unsplit"] = rel_l2(o, base)
    r["launches"] = k
    if S > 1:
        u, p = k["unsplit"], k[f"S={S} (planner)"]
        spread = max(u["max_ms"] - u["min_ms"], p["max_ms"] - p["min_ms"])
        r["speed_condition"] = {"unsplit_median_ms": u["median_ms"], "pair_median_ms": p["median_ms"], "spread_ms": spread,
                                "holds": p["median_ms"] <= u["median_ms"] + spread}
    del m, x, qk, vt, o, y
    torch.cuda.empty_cache()
    return r


def decode_shape(side, rounds, inner, g):
    cfg = sd_vae_config()
    vae = AutoencoderKL.from_state_dict(cfg, W.random_vae_decoder_state_dict(cfg, seed=2), device=DEV, dtype=DTYPE)
    attn = vae.decoder.mid_block.attentions[0]
    lat = (torch.randn(1, 4, side, side, generator=g) * cfg.scaling_factor).to(DEV)

    def run(route):
        attn.flash, attn.flash_split = ROUTES[route]
        return vae.decode_latents(lat)[0]
    r = alternate({k: (lambda k=k: run(k)) for k in ROUTES}, rounds, inner)
    y = {k: run(k) for k in ROUTES}
    S, ws_bytes = planner(512, 1, side * side)
    r.update(planner_splits=S, workspace_bytes=ws_bytes, rel_l2_flash_vs_materialised=rel_l2(y["flash"], y["materialised"]),
             rel_l2_split_vs_flash=rel_l2(y["flash+split"], y["flash"]))
    del vae, lat, y
    torch.cuda.empty_cache()
    return r


def _cell(v):
    return f"{v['median_ms']:.3f} [{v['min_ms']:.3f}, {v['max_ms']:.3f}]"


def markdown(res):
    L = ["# Key split of the wide-head flash attention: what was measured", "",
         f"Device: {res['device']}; library built from `{res['commit']}` or later; {res['rounds']} alternating rounds per shape, HIP events around eager calls",
         "(`scripts/attn_wide_split_timing.py`).  `materialised` and `flash` are the parent commit's two routes (`flash=False` / `flash=True`), `flash+split` is",
         "`flash=True, flash_split=True`: the planner of `tg_attention_wide_splits` decides per shape.  bf16; ms per call, median [min, max].", "",
         "| shape | materialised | flash | flash + split | planner S | workspace bytes | split vs flash rel-L2 |", "|---|---|---|---|---|---|---|"]
    for s in res["shapes"]:
        L.append(f"| {s['label']} | {_cell(s['materialised'])} | {_cell(s['flash'])} | {_cell(s['flash+split'])} | {s['planner_splits']} | "
                 f"{s['workspace_bytes']} | {s['rel_l2_split_vs_flash']:.1e} |")
    L += ["", "The attention launches alone (unsplit: `attention_wide_kernel<d>`; split: partial + combine), rate over the algorithmic 4 B N^2 d:", "",
          "| shape | workgroups unsplit | arm | median ms [min, max] | TFLOP/s | workspace bytes | vs unsplit rel-L2 |", "|---|---|---|---|---|---|---|"]
    for s in res["shapes"]:
        for name, v in s.get("launches", {}).items():
            L.append(f"| {s['label']} | {s['workgroups_unsplit']} | {name} | {_cell(v)} | {v['tflops']:.1f} | {v.get('workspace_bytes', 0)} | "
                     + (f"{v['rel_l2_vs_unsplit']:.1e} |" if "rel_l2_vs_unsplit" in v else "- |"))
    L += ["", "Speed condition (pair median <= unsplit median + the larger min-max spread of the two arms), where the planner answers S > 1:", ""]
    for s in res["shapes"]:
        c = s.get("speed_condition")
        if c:
            L.append(f"* {s['label']}: pair {c['pair_median_ms']:.3f} ms, unsplit {c['unsplit_median_ms']:.3f} ms, spread {c['spread_ms']:.3f} ms: "
                     + ("holds" if c["holds"] else "**DOES NOT HOLD**"))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--skip-1024", action="store_true", help="leave out the N = 16384 block and the 1024 x 1024 decode")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("attn_wide_split_timing.py: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("attn_wide_split_timing.py: needs the GPU (a CPU run measures nothing)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    except OSError:
        commit = ""
    if not commit and os.path.exists(os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json")):
        commit = json.load(open(os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json"))).get("commit", "")
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "dtype": "bfloat16", "unit": "ms per call", "shapes": []}
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for label, C_, B, side, inner, sweep in BLOCKS:
            if args.skip_1024 and side == 128:
                continue
            r = block_shape(C_, B, side, args.rounds, inner, sweep, g)
            r.update(label=label, channels=C_, batch=B, n=side * side, inner=inner)
            res["shapes"].append(r)
            print(f"{label:24s} S {r['planner_splits']}  materialised {r['materialised']['median_ms']:8.3f}  flash {r['flash']['median_ms']:8.3f}  "
                  f"flash+split {r['flash+split']['median_ms']:8.3f} ms   launches: "
                  + "  ".join(f"{k} {v['median_ms']:.3f}" for k, v in r["launches"].items()), flush=True)
        for label, side, inner in DECODES:
            if args.skip_1024 and side == 128:
                continue
            r = decode_shape(side, args.rounds, inner, g)
            r.update(label=label, channels=512, batch=1, n=side * side, inner=inner)
            res["shapes"].append(r)
            print(f"{label:24s} S {r['planner_splits']}  materialised {r['materialised']['median_ms']:8.3f}  flash {r['flash']['median_ms']:8.3f}  "
                  f"flash+split {r['flash+split']['median_ms']:8.3f} ms", flush=True)
    for path, text in ((args.out, json.dumps(res, indent=1)), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
