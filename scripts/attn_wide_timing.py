"""VAE mid-block attention (single head, d = C = 512, bf16): the flash route (``VAEAttention.flash`` / ``TG_VAE_FLASH=1``: one Q|K|V^T GEMM, one
``tg_attention_wide`` launch for the batch) against the materialised route of the parent commit (Q and K|V^T GEMMs, then per batch item
scores GEMM -> ``tg_softmax_rows`` -> PV GEMM), which is what the switch off runs.

One process, HIP events around ``--inner`` eager calls.  Per shape both routes are warmed up, then timed ALTERNATELY (off, on, off, on, ...) for
``--rounds`` rounds, so both see the same clocks and the same neighbours; median, min and max of the rounds are reported.  The attention kernel is
also timed alone on the same shapes (achieved TFLOP/s over the algorithmic 4 B N^2 d: the column half that d = 512 recomputes is not counted).

Shapes: one attention block at B = 1 and 8 with N = 4096 (512 x 512 images) and B = 1 with N = 16384 (1024 x 1024), and the full ``decode`` of
the SD VAE at 512 x 512 and 1024 x 1024 (seeded random weights).

    python scripts/attn_wide_timing.py [--rounds 7] [--out profiles/attn_wide_timing.json] [--md profiles/attn_wide_findings.md] [--errors FILE.json]

``--errors``: the per-case error pairs tests/test_attn_wide_gpu.py writes with ``TG_ATTN_WIDE_ERR_JSON`` set; they become the table of ``--md``.
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
from theatergen_amd import weights as W  # noqa: E402
from theatergen_amd.unet import _Act  # noqa: E402
from theatergen_amd.vae import AutoencoderKL, VAEAttention, sd_vae_config  # noqa: E402

DEV = "cuda:0"
DTYPE = torch.bfloat16
C_ = 512
# (label, B, side of the token map, inner calls per timing)
BLOCKS = [("block B=1 N=4096", 1, 64, 20), ("block B=8 N=4096", 8, 64, 4), ("block B=1 N=16384", 1, 128, 3)]
DECODES = [("decode 512x512", 64, 3), ("decode 1024x1024", 128, 1)]


def clocks():
    """current clocks as the management tool reports them (read only); None where the tool is missing"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=60)
        card = next(iter(json.loads(r.stdout).values()))
        return {k: v for k, v in card.items() if "clock" in k.lower()}
    except Exception as e:                                            # noqa: BLE001 - the record is optional, the timings are not
        return {"unavailable": repr(e)[:200]}


def timed_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(routes, rounds, inner):
    """routes: {name: fn}; -> {name: {median_ms, min_ms, max_ms, spread}} from ``rounds`` alternating timings after two warm-up calls each"""
    for fn in routes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed_ms(fn, inner))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / statistics.median(v)}
            for k, v in t.items()}


def block_shape(B, side, rounds, inner, g):
    m = {on: VAEAttention(C_, flash=on) for on in (False, True)}
    m[True].load_state_dict(m[False].state_dict())
    for mod in m.values():
        mod.requires_grad_(False).to(DEV, DTYPE)
    N = side * side
    x = torch.randn(B * N, C_, generator=g).to(DTYPE).to(DEV)
    r = alternate({"off": lambda: m[False].run(_Act(x, B, side, side, C_)), "on": lambda: m[True].run(_Act(x, B, side, side, C_))}, rounds, inner)
    a, b = m[False].run(_Act(x, B, side, side, C_)).t.double(), m[True].run(_Act(x, B, side, side, C_)).t.double()
    r["rel_l2_on_vs_off"] = float((a - b).norm() / a.norm())
    r["off_over_on"] = r["off"]["median_ms"] / r["on"]["median_ms"]
    # the attention launch alone, on the route's own operand layout
    qk = torch.randn(B * N, 2 * C_, generator=g).to(DTYPE).to(DEV)
    vt = torch.randn(B, C_, N, generator=g).to(DTYPE).to(DEV)
    o = torch.empty(B * N, C_, dtype=DTYPE, device=DEV)
    k = alternate({"kernel": lambda: ops.attention_wide(qk, 2 * C_, N * 2 * C_, qk[:, C_:], 2 * C_, N * 2 * C_, vt, N, C_ * N, N, B, 1, C_, N,
                                                        C_ ** -0.5, o, C_, N * C_)}, rounds, inner)["kernel"]
    flops = 4.0 * B * N * N * C_
    r["kernel"] = dict(k, algorithmic_flops=flops, tflops=flops / (k["median_ms"] * 1e-3) / 1e12,
                       workgroups=B * ((N + 127) // 128) * 2)              # 128-query blocks x the two 256-column halves of d = 512
    del m, x, qk, vt, o
    torch.cuda.empty_cache()
    return r


def decode_shape(side, rounds, inner, g):
    cfg = sd_vae_config()
    vae = AutoencoderKL.from_state_dict(cfg, W.random_vae_decoder_state_dict(cfg, seed=2), device=DEV, dtype=DTYPE)
    attn = vae.decoder.mid_block.attentions[0]
    lat = (torch.randn(1, 4, side, side, generator=g) * cfg.scaling_factor).to(DEV)

    def run(on):
        attn.flash = on
        return vae.decode_latents(lat)[0]
    r = alternate({"off": lambda: run(False), "on": lambda: run(True)}, rounds, inner)
    a, b = run(False).double(), run(True).double()
    r["rel_l2_on_vs_off"] = float((a - b).norm() / a.norm())
    r["off_over_on"] = r["off"]["median_ms"] / r["on"]["median_ms"]
    del vae, lat
    torch.cuda.empty_cache()
    return r


def markdown(res, errors):
    L = ["# Wide-head flash attention for the VAE mid block: what was measured", "",
         f"Device: {res['device']}; library built from `{res['commit']}` or later; {res['rounds']} alternating rounds per shape, HIP events around eager calls",
         "(`scripts/attn_wide_timing.py`).  `off` is the materialised route of the parent commit, `on` is `VAEAttention.flash` / `TG_VAE_FLASH=1`.",
         f"Clocks before: `{json.dumps(res['clocks_before'])}`; after: `{json.dumps(res['clocks_after'])}`.", "",
         "| shape (C = 512, bf16) | off median ms [min, max] | on median ms [min, max] | off / on | on vs off rel-L2 |", "|---|---|---|---|---|"]
    for s in res["shapes"]:
        L.append(f"| {s['label']} | {s['off']['median_ms']:.3f} [{s['off']['min_ms']:.3f}, {s['off']['max_ms']:.3f}] | "
                 f"{s['on']['median_ms']:.3f} [{s['on']['min_ms']:.3f}, {s['on']['max_ms']:.3f}] | {s['off_over_on']:.3f} | {s['rel_l2_on_vs_off']:.1e} |")
    L += ["", "The attention launch alone (`attention_wide_kernel<d512>`), achieved rate over the algorithmic 4 B N^2 d:", "",
          "| shape | workgroups (256 CUs) | median ms [min, max] | TFLOP/s |", "|---|---|---|---|"]
    for s in res["shapes"]:
        if "kernel" in s:
            k = s["kernel"]
            L.append(f"| {s['label']} | {k['workgroups']} | {k['median_ms']:.3f} [{k['min_ms']:.3f}, {k['max_ms']:.3f}] | {k['tflops']:.1f} |")
    if errors:
        L += ["", "## Error against fp64 (tests/test_attn_wide_gpu.py)", "",
              "rel-L2 of the new kernel and of the materialised route (scores GEMM -> `softmax_rows` -> PV GEMM) on the same stored inputs; the test asserts",
              "`err_new <= err_materialised` and `err_new <= 2^-8` (bf16) / `2^-11` (fp16) per case.", "",
              "| case | err_new | err_materialised |", "|---|---|---|"]
        for e in errors:
            L.append(f"| {e['case']} | {e['err_new']:.3e} | {e['err_materialised']:.3e} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--errors", default=None)
    ap.add_argument("--skip-1024", action="store_true", help="leave out the N = 16384 block and the 1024 x 1024 decode")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("attn_wide_timing.py: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("attn_wide_timing.py: needs the GPU (a CPU run measures nothing)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    except OSError:
        commit = ""
    if not commit and os.path.exists(os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json")):
        commit = json.load(open(os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json"))).get("commit", "")
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "dtype": "bfloat16", "channels": C_, "unit": "ms per call",
           "clocks_before": clocks(), "shapes": []}
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for label, B, side, inner in BLOCKS:
            if args.skip_1024 and side == 128:
                continue
            r = block_shape(B, side, args.rounds, inner, g)
            r.update(label=label, batch=B, n=side * side, inner=inner)
            res["shapes"].append(r)
            print(f"{label:22s} off {r['off']['median_ms']:9.3f} ms  on {r['on']['median_ms']:9.3f} ms  off/on {r['off_over_on']:.3f}  kernel "
                  f"{r['kernel']['median_ms']:.3f} ms = {r['kernel']['tflops']:.1f} TFLOP/s  |on - off| / |off| = {r['rel_l2_on_vs_off']:.1e}", flush=True)
        for label, side, inner in DECODES:
            if args.skip_1024 and side == 128:
                continue
            r = decode_shape(side, args.rounds, inner, g)
            r.update(label=label, batch=1, n=side * side, inner=inner)
            res["shapes"].append(r)
            print(f"{label:22s} off {r['off']['median_ms']:9.3f} ms  on {r['on']['median_ms']:9.3f} ms  off/on {r['off_over_on']:.3f}  "
                  f"|on - off| / |off| = {r['rel_l2_on_vs_off']:.1e}", flush=True)
    res["clocks_after"] = clocks()
    errors = json.load(open(args.errors)) if args.errors and os.path.exists(args.errors) else []
    res["errors_vs_fp64"] = errors
    for path, text in ((args.out, json.dumps(res, indent=1)), (args.md, markdown(res, errors))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
