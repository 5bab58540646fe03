"""Reverse pass of attention at SD-1.5's inner levels (head dims 80 / 160): the wide recompute kernels (tg_attention_bwd_wide /
tg_attention_bwd_cross_wide, backward.FLASH_BWD_WIDE on) against the materialised per-(item, head) route (switch off).

One process, bf16, HIP events; after a warm-up of both routes the two are timed ALTERNATELY (off, on, off, on, ...), so both see the same clocks
and the same neighbours; the median and the spread of the rounds are printed.  Layers: ``backward.attention_input_grad`` at batch 2 x 8 heads,
(N 1024, d 80), (N 256, d 160), (N 64, d 160), self-attention and IP cross-attention (77 text + 4 image keys, scale 0.4, with the guidance
loss's ``extra``).  Iteration: one eager ``UNetInputGrad.loss_and_grad`` on config.sd15() at batch 1 (random weights).

    python scripts/attn_bwd_wide_timing.py [--rounds 7] [--out FILE.json]
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

from theatergen_amd import backward, config, weights  # noqa: E402
from theatergen_amd import guidance as G  # noqa: E402
from theatergen_amd.attention_processor import Attention, AttnProcessor, IPAttnProcessor  # noqa: E402
from theatergen_amd.unet import UNet2DConditionModel  # noqa: E402

DEV, DT = "cuda:0", torch.bfloat16
SHAPES = [(2, 1024, 8, 80), (2, 256, 8, 160), (2, 64, 8, 160)]          # (batch, N, heads, head dim): SD-1.5's 32^2 / 16^2 / 8^2 levels


def ev_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fn, rounds, inner):
    """-> {"off": [ms per round], "on": [...]}: both routes warmed up first, then off / on alternately"""
    out = {"off": [], "on": []}
    for wide in (False, True, False, True):
        backward.FLASH_BWD_WIDE = wide
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, wide in (("off", False), ("on", True)):
            backward.FLASH_BWD_WIDE = wide
            out[name].append(ev_ms(fn, inner))
    backward.FLASH_BWD_WIDE = False
    return out


def summary(t):
    r = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in t.items()}
    r["off_over_on"] = r["off"]["median_ms"] / r["on"]["median_ms"]
    return r


def count_launches(fn):
    """C-ABI calls of one invocation per route (every one passes ``_lib.check``; tg_attention_bwd_wide is 3 kernel launches, _cross_wide 2,
    every other call of these layers one)"""
    from theatergen_amd import _lib
    out, orig = {}, _lib.check
    for name, wide in (("off", False), ("on", True)):
        backward.FLASH_BWD_WIDE = wide
        n = [0]

        def counted(rc):
            n[0] += 1
            return orig(rc)
        _lib.check = counted
        try:
            fn()
        finally:
            _lib.check = orig
        out[name] = n[0]
    backward.FLASH_BWD_WIDE = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-unet", action="store_true")
    args = ap.parse_args()
    assert backward.FLASH_BWD, "TG_FLASH_BWD=0 switches every recompute route off"
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    except OSError:
        commit = ""
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "dtype": "bf16", "rounds": args.rounds, "layers": [], "unet": None}
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for (B, N, heads, d) in SHAPES:
            C, ctx, T = heads * d, 768, 4
            h = torch.randn(B * N, C, generator=g).to(DEV, DT)
            do = torch.randn(B * N, C, generator=g).to(DEV, DT)
            enc = (torch.randn(B, 77 + T, ctx, generator=g) * 0.5).to(DEV, DT)
            extra = (torch.randn(B, heads, N, 77, generator=g) * 0.2).to(DEV)
            sattn = Attention(query_dim=C, heads=heads, dim_head=d).to(DEV, DT)
            cattn = Attention(query_dim=C, cross_attention_dim=ctx, heads=heads, dim_head=d).to(DEV, DT)
            proc = IPAttnProcessor(hidden_size=C, cross_attention_dim=ctx, scale=0.4, num_tokens=T).to(DEV, DT)
            sproc = AttnProcessor()
            for kind, fn in (("self", lambda: backward.attention_input_grad(sattn, sproc, h, B, N, None, do, None)),
                             ("ip-cross", lambda: backward.attention_input_grad(cattn, proc, h, B, N, enc, do, extra))):
                r = summary(alternate(fn, args.rounds, 5))
                r.update(kind=kind, batch=B, n=N, heads=heads, head_dim=d, abi_calls=count_launches(fn))
                res["layers"].append(r)
                print(f"{kind:8s} B={B} N={N:5d} heads={heads} d={d:3d}: off {r['off']['median_ms']:8.3f} ms [{r['off']['min_ms']:.3f}, {r['off']['max_ms']:.3f}]   "
                      f"on {r['on']['median_ms']:8.3f} ms [{r['on']['min_ms']:.3f}, {r['on']['max_ms']:.3f}]   off/on {r['off_over_on']:.2f}   "
                      f"C-ABI calls {r['abi_calls']['off']} -> {r['abi_calls']['on']}", flush=True)
        if not args.no_unet:
            cfg = config.sd15()
            sd = weights.random_unet_state_dict(cfg, seed=0, device=DEV)
            unet = UNet2DConditionModel.from_state_dict(cfg, sd, device=DEV, dtype=DT, num_tokens=4, ip_scale=0.4)
            del sd
            lat = torch.randn(1, 4, 64, 64, generator=g).to(DEV, DT)
            enc = (torch.randn(1, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, DT)
            keys = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
            boxes = [[40 / 512, 150 / 512, 230 / 512, 450 / 512], [280 / 512, 150 / 512, 470 / 512, 450 / 512]]
            pos = [[2, 3], [7]]

            def loss_fn(sv):
                return G.compute_ca_lossv3(sv, boxes, pos, keys, return_grads=True, loss_scale=30.0, use_ratio_based_loss=True)
            eng = backward.UNetInputGrad(unet)
            grads = {}

            def it():
                grads[backward.FLASH_BWD_WIDE] = eng.loss_and_grad(lat, 741, enc, loss_fn, keys)[1]
            r = summary(alternate(it, max(3, args.rounds // 2), 1))
            a, b = grads[False].double(), grads[True].double()
            r["grad_rel_l2_on_vs_off"] = float((a - b).norm() / a.norm())
            res["unet"] = r
            print(f"sd15 UNetInputGrad.loss_and_grad, batch 1, eager: off {r['off']['median_ms']:8.2f} ms [{r['off']['min_ms']:.2f}, {r['off']['max_ms']:.2f}]   "
                  f"on {r['on']['median_ms']:8.2f} ms [{r['on']['min_ms']:.2f}, {r['on']['max_ms']:.2f}]   off/on {r['off_over_on']:.2f}   "
                  f"|grad_on - grad_off| / |grad_off| = {r['grad_rel_l2_on_vs_off']:.2e}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
