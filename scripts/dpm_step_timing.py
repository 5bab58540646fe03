"""What the DPM-Solver++ multistep step costs next to the DDIM step it can replace (``DPMSolverMultistepScheduler`` handed to ``DenoiseEngine``).

Three measurements, one process, each timed ALTERNATELY with its DDIM counterpart (ddim, dpm, ddim, dpm, ...) for ``--rounds`` rounds after warm-up, so both
see the same clocks and the same neighbours; median, min and max of the rounds are reported:

 (a) the step-epilogue launch alone at the flagship shape (8 x 4 x 64 x 64 latents, CFG, history row, bf16 model input, counter advanced): 50 launches
     captured in one graph per route, ms per replay / 50.  Bytes per element: DDIM reads u, c, x and writes x, the history row and two bf16 model inputs
     = 24; DPM also reads and rewrites the fp32 state = 32; Euler ancestral also reads its bf16 noise row = 26 (timed beside them by the same method,
     so all three instances of the one kernel body are covered).
 (b) ms per replayed step of the 8-image engine (SD-1.5 plan, seeded random weights, 50 steps each): the UNet is the same, only the epilogue differs.
 (c) the 8-image story: 50 DDIM steps against 25 DPM steps, time only.

Every section runs under an alarm of its own (``--limit`` seconds; the default action of the signal ends the process, also inside a blocked driver call), so a
hang ends the script instead of the next section starting on a device in an unknown state.

    python scripts/dpm_step_timing.py [--rounds 7] [--out profiles/dpm_step_timing.json] [--md profiles/dpm_solver_findings.md] [--parity FILE.jsonl]

``--parity``: the ``parity_metrics.jsonl`` the GPU tests append to (tests/parity_metrics.py); the oracle-loop rel-L2 of the DDIM engine
(tests/test_hotpath_gpu.py) and of the DPM engine (tests/test_dpm_solver_gpu.py) are copied from it into ``--md``.
"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from theatergen_amd import config, ops, weights  # noqa: E402
from theatergen_amd.pipelines import DenoiseEngine  # noqa: E402
from theatergen_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler  # noqa: E402
from theatergen_amd.unet import UNet2DConditionModel  # noqa: E402

DEV = "cuda:0"
DTYPE = torch.bfloat16
N_IMG, C_, HW = 8, 4, 64


class section:
    """``with section(name, seconds):`` — the process is ended by SIGALRM's default action if the block runs longer"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, int(seconds)

    def __enter__(self):
        print(f"[{self.name}] limit {self.seconds} s", flush=True)
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(routes, rounds, warm=2):
    for fn in routes.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed_ms(fn))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / statistics.median(v)}
            for k, v in t.items()}


def epilogue_launch(rounds, g, steps=50):
    shape = (N_IMG, C_, HW, HW)
    noise_pred = torch.randn((2 * N_IMG, C_, HW, HW), generator=g).to(DEV)
    ddim, dpm, euler_a = DDIMScheduler(), DPMSolverMultistepScheduler(), EulerAncestralDiscreteScheduler()
    for s in (ddim, dpm, euler_a):
        s.set_timesteps(steps)
    # every buffer a captured launch addresses stays referenced from `bufs` until the timing is over: a graph holds raw addresses, and entering
    # `torch.cuda.graph` empties the allocator's cache, which would hand a dropped tensor of an earlier capture back to the driver
    bufs = {}
    for name, coef in (("ddim", ddim.coef_table()), ("dpm", dpm.coef_table()), ("euler_a", euler_a.coef_table())):
        bufs[name] = dict(coef=coef.to(DEV), lat=torch.randn(shape, generator=g).to(DEV), state=torch.zeros(shape, device=DEV),
                          idx=torch.zeros(1, dtype=torch.int32, device=DEV), hist=torch.zeros((steps + 1,) + shape, device=DEV),
                          model_in=torch.zeros((2 * N_IMG, C_, HW, HW), dtype=DTYPE, device=DEV))
    bufs["euler_a"]["noise"] = torch.randn((steps,) + shape, generator=g).to(DEV, DTYPE)

    def chain(name):
        b = bufs[name]
        b["idx"].zero_()                                   # the counter walks rows 0 .. steps - 1 of the table and of the history
        for _ in range(steps):
            if name == "ddim":
                ops.step_epilogue(noise_pred, b["lat"], 7.5, b["coef"], b["idx"], advance=True, history=b["hist"], model_in=b["model_in"])
            elif name == "dpm":
                ops.step_epilogue_dpm(noise_pred, b["lat"], b["state"], 7.5, b["coef"], b["idx"], advance=True, history=b["hist"],
                                      model_in=b["model_in"])
            else:
                ops.step_epilogue_sigma(noise_pred, b["lat"], 7.5, b["coef"], b["idx"], advance=True, noise=b["noise"], history=b["hist"],
                                        model_in=b["model_in"])
    graphs = {}
    for name in bufs:
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain(name)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            chain(name)
        graphs[name] = gr
    r = alternate({k: gr.replay for k, gr in graphs.items()}, rounds, warm=3)
    for v in r.values():                                   # per launch (the counter reset of each replay is one 4-byte fill in 51 nodes)
        for k in ("median_ms", "min_ms", "max_ms"):
            v[k.replace("_ms", "_us_per_step")] = v[k] * 1e3 / steps
    r["dpm_over_ddim"] = r["dpm"]["median_ms"] / r["ddim"]["median_ms"]
    r["bytes_per_element"] = {"ddim": 24, "dpm": 32, "euler_a": 26}
    r["elements"] = N_IMG * C_ * HW * HW
    torch.cuda.synchronize()
    del graphs                                             # before the buffers they address
    return r


def engines(rounds, g):
    cfg = config.sd15()
    sd = weights.random_unet_state_dict(cfg, seed=0, device=DEV)
    unet = UNet2DConditionModel.from_state_dict(cfg, sd, device=DEV, dtype=DTYPE, num_tokens=4, ip_scale=0.4)
    del sd
    lat = torch.randn(N_IMG, C_, HW, HW, generator=g)
    enc = (torch.randn(2 * N_IMG, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, DTYPE)

    def engine(sched, steps):
        e = DenoiseEngine(unet, sched, n_img=N_IMG, height=512, width=512, num_inference_steps=steps, guidance_scale=7.5, enc_len=81)
        e.set_conditioning(enc)
        return e
    ddim50 = engine(DDIMScheduler(), 50)
    dpm50 = engine(DPMSolverMultistepScheduler(), 50)
    dpm25 = engine(DPMSolverMultistepScheduler(), 25)
    with torch.no_grad():
        per_step = alternate({"ddim": lambda: ddim50.run(lat), "dpm": lambda: dpm50.run(lat)}, rounds, warm=1)
        for v in per_step.values():
            for k in ("median_ms", "min_ms", "max_ms"):
                v[k.replace("_ms", "_ms_per_step")] = v[k] / 50
        per_step["dpm_over_ddim"] = per_step["dpm"]["median_ms"] / per_step["ddim"]["median_ms"]
        story = alternate({"ddim_50_steps": lambda: ddim50.run(lat), "dpm_25_steps": lambda: dpm25.run(lat)}, rounds, warm=1)
        story["ddim_over_dpm"] = story["ddim_50_steps"]["median_ms"] / story["dpm_25_steps"]["median_ms"]
        finite = bool(torch.isfinite(dpm25.run(lat)[-1]).all())
    return per_step, story, finite


def parity_rows(path):
    """the last bf16 / fp16 rel-L2 of each engine's oracle-loop comparison in the tests' log (tests/parity_metrics.py)"""
    want = {"denoise loop graph=True": "DDIM engine, 5 steps (tests/test_hotpath_gpu.py)",
            "dpm denoise loop vs oracle torch.bfloat16": "DPM engine, 5 steps, bf16 (tests/test_dpm_solver_gpu.py)",
            "dpm denoise loop vs oracle torch.float16": "DPM engine, 5 steps, fp16 (tests/test_dpm_solver_gpu.py)"}
    rows = {}
    for line in open(path):
        try:
            e = json.loads(line)
        except ValueError:
            continue
        if e.get("what") in want:
            label = want[e["what"]]
            if e["what"].startswith("denoise loop"):       # both dtypes log under one name: the stated tolerance tells them apart
                label = label.replace("5 steps", "5 steps, " + ("bf16" if e["l2_tol"] > 1e-2 else "fp16"))
            rows[label] = {"rel_l2": e["rel_l2"], "max_rel": e["max_rel"], "l2_tol": e["l2_tol"], "max_tol": e["max_tol"]}
    return rows


def fmt(v, key="median_ms", scale=1.0, digits=3):
    lo, hi = key.replace("median", "min"), key.replace("median", "max")
    return f"{v[key] * scale:.{digits}f} [{v[lo] * scale:.{digits}f}, {v[hi] * scale:.{digits}f}]"


def markdown(res):
    a, b, c = res["epilogue"], res["per_step"], res["story"]
    L = ["# DPM-Solver++ multistep on the device step path: what was measured", "",
         f"Device: {res['device']}; library built from `{res['commit']}` or later; {res['rounds']} alternating rounds per pair, HIP events, one process",
         "(`scripts/dpm_step_timing.py`).  Median [min, max] of the rounds.", "",
         "## (a) The epilogue launch alone", "",
         f"8 x 4 x 64 x 64 fp32 latents ({a['elements']} elements), CFG combine, history row, bf16 model input, counter advanced; 50 launches per graph replay.",
         "Bytes moved per element: 24 (DDIM) against 32 (DPM: the fp32 state is read and rewritten), so <= 1.33x is what the traffic predicts.", "",
         "| route | us per step | spread of the rounds |", "|---|---|---|",
         f"| `tg_step_epilogue` (DDIM) | {fmt(a['ddim'], 'median_us_per_step')} | {a['ddim']['spread']:.1%} |",
         f"| `tg_step_epilogue_dpm` | {fmt(a['dpm'], 'median_us_per_step')} | {a['dpm']['spread']:.1%} |",
         f"| `tg_step_epilogue_sigma` (Euler ancestral, bf16 noise row: 26 bytes) | {fmt(a['euler_a'], 'median_us_per_step')} | {a['euler_a']['spread']:.1%} |", "",
         f"DPM / DDIM = {a['dpm_over_ddim']:.3f}.  A step is the epilogue launch plus the one-thread counter launch that both routes make.",
         "At about 4 us for 3-4 MB both launches are set by launch latency rather than by HBM traffic, which is why the ratio stays under what the bytes predict.", "",
         "## (b) ms per replayed step, 8-image engine (SD-1.5 plan, bf16, 50 steps each)", "",
         "| scheduler | ms per step | ms per 50-step chain | spread |", "|---|---|---|---|",
         f"| DDIM | {fmt(b['ddim'], 'median_ms_per_step')} | {fmt(b['ddim'], digits=1)} | {b['ddim']['spread']:.2%} |",
         f"| DPM-Solver++ 2M | {fmt(b['dpm'], 'median_ms_per_step')} | {fmt(b['dpm'], digits=1)} | {b['dpm']['spread']:.2%} |", "",
         f"DPM / DDIM = {b['dpm_over_ddim']:.4f}: the UNet is identical, the target is equality within the spread.", "",
         "## (c) The 8-image story: 50 DDIM steps against 25 DPM steps", "",
         "| chain | ms | spread |", "|---|---|---|",
         f"| DDIM, 50 steps | {fmt(c['ddim_50_steps'], digits=1)} | {c['ddim_50_steps']['spread']:.2%} |",
         f"| DPM-Solver++ 2M, 25 steps | {fmt(c['dpm_25_steps'], digits=1)} | {c['dpm_25_steps']['spread']:.2%} |", "",
         f"DDIM 50 / DPM 25 = {c['ddim_over_dpm']:.3f}.  This is TIME ONLY.  Image quality at 25 steps is unmeasured here: it needs real weights, which are not",
         "in this tree.  On the closed-form Gaussian model of tests/dpm_solver_reference.py 2M at 25 steps is closer to the exact solution than DDIM at 50 for",
         "data std 2 and farther for data std 0.5, so no claim either way follows from it.", ""]
    if res.get("parity"):
        L += ["## Engine against the oracle loop (tiny plan, 2 images, 5 steps)", "",
              "rel-L2 and max|err| / max|ref| of the final latents against the free-running CPU loop (oracle UNet + the restated step), as the GPU tests log them.",
              "The DPM allowance is twice the DDIM one: a 2M row weights two UNet outputs by |B| + |C| <= 1 + 1 / r0 ~ 2 where DDIM weights one.", "",
              "| engine | rel-L2 | allowed | max-rel | allowed |", "|---|---|---|---|---|"]
        for k, v in sorted(res["parity"].items()):
            L.append(f"| {k} | {v['rel_l2']:.3e} | {v['l2_tol']:.1e} | {v['max_rel']:.3e} | {v['max_tol']:.1e} |")
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds each section may take before the process is ended")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--parity", default=None)
    ap.add_argument("--epilogue-only", action="store_true", help="section (a) alone, as JSON to --out: for many short runs interleaved between two builds")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("dpm_step_timing.py: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("dpm_step_timing.py: needs the GPU (a CPU run measures nothing)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    except OSError:
        commit = ""
    if not commit and os.path.exists(os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json")):
        commit = json.load(open(os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json"))).get("commit", "")
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "dtype": "bfloat16", "n_img": N_IMG}
    g = torch.Generator().manual_seed(0)
    with section("epilogue launch", args.limit):
        res["epilogue"] = epilogue_launch(args.rounds, g)
        print(json.dumps(res["epilogue"]), flush=True)
    if args.epilogue_only:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    with section("8-image engines", args.limit):
        res["per_step"], res["story"], res["dpm25_finite"] = engines(args.rounds, g)
        print(json.dumps({"per_step": res["per_step"], "story": res["story"]}), flush=True)
    res["parity"] = parity_rows(args.parity) if args.parity and os.path.exists(args.parity) else {}
    for path, text in ((args.out, json.dumps(res, indent=1)), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
