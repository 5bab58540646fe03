#!/usr/bin/env python
"""bench.py — 512 px, 50-step character images / second on synthetic CMIGBench 4-turn stories (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]   # N = 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W                    # one rank per GPU over RCCL

One "step" = one pass of the hot path over one batch of synthetic input = ONE 4-turn x 2-character story per
GPU: 8 character images, each a full 50-step DDIM chain with CFG (SD-1.5 plan, 512x512, IP-Adapter decoupled
cross-attention, 77 text + 4 image tokens), i.e. 50 CFG UNet calls of batch 2 x `char_batch` + the fused
CFG/DDIM step epilogue.  Inputs (latents, embeddings) are resident in HBM before the timed region.  Weak
scaling: every rank denoises its own dialogue per step (no data-path collective); RCCL only broadcasts the
shared conditioning once and all-gathers the final latents of each step.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps, writes --dump-outputs if given and prints the line.  With --full,
rank 0 at N = 1 then runs extra legs outside the timed region (--no-roofline / --no-cpu-baseline / --no-other-configs
drop one of them):
  roofline      — per-launch HIP-event timing of the dominant kernel family (MFMA GEMM / implicit-GEMM conv),
                  algorithmic FLOPs (2*M*N*K per launch) / measured time vs the 2.5 PFLOP/s dense bf16 MFMA peak
  cpu_baseline  — the CPU oracle (fp32 PyTorch restatement of the reference path, `oracle/`) timed on the host
                  cores for a bounded sample (CFG UNet calls), converted to char images / s
  other_configs — short runs of BASELINE.json configs[3] / configs[4] (--plan sd21 / sdxl) and the drop-in
                  char-batch-1 loops
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0        # dense bf16/fp16, MI355X_MICROARCH.md
SD15_FLOP_PER_CFG_CALL = 1.607e12  # 401.8 GMAC / sample, batch 2
PLAN_FLOP_PER_CFG_CALL = {"sd15": 1.607e12, "sd21": 4.30e12, "sdxl": 13.56e12}      # SURVEY.md §8(d), batch-2 CFG unit
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md (6.3 TB/s achievable)
DUMP_MAX_BYTES = 64 << 20        # --dump-outputs: what a comparison of two builds reads back


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--char-batch", type=int, default=8, help="character images denoised together (8 = one whole story)")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--streams", type=int, default=1,
                    help="denoise the character batch as this many independent sub-batches replayed concurrently on separate "
                         "HIP streams (same UNet weights).  2 is +2 %% images/s, but every launch is then a half-batch call "
                         "overlapping with the other chain, so per-kernel roofline / rocprof figures are no longer those of "
                         "one kernel owning the chip: the default line keeps 1")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak (default, the SCALE line): every rank denoises ITS OWN story per step — work grows with N.  strong: ONE "
                         "story per step in total, its 8 (turn, character) jobs split over the ranks (rank r: jobs r, r + N, ...; N must "
                         "divide 8), image tokens broadcast from rank 0, final latents all-gathered back into job order")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--plan", default="sd15", choices=["sd15", "sd21", "sdxl"],
                    help="sd15 = the north-star line (BASELINE.json configs[1]); sd21 = configs[3] (768px editing step with 4-box "
                         "guidance); sdxl = configs[4] (1024px, IP-Adapter-Plus, use --dtype fp16)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run the extra legs on rank 0 at N = 1 (outside the timed region): roofline, cpu_baseline "
                         "and other_configs.  Off by default: a plain run does only what its headline figure needs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline leg")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full: skip the short configs[3] (SD-2.1 768px editing step) / configs[4] (SDXL 1024px) legs")
    ap.add_argument("--cpu-calls", type=int, default=3)
    ap.add_argument("--cpu-loop-steps", type=int, default=0,
                    help="with --full: also run BASELINE.json configs[0] as an actual loop on the CPU oracle: SD-1.5 512x512, ONE character box, this "
                         "many DDIM steps (20 = the config; ~100 s at 64 threads), latents by the reference recipe; recorded as "
                         "cpu_baseline.config1_loop next to the bounded-sample extrapolation")
    ap.add_argument("--with-vae", action="store_true",
                    help="NOT the north-star line: also decode the 8 final latents of every story with the VAE (pipelines.py:468) "
                         "inside the timed region, i.e. end-to-end decoded images/s")
    ap.add_argument("--dry-launch", action="store_true",
                    help="launcher self-test (CPU, gloo): every rank joins the process group, takes part in the barrier / "
                         "max-over-ranks / gather plumbing and rank 0 prints a JSON line with the group's world size; no GPU work")
    ap.add_argument("--stage2", action="store_true",
                    help="NOT the north-star line: time the stage-2 step (ControlNet + IP-Adapter UNet, reference "
                         "pipelines.py:759-835) on the same stories instead of the stage-1 per-character step")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32): final_latents = "
                         "the final latents [jobs, 4, 64, 64] of that step's (turn, character) jobs, 8 per story, one story per GPU under "
                         "weak scaling (with --with-vae too: the decoded images are not written).  The inputs are seeded: two builds run with the "
                         "same arguments can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


def build_model(plan, dtype, device, num_tokens=4, scale=0.4):
    from theatergen_amd import config, weights
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.pipelines import SDPipe
    from theatergen_amd.unet import UNet2DConditionModel
    cfg = config.PLANS[plan]()
    # weights drawn ON the device from the seed (every rank of a multi-GPU launch gets the same values from its own generator: nothing to broadcast, no host RNG);
    # the module tree is built on the meta device (theatergen_amd.unet._load_on_meta): start-up ~45 s -> ~2 s per rank
    sd = weights.random_unet_state_dict(cfg, seed=0, device=device)
    unet = UNet2DConditionModel.from_state_dict(cfg, sd, device=device, dtype=dtype, num_tokens=num_tokens, ip_scale=scale)
    adapter = IPAdapter(SDPipe(unet), None, None, device, num_tokens=num_tokens)
    adapter.set_scale(scale)
    return cfg, sd, unet, adapter


def gemm_by_kernel(step_fn):
    """One eager invocation of ``step_fn`` with HIP events around every GEMM / conv launch (ops.gemm profiling mode) ->
    ({kernel label: {launches, ms, tflops}}, total ms of those launches, total algorithmic flop).  The per-plan ``roofline.by_kernel`` block."""
    from theatergen_amd import ops
    with torch.no_grad():
        step_fn()                                        # warm (eager): allocator, packed weights
        torch.cuda.synchronize()
        ops.gemm_profile_start()
        step_fn()
        torch.cuda.synchronize()
        recs = ops.gemm_profile_stop()
    if os.environ.get("TG_DUMP_RECS"):                   # dev: per-launch records (shape, kernel, ms) of this plan's step
        with open(os.environ["TG_DUMP_RECS"], "w") as f:
            json.dump(recs, f)
    by = {}
    for r in recs:
        k = by.setdefault(r["kernel"], dict(launches=0, ms=0.0, flops=0.0))
        k["launches"] += 1
        k["ms"] += r["ms"]
        k["flops"] += r["flops"]
    tot_ms = sum(v["ms"] for v in by.values())
    tot_fl = sum(v["flops"] for v in by.values())
    table = {k: {"launches": v["launches"], "ms": round(v["ms"], 3), "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1)}
             for k, v in sorted(by.items(), key=lambda kv: -kv[1]["ms"])}
    return table, tot_ms, tot_fl


def _family(label):
    """kernel TEMPLATE of a per-launch label: `gemm_glds_kernel<plain+ln,128x128>` -> `gemm_glds_kernel` (the sum over its instantiations
    decides which kernel is dominant: a template split into two symbols must not change the headline)"""
    return label.split("<", 1)[0]


def _sustained_peak():
    """what the matrix pipe sustains on RANDOM bf16 with every CU busy for seconds (profiles/*_mfma_sustained.json, scripts/r6_mfma_sustained.py: an MFMA-only
    loop with register-resident operands; the nominal 2.5 PFLOP/s assumes 2.4 GHz, under that load the part clocks ~1.83 GHz at ~1.28 kW) and the vendor
    GEMM's rate beside it on the same box -> (sustained TFLOP/s, vendor TFLOP/s, file) or (None, None, None)"""
    pdir = os.path.join(ROOT, "profiles")
    try:
        for fn in sorted((f for f in os.listdir(pdir) if f.endswith("_mfma_sustained.json")), reverse=True):
            with open(os.path.join(pdir, fn)) as f:
                arms = json.load(f)["arms"]
            rnd = [v["tflops_second_half"] for k, v in arms.items() if k.startswith("mfma_loop mode0") and k.endswith("random")]
            ven = [v["tflops_second_half"] for k, v in arms.items() if k.startswith("vendor matmul 8192x4096x4096 random")]
            if rnd:
                return max(rnd), (max(ven) if ven else None), f"profiles/{fn}"
    except (OSError, ValueError, KeyError):
        pass
    return None, None, None


def _library_build():
    try:
        with open(os.path.join(ROOT, "theatergen_amd", "lib", "build_info.json")) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def roofline_leg(unet, engine):
    """One eager CFG step with HIP events around every GEMM / conv / ATTENTION launch -> the dominant kernel TEMPLATE's achieved TFLOP/s
    (all instantiations of one template summed)."""
    from theatergen_amd import ops
    with torch.no_grad():
        engine._reset(engine.history[0].clone())
        engine._step()                                   # warm (eager)
        torch.cuda.synchronize()
        ops.gemm_profile_start()
        t0 = time.perf_counter()
        engine._step()
        torch.cuda.synchronize()
        eager_ms = (time.perf_counter() - t0) * 1e3
        recs = ops.gemm_profile_stop()
    if os.environ.get("TG_DUMP_RECS"):
        with open(os.environ["TG_DUMP_RECS"], "w") as f:
            json.dump(recs, f)
    by, fam = {}, {}
    for r in recs:
        for table, key in ((by, r["kernel"]), (fam, _family(r["kernel"]))):
            k = table.setdefault(key, dict(launches=0, ms=0.0, flops=0.0))
            k["launches"] += 1
            k["ms"] += r["ms"]
            k["flops"] += r["flops"]
    # Which template the headline `frac` describes is NOT decided by this run's timings (two templates within 1 % of each other made the
    # round-4 line flip between 0.21 and 0.38): it is the dominant template of the COMMITTED graph-replay trace of this
    # command (profiles/*_dominant_template.json, written by scripts/step_breakdown.py from a rocprofv3 kernel trace); its live numbers come
    # from this run's HIP events, and the runner-up's frac rides beside it when the trace has them within 5 %.
    live_name = max(fam.items(), key=lambda kv: kv[1]["ms"])[0]
    name, dom_src, runner = live_name, "this run's HIP events (no committed trace names a template this run launches)", None
    pdir0 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    for fn in sorted((f for f in os.listdir(pdir0) if f.endswith("_dominant_template.json")), reverse=True):
        try:
            with open(os.path.join(pdir0, fn)) as f:
                dj = json.load(f)
            if dj["template"] in fam:
                name, dom_src = dj["template"], f"profiles/{fn} <- {dj.get('source', 'rocprofv3 kernel trace')}"
                if dj.get("runner_up") in fam and dj.get("within_5pct"):
                    runner = dj["runner_up"]
                break
        except (OSError, KeyError, ValueError):
            continue
    top = fam[name]
    members = {k: v for k, v in by.items() if _family(k) == name}
    tot_ms = sum(v["ms"] for v in by.values())
    tot_fl = sum(v["flops"] for v in by.values())
    ach = top["flops"] / (top["ms"] * 1e-3) / 1e12
    # HBM traffic of the same kernel template from the PMC passes committed under profiles/ (rocprofv3 cannot run inside this
    # process): launch-weighted mean over the template's instantiations; the file names the library build it was collected on
    traffic, traffic_src, traffic_build = None, None, None
    pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    for fn in sorted((f for f in os.listdir(pdir) if f.endswith("_pmc_traffic.json")), reverse=True):   # newest round first
        try:
            with open(os.path.join(pdir, fn)) as f:
                pmc = json.load(f)
            rows = [v for k, v in pmc["kernels"].items() if _family(k) == name]
            if not rows:
                continue
            traffic = sum(v["traffic_bytes_per_launch"] * v["launches"] for v in rows) / sum(v["launches"] for v in rows)
            traffic_build = {"commit": pmc.get("commit", "n/a"), "sources_sha256": pmc.get("sources_sha256")}
            traffic_src = (f"profiles/{fn} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes over this bench command, gfx950 x2 "
                           f"fetch correction, launch-weighted over the template's instantiations; collected at commit "
                           f"{pmc.get('commit', 'n/a')}: rocprofv3 cannot run inside this process)")
            break
        except (OSError, KeyError, ValueError, ZeroDivisionError):
            continue
    # algorithmic bytes per launch: operands once + result once + the residual tensor where the layer adds one; a 3x3 conv reads its
    # input ONCE (M x C, not the M x 9C of the implicit GEMM); the fused GEGLU writes N / 2 columns; attention reads Q, K, V and writes O
    def alg_bytes(r):
        if "alg_bytes" in r:                                   # row-chain launches state theirs (several layers per launch)
            return r["alg_bytes"]
        if r.get("attention"):
            return 2.0 * (2 * r["M"] * r["N"] + 2 * r["batch"] * r["K"] * r["N"])          # Q + O, K + V (once per batch item)
        a_elems = r["M"] * (r["K"] // 9 if "conv" in r["kernel"] else r["K"])
        n_out = r.get("n_out", r["N"])
        return 2.0 * (a_elems + r["N"] * r["K"] + r["M"] * n_out + (r["M"] * n_out if r.get("has_res") else 0))
    alg = sum(alg_bytes(r) for r in recs if _family(r["kernel"]) == name) / top["launches"]
    avg_s = top["ms"] / top["launches"] * 1e-3
    # the other roof: HBM-side rate of the same launches, from the counters (traffic) and from the algorithmic bytes
    hbm = {"peak": HBM_PEAK_GBS, "unit": "GB/s", "algorithmic": round(alg / avg_s / 1e9, 1), "algorithmic_frac": round(alg / avg_s / 1e9 / HBM_PEAK_GBS, 4),
           "measured": round(traffic / avg_s / 1e9, 1) if traffic else None,
           "measured_frac": round(traffic / avg_s / 1e9 / HBM_PEAK_GBS, 4) if traffic else None,
           "traffic_over_algorithmic": round(traffic / alg, 3) if traffic else None}
    lib = _library_build()
    families = {k: {"launches": v["launches"], "ms": round(v["ms"], 3), "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1),
                    "frac": round(v["flops"] / (v["ms"] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)}
                for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])}
    # SHORT SCALARS FIRST (the driver's record keeps scalars and cuts strings / nested tables: VERDICT r4 weak 15b); tables and prose last
    sus, ven, sus_src = _sustained_peak()
    out = {"bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4),
           "traffic": round(traffic) if traffic else None, "kernel": name + "<*>",
           # the nominal peak assumes 2.4 GHz; on random operands the pipe sustains sustained_peak (committed probe), the vendor GEMM
           # vendor_gemm_tflops on the same box: frac_of_sustained is what the kernel leaves on the table at the clocks the part really grants
           "sustained_peak": sus, "frac_of_sustained": round(ach / sus, 4) if sus else None, "vendor_gemm_tflops": ven,
           "runner_up_kernel": (runner + "<*>") if runner else None,
           "runner_up_frac": families[runner]["frac"] if runner else None,
           "live_dominant_kernel": live_name + "<*>",
           "avg_launch_us": round(top["ms"] / top["launches"] * 1e3, 2), "launches_per_cfg_call": top["launches"],
           "algorithmic_bytes_per_launch_avg": round(alg), "traffic_over_algorithmic": hbm["traffic_over_algorithmic"],
           "hbm_frac_algorithmic": hbm["algorithmic_frac"], "hbm_frac_measured": hbm["measured_frac"],
           "all_kernels_tflops": round(tot_fl / (tot_ms * 1e-3) / 1e12, 2), "all_kernels_frac": round(tot_fl / (tot_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
           "library_sha256": lib.get("sources_sha256"), "library_commit": lib.get("commit"),
           "traffic_build_matches_library": (bool(traffic_build) and bool(lib) and traffic_build.get("sources_sha256") == lib.get("sources_sha256")) if traffic else None}
    for k, v in list(families.items())[:6]:                # per-template fractions as flat scalars: frac.gemm_glds_kernel, frac.conv_slab_kernel, ...
        out["frac." + k] = v["frac"]
    out.update({
            "sustained_peak_source": sus_src,
            "dominant_template_source": dom_src,
            "traffic_source": traffic_src, "traffic_collected_on_build": traffic_build,
            "library_build": lib, "hbm": hbm,
            "kernel_instantiations": sorted(members), "dominant_by": "kernel template, summed over instantiations",
            "cfg_batch_of_measured_call": 2 * engine.n_img,
            "flop_per_launch_avg": top["flops"] / top["launches"],
            "by_template": families,
            "all_timed_kernels": {"achieved": round(tot_fl / (tot_ms * 1e-3) / 1e12, 2), "ms_per_cfg_call": round(tot_ms, 3),
                                  "flop_per_cfg_call": tot_fl, "launches": len(recs), "includes": "GEMM / conv / attention / row-chain launches"},
            "by_kernel": {k: {"launches": v["launches"], "ms": round(v["ms"], 3), "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1)}
                          for k, v in sorted(by.items(), key=lambda kv: -kv[1]["ms"])}})
    out["executed_flop_per_step_call"] = tot_fl              # what ONE captured step really runs (the hoisted projections are not in it)
    return out


class ClockPowerSampler:
    """rocm-smi --showclocks --showpower sampled from a side thread while the timed region runs (the pool spreads 12 % for one
    build; the granted shader clock and the package power say which kind of box a line came from).  Host-side only: nothing is launched on the GPU."""

    def __init__(self, period=2.0):
        """period 2 s (round 5 sampled every 0.5 s: a rocm-smi process per sample takes driver locks and host CPU inside the timed region);
        the timed region of the default line is ~17 s, i.e. ~8 samples"""
        import threading
        self.period, self.samples, self._stop = period, [], threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        import re
        smi = "/opt/rocm/bin/rocm-smi"
        if not os.path.exists(smi):
            return
        while not self._stop.is_set():
            try:
                r = subprocess.run([smi, "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=10)
                d = json.loads(r.stdout)
                c = d.get(f"card{torch.cuda.current_device()}", d.get("card0", {}))
                sclk = pwr = None
                for k, v in c.items():
                    if "sclk" in k.lower():
                        m = re.search(r"(\d+)\s*Mhz", str(v), re.I)
                        if m:
                            sclk = int(m.group(1))
                    if "Graphics Package Power" in k:
                        try:
                            pwr = float(v)
                        except ValueError:
                            pass
                if sclk is not None:
                    self.samples.append((sclk, pwr))
            except (OSError, ValueError, subprocess.SubprocessError):
                pass
            self._stop.wait(self.period)

    def __enter__(self):
        self._t.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        self._t.join(timeout=15)

    def summary(self):
        import statistics
        load = [s for s in self.samples if s[1] is None or s[1] > 600.0] or self.samples
        if not load:
            return {"sclk_mhz_median": None, "power_w_median": None, "clock_power_samples": 0}
        pw = [p for _, p in load if p is not None]
        med = statistics.median([c for c, _ in load])
        return {"sclk_mhz_median": med, "power_w_median": statistics.median(pw) if pw else None, "clock_power_samples": len(load),
                "mfma_peak_at_granted_clock_tflops": round(MFMA_PEAK_TFLOPS * med / 2400.0, 1)}


def cpu_config1_loop(cfg, sd32, steps):
    """BASELINE.json configs[0] on the oracle: fp32, 1 box, `steps` DDIM steps with CFG 7.5, reference op order"""
    from oracle import ddim as oddim
    from oracle import latent_ops as ol
    from oracle import unet as ou
    from theatergen_amd import story
    lat = ol.get_input_latents_list(0, 123456789, 0.01, 512, 512, [story.box_xyxy(0)])[0][0]
    enc = torch.randn(2, 81, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(77)) * 0.5
    osch = oddim.DDIMSchedule()
    osch.set_timesteps(steps)
    t0 = time.perf_counter()
    with torch.no_grad():
        for t in osch.timesteps.tolist():
            lat = oddim.step_epilogue(osch, ou.unet_forward(cfg, sd32, torch.cat([lat] * 2), t, enc, ip_scale=0.4, num_tokens=4), t, lat, 7.5)
    dt = time.perf_counter() - t0
    assert torch.isfinite(lat).all()
    return {"ddim_steps": steps, "s_per_image": round(dt, 2), "s_per_step": round(dt / steps, 3), "images_per_s": round(1.0 / dt, 6)}


def cpu_baseline_leg(cfg, sd, dtype, n_calls, ddim_steps, loop_steps=0):
    """The oracle (CPU fp32 restatement of the reference op order) on the host cores: `n_calls` CFG UNet calls."""
    from oracle import unet as ou
    cores = min(os.cpu_count() or 1, 64)
    prev = torch.get_num_threads()
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, cfg.in_channels, 64, 64, generator=g)
    enc = torch.randn(2, 81, cfg.cross_attention_dim, generator=g) * 0.5
    sd32 = {k: v.float().cpu() for k, v in sd.items()}
    with torch.no_grad():
        ou.unet_forward(cfg, sd32, x, 981, enc, ip_scale=0.4, num_tokens=4)      # warm-up
        t0 = time.perf_counter()
        for i in range(n_calls):
            ou.unet_forward(cfg, sd32, x, 981 - 20 * i, enc, ip_scale=0.4, num_tokens=4)
        dt = (time.perf_counter() - t0) / n_calls
    loop = cpu_config1_loop(cfg, sd32, loop_steps) if loop_steps > 0 else None
    torch.set_num_threads(prev)
    out = {"value": round(1.0 / (dt * ddim_steps), 6), "unit": "char_images/s", "cores": cores, "kind": "port",
           "sample": f"{n_calls} CFG UNet calls (batch 2, SD-1.5 512x512, fp32, reference op order incl. unfused "
                     f"baddbmm/softmax/bmm attention) = {dt:.2f} s/call; x{ddim_steps} calls per char image",
           "s_per_cfg_call": round(dt, 3)}
    if loop is not None:
        out["config1_loop"] = loop
    return out


def self_launch(args):
    """`python bench.py --gpus N` with no torchrun environment: start the N ranks ourselves (one process per GPU, the
    same command line the driver uses) and hand over its exit code.  Fails loudly when fewer than N devices are visible."""
    if not args.dry_launch:
        n = torch.cuda.device_count()
        if n < args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} requested but only {n} GPU(s) are visible on this node")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this pool (RCCL needs it)
    raise SystemExit(subprocess.call(cmd, env=env))


def dry_launch(args, D, rank, world):
    """what the launcher test checks: the group really has `--gpus` members and the collectives of the timed region work"""
    D.init(backend="gloo")
    n = torch.distributed.get_world_size() if D.is_dist() else 1
    if n != args.gpus:
        raise SystemExit(f"bench.py: process group has {n} rank(s), --gpus {args.gpus}")
    D.barrier()
    worst = D.max_over_ranks(float(rank + 1), torch.device("cpu"))
    got = D.gather_latents(torch.full((2, 3), float(rank)))
    ok = worst == float(n) and got.shape[0] == 2 * n and [float(v) for v in got[::2, 0]] == [float(r) for r in range(n)]
    # the strong partition's round trip through the REAL group: rank r owns items r, r + n, ... of a 2 n-item story; all_gather + unshard
    # must give the items back in item order (theatergen_amd.distributed.run_story_strong)
    items = list(range(2 * n))
    mine = torch.tensor(D.shard(items, rank, n), dtype=torch.float32).reshape(-1, 1)
    back = D.unshard(D.gather_latents(mine), n) if n > 1 else mine
    unshard_ok = [int(v) for v in back[:, 0]] == items
    ok = ok and unshard_ok
    if rank == 0:
        rec = {"dry": True, "n_gpus": n, "collectives_ok": bool(ok)}
        if n > 2:
            rec.update({"unshard_of_shard_is_identity": bool(unshard_ok), "host_threads": torch.get_num_threads(),
                        "cpus_of_rank0": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None})
        print(json.dumps(rec), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    if not ok:
        raise SystemExit(1)


def _ev_ms(fn, iters=1):
    """HIP-event time of fn() on the current stream (ms per call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_sd21_editing(args):
    """BASELINE.json configs[3]: SD-2.1 plan 768x768 (latent 96x96, v-prediction, ctx 1024, 20 heads x 64 on the guidance
    layers), ONE edited image with 4 character boxes: per DDIM step the CFG UNet call with the attention-map side channel on
    the 4 guidance keys (cond half), compute_ca_lossv3 over the 4 boxes with its analytic d loss / d A (HIP reductions), and
    the fused CFG + DDIM + frozen-mask replace epilogue fed by the 4-object composed latents.  The UNet call (with the capture
    side channel) replays from a hipGraph; the guidance table is built on the host per call.  NOT the north-star line."""
    from theatergen_amd import guidance as G
    from theatergen_amd import latents as L
    from theatergen_amd import ops, story
    from theatergen_amd.scheduler import DDIMScheduler
    device = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    T = 4
    cfg, sd, unet, adapter = build_model("sd21", dtype, device, num_tokens=T)
    del sd
    steps = args.ddim_steps
    sch = DDIMScheduler(prediction_type="v_prediction")
    sch.set_timesteps(steps)
    hw = cfg.sample_size
    boxes = [story.box_xyxy(i) for i in range(4)]
    positions = [[2, 3], [7], [10, 11, 12], [15]]
    keys = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
    g = torch.Generator().manual_seed(40)
    enc = (torch.randn(2, 77 + T, cfg.cross_attention_dim, generator=g) * 0.5).to(device, dtype)
    # per-object stage-1 histories (synthetic) -> align + compose at 96x96 (utils/latents.py:168-240), timed separately
    lat_all = [torch.randn(steps + 1, 1, 4, hw, hw, generator=g).to(device) for _ in range(4)]
    masks = []
    for i, b in enumerate(boxes):
        m = torch.zeros(hw, hw, dtype=torch.bool)
        x0, y0, x1, y1 = [int(round(v * hw)) for v in b]
        m[y0 + 2:y1 - 2, x0 + 2:x1 - 2] = True
        masks.append(m)
    bg = torch.randn(1, 4, hw, hw, generator=g).to(device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    new_l, new_m, _ = L.align_with_bboxes(lat_all, masks, boxes)
    composed, fg_idx = L.compose_latents(adapter, None, new_l, new_m, steps, 1, 8 * hw, 8 * hw, latents_bg=bg)
    torch.cuda.synchronize()
    compose_ms = (time.perf_counter() - t0) * 1e3
    frozen_mask = (fg_idx != 0).to(torch.float32).reshape(1, hw, hw).contiguous()
    coef = sch.coef_table().to(device)
    step_idx = torch.zeros(1, dtype=torch.int32, device=device)
    t_table = sch.timesteps.to(device=device, dtype=torch.float32)
    from theatergen_amd.unet import DeviceSchedule
    dsch = DeviceSchedule(t_table, step_idx)
    latents = composed[0].clone()
    model_in = torch.cat([latents] * 2).to(dtype)
    parts = {"unet": 0.0, "guidance": 0.0, "epilogue": 0.0}
    map_bytes = 0

    # The CFG UNet call with its attention-map side channel is captured in a hipGraph (static buffers: model_in, the device-side
    # schedule, the saved maps live in the graph's pool); the guidance losses (host-built item table) and the step epilogue stay
    # eager launches.  Falls back to eager launches if the capture is refused.
    saved = {}
    kw = {"save_attn_to_dict": saved, "save_keys": keys, "return_cond_ca_only": True}
    out = {}

    def unet_call():
        out["np"] = unet(model_in, dsch, enc, cross_attention_kwargs=kw, return_dict=False, out_dtype=torch.float32)[0]

    def guid_call():
        out["loss"], out["grads"] = G.compute_ca_lossv3(saved, boxes, positions, keys, return_grads=True,
                                                        use_ratio_based_loss=False, fg_top_p=0.2, bg_top_p=0.2, fg_weight=1.0, bg_weight=4.0)

    def epi_call():
        ops.step_epilogue(out["np"], latents, 7.5, coef, step_idx, advance=True, prediction_type=1, frozen=composed,
                          frozen_mask=frozen_mask, frozen_steps=steps, history=None, model_in=model_in)

    def full_step():
        unet_call(); guid_call(); epi_call()
    graph = None
    with torch.no_grad():
        try:
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):
                full_step()                                   # warm-up: allocator, packed weights, K / V^T caches, guidance item table + masks
            torch.cuda.current_stream(device).wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                full_step()                                   # round 3: the WHOLE step (UNet + capture, guidance losses + d loss / d A, epilogue)
            graph = gr
            gr2 = torch.cuda.CUDAGraph()                      # the guidance call alone, captured: its device-side cost without the host's Python
            with torch.cuda.graph(gr2):
                guid_call()
            out["guid_graph_ms"] = _ev_ms(gr2.replay, iters=20)
        except Exception as e:                                # noqa: BLE001 - any capture failure means eager launches
            sys.stderr.write(f"[bench sd21] hipGraph capture of the UNet call refused ({type(e).__name__}: {e}); eager launches\n")
            torch.cuda.synchronize()
            saved.clear()

    def one_step(timed):
        nonlocal map_bytes
        if timed:                                             # per-part times: eager launches, HIP events around each part
            saved.clear()
            parts["unet"] += _ev_ms(unet_call)
            parts["guidance"] += _ev_ms(guid_call)
            parts["epilogue"] += _ev_ms(epi_call)
            map_bytes = sum(2 * v.numel() * 4 for v in saved.values())       # maps read once, gradients written once
        elif graph is not None:
            graph.replay()
        else:
            saved.clear()
            full_step()
        return out

    with torch.no_grad():
        for _ in range(args.warmup * 2 + 2):
            one_step(False)
        step_idx.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_timed = args.steps * steps
        for i in range(n_timed):
            if i % steps == 0:
                step_idx.zero_()
                latents.copy_(composed[0])
                model_in.copy_(torch.cat([latents] * 2))
            res = one_step(False)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        step_idx.zero_()
        for _ in range(5):
            one_step(True)
    assert torch.isfinite(res["np"]).all() and torch.isfinite(res["loss"])
    # one iteration of latent_backward_guidance (models/pipelines.py:62-128): forward to the last guidance key + the explicit input-gradient pass
    from theatergen_amd.backward import UNetInputGrad
    eng_g = UNetInputGrad(unet)

    def loss_fn(sv):
        return G.compute_ca_lossv3(sv, boxes, positions, keys, return_grads=True, loss_scale=30.0, use_ratio_based_loss=False, fg_top_p=0.2,
                                   bg_top_p=0.2, fg_weight=1.0, bg_weight=4.0)
    lat1 = composed[0].to(dtype)
    enc1 = enc[1:2].contiguous()
    with torch.no_grad():
        gl, gg = eng_g.loss_and_grad(lat1, 741, enc1, loss_fn, keys)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n_guide = int(os.environ.get("TG_GUIDE_ITERS", "3"))       # dev: more iterations for a kernel-level profile of the reverse pass
        for _ in range(n_guide):
            gl, gg = eng_g.loss_and_grad(lat1, 741, enc1, loss_fn, keys)
        torch.cuda.synchronize()
        guide_ms = (time.perf_counter() - t1) / n_guide * 1e3
    assert torch.isfinite(gg).all() and float(gg.abs().max()) > 0
    saved.clear()
    by_kernel, gemm_ms, gemm_fl = gemm_by_kernel(unet_call)
    # the same iteration captured into ONE hipGraph (what it costs on the GPU without the host's Python between ~3000 launches)
    guide_graph_ms, guide_graph_note = None, None
    try:
        from theatergen_amd.backward import GraphedInputGrad
        gig = GraphedInputGrad(unet, lat1, 741, enc1, loss_fn, keys, streams=8)
        gl2, gg2 = gig.run()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            gig.run(lat1)
        torch.cuda.synchronize()
        guide_graph_ms = (time.perf_counter() - t1) / 3 * 1e3
        guide_graph_note = "GraphedInputGrad (per-head chains, where a layer still has them, on 8 forked streams); " + (
            "bit-identical to the eager iteration" if torch.equal(gg2, gg) and torch.equal(gl2, gl) else
            f"max |graph - eager| = {float((gg2 - gg).abs().max()):.3e}")
        del gig
    except Exception as e:                                  # capture is a measurement aid here, never a reason to lose the line
        guide_graph_note = "capture failed: " + repr(e)[:160]
    ms_step = elapsed / n_timed * 1e3
    unet_ms = parts["unet"] / 5
    ach = PLAN_FLOP_PER_CFG_CALL["sd21"] / (unet_ms * 1e-3) / 1e12
    gb = map_bytes / (parts["guidance"] / 5 * 1e-3) / 1e9
    result = {
        "metric": "SD-2.1 768px editing step with 4-box attention-mask guidance: seconds per DDIM step", "value": round(ms_step * 1e-3, 5),
        "unit": "s/step", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step * steps, 2),
        "higher_is_better": False, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"BASELINE.json configs[3]: SD-2.1 plan 768x768, 1 image x 4 character boxes, {steps} DDIM steps (v-prediction), "
                               "CFG 7.5, IP 77+4 tokens; per step: CFG-batch-2 UNet with attention capture on 4 keys (12x12 / 24x24 x 20 heads "
                               "x 77 tokens), compute_ca_lossv3 + d loss / d A over 4 boxes, CFG + DDIM + frozen-mask replace; the whole step "
                               + ("replayed from ONE hipGraph" if graph is not None else "as eager launches") + " (per_step_ms: eager parts, HIP events)",
                   "plan": "sd21", "ddim_steps": steps, "boxes": 4},
        "images_per_s": round(1.0 / (ms_step * 1e-3 * steps), 4),
        "per_step_ms": {k: round(v / 5, 3) for k, v in parts.items()}, "compose_align_ms_once": round(compose_ms, 2),
        "latent_backward_guidance_iteration_ms": round(guide_ms, 1),
        "latent_backward_guidance_iteration_graph_ms": None if guide_graph_ms is None else round(guide_graph_ms, 1),
        "latent_backward_guidance_graph_note": guide_graph_note,
        "latent_backward_guidance_note": "one iteration = cond-only UNet forward to the last guidance key + compute_ca_lossv3 + d loss / d latents "
                                         "(explicit reverse pass; round 5: attention differentiated by recompute kernels, tg_attention_bwd / tg_attention_bwd_cross — no N x N tensor; TG_FLASH_BWD=0 = the materialised per-head path); "
                                         "host wall time, eager; the reference runs up to 5 per step for the first 10 steps (dead code in its shipped flow)",
        "roofline": {"bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4),
                     "traffic": None, "kernel": "whole CFG-batch-2 UNet call incl. attention capture (4.30 TFLOP algorithmic, SURVEY 8(d))",
                     "avg_launch_us": round(unet_ms * 1e3, 1),
                     "all_gemm_kernels": {"achieved": round(gemm_fl / (gemm_ms * 1e-3) / 1e12, 2), "ms_per_cfg_call": round(gemm_ms, 3),
                                          "note": "eager launches, HIP events per launch (event overhead ~2 us each)"},
                     "by_kernel": by_kernel},
        "guidance": {"bound": "latency", "achieved": round(gb, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gb / HBM_PEAK_GBS, 5),
                     "bytes_per_step": map_bytes, "ms": round(parts["guidance"] / 5, 3),
                     "ms_in_graph": round(out["guid_graph_ms"], 4) if "guid_graph_ms" in out else None,
                     "note": "4 maps x 20 heads x (144 | 576) x 77 fp32 read + gradients written (1.5 MB per step); `ms` = eager call incl. the host's Python "
                             "(loop over keys / boxes / positions), `ms_in_graph` = the same call replayed from a hipGraph: what it costs inside the captured step; "
                             "achieved / frac use `ms`; 23 MB per call is far below what fills HBM: the call is LATENCY-bound (launch + a 31-step radix select per term), the GB/s figure is informational"},
    }
    return result


def bench_sdxl(args):
    """BASELINE.json configs[4]: SDXL-base plan 1024x1024 (latent 128x128, text_time conditioning), IP-Adapter-Plus = 16 image
    tokens from the Perceiver Resampler, fp16, 30 DDIM steps, one image per step (CFG batch 2) on the hipGraph engine;
    the Resampler (cond + zero-image uncond, once per character) is timed separately.  NOT the north-star line."""
    from theatergen_amd.pipelines import DenoiseEngine
    from theatergen_amd.resampler import Resampler
    from theatergen_amd import weights as W
    device = torch.device("cuda", 0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    T = 16
    cfg, sd, unet, adapter = build_model("sdxl", dtype, device, num_tokens=T)
    del sd
    steps = 30 if args.ddim_steps == 50 else args.ddim_steps
    g = torch.Generator().manual_seed(50)
    kw = dict(dim=1280, depth=4, dim_head=64, heads=20, num_queries=T, embedding_dim=1280, output_dim=cfg.cross_attention_dim, ff_mult=4)
    rs = Resampler(**kw)
    rs.load_state_dict(W.random_resampler_state_dict(seed=401, **kw))
    rs = rs.to(device, dtype)
    clip_hidden = torch.randn(2, 257, 1280, generator=g).to(device, dtype)      # cond image + zero image (CLIP penultimate states)
    with torch.no_grad():
        for _ in range(3):
            tok = rs(clip_hidden)
        res_ms = _ev_ms(lambda: rs(clip_hidden), iters=20)
        rs.graphed(clip_hidden)                               # capture
        res_graph_ms = _ev_ms(lambda: rs.graphed(clip_hidden), iters=20)
    text = (torch.randn(2, 77, cfg.cross_attention_dim, generator=g) * 0.5).to(device, dtype)
    enc = torch.cat([text, torch.stack([tok[1], tok[0]])], dim=1).contiguous()    # negatives first: uncond tokens on row 0
    added = {"text_embeds": torch.randn(2, 1280, generator=g).to(device, dtype),
             "time_ids": torch.tensor([[1024., 1024., 0., 0., 1024., 1024.]] * 2, device=device)}
    eng = DenoiseEngine(unet, None, n_img=1, height=1024, width=1024, num_inference_steps=steps, guidance_scale=7.5, enc_len=77 + T)
    eng.set_conditioning(enc, added)
    lat = torch.randn(1, 4, 128, 128, generator=g)
    for _ in range(args.warmup):
        eng.run(lat)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        hist = eng.run(lat)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    assert torch.isfinite(hist[-1]).all()
    s_step = elapsed / (args.steps * steps)
    def one_eager_step():
        eng._reset(lat)                                   # step counter back to 0: the epilogue indexes its tables with it
        eng._step()
    by_kernel, gemm_ms, gemm_fl = gemm_by_kernel(one_eager_step)
    ach = PLAN_FLOP_PER_CFG_CALL["sdxl"] / s_step / 1e12
    result = {
        "metric": "SDXL 1024px IP-Adapter-Plus: seconds per DDIM step (CFG batch 2)", "value": round(s_step, 5), "unit": "s/step",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 2),
        "higher_is_better": False, "scaling": "weak", "vs_baseline": None, "dtype": "fp16" if dtype == torch.float16 else "bf16",
        "data": "synthetic",
        "config": {"workload": f"BASELINE.json configs[4]: SDXL-base plan 1024x1024 (latent 128x128, 2.6 B parameters, text_time conditioning), "
                               f"IP-Adapter-Plus 77+16 tokens scale 0.4, {steps} DDIM steps, CFG 7.5, one image per step, hipGraph engine",
                   "plan": "sdxl", "ddim_steps": steps},
        "images_per_s": round(1.0 / (s_step * steps), 4),
        "resampler_us_per_character": round(res_ms * 1e3, 1),
        "resampler_us_per_character_graph_replay": round(res_graph_ms * 1e3, 1),
        "resampler_note": "SDXL-Plus Resampler (depth 4, 20 heads x 64, 16 queries, 257 CLIP tokens), batch 2 = cond + zero-image uncond "
                          "(ip_adapter.py:347-359): 2 x 5.13 GMAC",
        "roofline": {"bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_PEAK_TFLOPS, 4),
                     "traffic": None, "kernel": "whole CFG-batch-2 UNet step (13.56 TFLOP algorithmic, SURVEY 8(d)) incl. the step epilogue",
                     "avg_launch_us": round(s_step * 1e6, 1),
                     "all_gemm_kernels": {"achieved": round(gemm_fl / (gemm_ms * 1e-3) / 1e12, 2), "ms_per_cfg_call": round(gemm_ms, 3),
                                          "note": "eager launches, HIP events per launch (event overhead ~2 us each)"},
                     "by_kernel": by_kernel},
    }
    return result


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy in float32, at most DUMP_MAX_BYTES in all"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {k: v.float().cpu().numpy() for k, v in arrays.items()}
    assert sum(a.nbytes for a in host.values()) <= DUMP_MAX_BYTES, {k: a.shape for k, a in host.items()}
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def main():
    args = parse()
    from theatergen_amd import distributed as D
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    if args.plan in ("sd21", "sdxl"):
        if args.gpus != 1:
            raise SystemExit("bench.py: --plan sd21 / sdxl are single-GPU lines")
        if args.dump_outputs:
            raise SystemExit("bench.py: --dump-outputs covers the story line (--plan sd15) only")
        torch.cuda.set_device(0)
        print(json.dumps(bench_sd21_editing(args) if args.plan == "sd21" else bench_sdxl(args)), flush=True)
        return
    rank, world, local = D.env_world()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    D.pin_host_threads(local, world)                      # N launch threads on one node: one CPU slice each (no-op at N = 1)
    if args.dry_launch:
        return dry_launch(args, D, rank, world)
    if local >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: LOCAL_RANK {local} but only {torch.cuda.device_count()} GPU(s) visible")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    D.init(device=device)
    if (torch.distributed.get_world_size() if D.is_dist() else 1) != args.gpus:
        raise SystemExit(f"bench.py: the process group has {torch.distributed.get_world_size() if D.is_dist() else 1} rank(s), "
                         f"--gpus {args.gpus}")
    world = args.gpus                                     # = the process group's size (checked above): what the line reports
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16

    from theatergen_amd import story
    from theatergen_amd.pipelines import DenoiseEngine
    T = 4
    cfg, sd, unet, adapter = build_model(args.plan, dtype, device, num_tokens=T)
    ctx = cfg.cross_attention_dim
    strong = args.scaling == "strong"
    jobs_per_story = 8
    if strong:
        if jobs_per_story % world or args.stage2 or args.with_vae or args.streams != 1:
            raise SystemExit("bench.py: --scaling strong needs --gpus in {1, 2, 4, 8} and none of --stage2 / --with-vae / --streams")
        args.char_batch = jobs_per_story // world            # a rank's share of the story is ONE CFG batch
    cb = args.char_batch
    assert jobs_per_story % cb == 0, "--char-batch must divide 8"
    controlnet = None
    if args.stage2:
        from theatergen_amd import weights
        from theatergen_amd.controlnet import ControlNetModel
        controlnet = ControlNetModel.from_state_dict(cfg, weights.random_controlnet_state_dict(cfg, seed=1), device=device,
                                                     dtype=dtype, num_tokens=T)
    ns = 1 if args.stage2 else max(1, args.streams)
    assert cb % ns == 0, "--streams must divide --char-batch"
    sub = cb // ns
    engines = [DenoiseEngine(unet, None, n_img=sub, height=512, width=512, num_inference_steps=args.ddim_steps,
                             guidance_scale=7.5, enc_len=77 + T, controlnet=controlnet, controlnet_enc_len=77) for _ in range(ns)]
    engine = engines[0]
    vae = None
    if args.with_vae:
        from theatergen_amd import weights
        from theatergen_amd.vae import AutoencoderKL, sd_vae_config
        vcfg = sd_vae_config()
        vae = AutoencoderKL.from_state_dict(vcfg, weights.random_vae_decoder_state_dict(vcfg, seed=2), device=device, dtype=dtype)
    control_image = None
    if args.stage2:
        gctl = torch.Generator().manual_seed(1234)
        control_image = torch.rand(1, 3, 512, 512, generator=gctl).repeat(2 * cb, 1, 1, 1).to(device=device, dtype=dtype)

    # shared conditioning: generated on rank 0, broadcast over RCCL (the only collective besides the final gather)
    shared = story.shared_conditioning(ctx, T, dtype, device)
    if rank != 0:
        for v in shared.values():
            v.zero_()
    D.broadcast_conditioning(shared, src=0)

    n_steps_total = args.warmup + args.steps
    # weak: every rank owns dialogues rank, rank + world, ...: one dialogue (story) per step.  strong: every rank works on the SAME
    # dialogue s and owns its jobs rank, rank + world, ... (theatergen_amd.distributed.run_story_strong)
    my_dialogues = list(range(n_steps_total)) if strong else [rank + world * s for s in range(n_steps_total)]
    prepared = []
    for d in my_dialogues:
        jobs = story.story_jobs(d)
        char_ids = sorted({j.char_id for j in jobs})
        img_tok = story.character_image_tokens(char_ids, ctx, T, dtype, device)
        if strong:
            # the per-character image tokens are the shared payload of this partitioning: rank 0's copy is the one everybody uses
            if rank != 0:
                img_tok.zero_()
            D.broadcast_conditioning({"image_tokens": img_tok}, src=0)
        cidx = {c: i for i, c in enumerate(char_ids)}
        batches = []
        mine = D.shard(jobs, rank, world) if strong else jobs
        for b0 in range(0, len(mine), cb):
            jb = mine[b0:b0 + cb]
            enc = story.job_conditioning(jb, shared, img_tok, cidx, ctx, dtype, device)
            lat = story.job_latents(jb, adapter)
            batches.append((enc, lat))
        prepared.append(batches)
    torch.cuda.synchronize()

    finals = torch.zeros((cb if strong else jobs_per_story, cfg.in_channels, 64, 64), dtype=torch.float32, device=device)

    def run_story(batches):
        for bi, (enc, lat) in enumerate(batches):
            if ns == 1:
                engine.set_conditioning(enc)
                if args.stage2:
                    engine.set_control(enc[:, :77], control_image, 1.0)
                hist = engine.run(lat)
                finals[bi * cb:(bi + 1) * cb].copy_(hist[-1])
            else:
                # enc rows: [negatives of the cb images ; positives of the cb images] -> per sub-batch slices
                lats = []
                for k, e in enumerate(engines):
                    rows = list(range(k * sub, (k + 1) * sub)) + list(range(cb + k * sub, cb + (k + 1) * sub))
                    e.set_conditioning(enc[rows])
                    lats.append(lat[k * sub:(k + 1) * sub])
                hists = DenoiseEngine.run_concurrent(engines, lats)
                for k, h in enumerate(hists):
                    finals[bi * cb + k * sub:bi * cb + (k + 1) * sub].copy_(h[-1])
        if vae is not None:
            with torch.no_grad():
                images_out = vae.decode_latents(finals)[0]
            assert images_out.shape[-1] == 512
        gathered = D.gather_latents(finals)
        return D.unshard(gathered, world) if strong and world > 1 else gathered          # strong: back into (turn, character) order

    for s in range(args.warmup):
        run_story(prepared[s])
    sampler = ClockPowerSampler() if rank == 0 else None
    D.barrier()
    torch.cuda.synchronize()
    if sampler is not None:
        sampler.__enter__()
    t0 = time.perf_counter()
    for s in range(args.warmup, n_steps_total):
        gathered = run_story(prepared[s])
    D.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if sampler is not None:
        sampler.__exit__()
    elapsed = D.max_over_ranks(elapsed, device)
    assert torch.isfinite(gathered).all()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"final_latents": gathered})

    images = jobs_per_story * args.steps * (1 if strong else world)
    value = images / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    cfg_calls = images * args.ddim_steps          # algorithmic units (batch-2 CFG UNet calls)
    result = {
        "metric": "512px 50-step char images/sec (node), CMIGBench 4-turn story",
        "value": round(value, 4), "unit": "char_images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 2), "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"SD-1.5 512x512, 4-turn story x 2 characters = 8 char images per step per GPU, {args.ddim_steps} DDIM "
                               f"steps, CFG 7.5, IP-Adapter 77+4 tokens scale 0.4, {args.dtype}, random-init weights",
                   "plan": args.plan, "char_batch": cb, "cfg_batch": 2 * cb, "streams": ns, "ddim_steps": args.ddim_steps,
                   "parallelism": (f"one story's 8 (turn, character) jobs split x{world} (RCCL broadcast of image tokens + all_gather only)"
                                   if strong else f"dialogue-sharded x{world} (RCCL broadcast + all_gather only)")},
        "whole_job_tflops": round(cfg_calls * SD15_FLOP_PER_CFG_CALL / elapsed / 1e12, 2),
        "whole_job_mfma_frac": round(cfg_calls * SD15_FLOP_PER_CFG_CALL / elapsed / 1e12 / (MFMA_PEAK_TFLOPS * world), 4),
    }
    if strong:
        result["config"]["workload"] = result["config"]["workload"].replace("8 char images per step per GPU", "8 char images per step in TOTAL")
    if args.with_vae:
        result["metric"] = result["metric"] + " + VAE decode of every image"
        result["config"]["workload"] += "; each final latent decoded to 512x512 by the SD VAE decoder (49.5 M params) inside the timed region"
    if args.stage2:
        result["metric"] = "512px 50-step stage-2 images/sec (ControlNet + IP-Adapter UNet per step)"
        result["unit"] = "images/s"
        result["config"]["workload"] += "; STAGE 2: SD-1.5 ControlNet (361 M params, control image 512x512, scale 1.0) runs every step before the UNet"
        result.pop("whole_job_tflops"); result.pop("whole_job_mfma_frac")
    if sampler is not None:
        result.update(sampler.summary())
    legs = args.full and rank == 0 and world == 1 and not args.stage2 and not args.with_vae
    if legs:
        if not args.no_roofline:
            result["roofline"] = roofline_leg(unet, engine)
            # flat scalars the driver's record keeps: the granted clock / power of THIS run and the whole-job fractions
            sus = result["roofline"].get("sustained_peak")
            flat = {"sclk_mhz_median": result.get("sclk_mhz_median"), "power_w_median": result.get("power_w_median"),
                    "whole_job_tflops": result.get("whole_job_tflops"), "whole_job_mfma_frac": result.get("whole_job_mfma_frac"),
                    "whole_job_frac_of_sustained": round(result["whole_job_tflops"] / sus, 4) if sus and result.get("whole_job_tflops") else None,
                    "clock_power_sample_period_s": sampler.period if sampler is not None else None}
            result["roofline"] = {**{k: v for k, v in list(result["roofline"].items())[:7]}, **flat, **{k: v for k, v in list(result["roofline"].items())[7:]}}
            if ns == 1 and cb == 8:
                # whole_job_tflops prices every image at the algorithmic 1.607 TFLOP per CFG call; the captured step does not re-run the
                # conditioning K / V projections or the timestep path (hoisted, bit-identical): what it EXECUTES is stated beside it
                ex = result["roofline"]["executed_flop_per_step_call"] * args.ddim_steps * args.steps
                result["whole_job_tflops_executed"] = round(ex / elapsed / 1e12, 2)
                result["whole_job_mfma_frac_executed"] = round(ex / elapsed / 1e12 / MFMA_PEAK_TFLOPS, 4)
        if not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline_leg(cfg, sd, dtype, args.cpu_calls, args.ddim_steps, args.cpu_loop_steps)
    if legs and not args.no_other_configs:
        # BASELINE.json configs[3] / configs[4], short runs of the same code as --plan sd21 / --plan sdxl, folded into the --full line
        # so that one bench call records them (they are parity-test configurations, not the metric)
        del engines, engine, unet, adapter, prepared
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        result["other_configs"] = other_configs_leg(args)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def drop_in_leg(args):
    """what an UNCHANGED caller gets.  (a) the reference's own stage-1 loop (models/pipelines.py:406-453) driving the HIP UNet through the
    diffusers call surface: one character at a time, CFG batch 2, an eager ``unet(...)`` call + ``scheduler.step`` + ``latents.cpu()`` per step;
    (b) the same character on ``DenoiseEngine`` at char-batch 1 (what ``theatergen_amd.pipelines.generate_semantic_guidance`` runs: one captured step
    replayed, no per-step host sync).  SD-1.5 512 x 512, ``args.ddim_steps`` steps; images/s and the fraction of the dense MFMA peak at 80.4 TFLOP per image."""
    from theatergen_amd import story
    from theatergen_amd.pipelines import DenoiseEngine
    from theatergen_amd.scheduler import DDIMScheduler
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    T = 4
    cfg, sd, unet, adapter = build_model("sd15", dtype, dev, num_tokens=T)
    ctx = cfg.cross_attention_dim
    shared = story.shared_conditioning(ctx, T, dtype, dev)
    jobs = story.story_jobs(0)[:5]                    # one warm-up character + four timed
    img_tok = story.character_image_tokens(sorted({j.char_id for j in jobs}), ctx, T, dtype, dev)
    cidx = {c: i for i, c in enumerate(sorted({j.char_id for j in jobs}))}
    steps = args.ddim_steps
    flop_per_image = SD15_FLOP_PER_CFG_CALL * steps
    out = {}

    def line(sec, n):
        return {"images_per_s": round(n / sec, 4), "ms_per_image": round(sec / n * 1e3, 1),
                "mfma_frac": round(flop_per_image * n / sec / 1e12 / MFMA_PEAK_TFLOPS, 4), "images_timed": n}
    # (a) reference-shaped eager loop, one character per pass, per-step D2H copy (the first job warms allocator / packed weights)
    sched = DDIMScheduler()
    sched.set_timesteps(steps)
    with torch.no_grad():
        for k, jb in enumerate(jobs):
            enc = story.job_conditioning([jb], shared, img_tok, cidx, ctx, dtype, dev)        # [2, 81, D]: negatives first
            latents = story.job_latents([jb], adapter).to(dev, dtype)
            if k == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            latents_all = [latents.cpu()]
            for t in sched.timesteps:
                x = sched.scale_model_input(torch.cat([latents] * 2), t)
                noise_pred = unet(x, t, encoder_hidden_states=enc, cross_attention_kwargs=None, return_dict=False)[0]
                u, c = noise_pred.chunk(2)
                latents = sched.step(u + 7.5 * (c - u), t, latents).prev_sample
                latents_all.append(latents.cpu())
        torch.cuda.synchronize()
        out["reference_shaped_eager_loop"] = line(time.perf_counter() - t0, len(jobs) - 1)
        out["reference_shaped_eager_loop"]["what"] = ("models/pipelines.py:406-453 as written: cat([latents]*2) -> unet(x, t, encoder_hidden_states=enc, "
                                                      "cross_attention_kwargs=None) -> CFG -> scheduler.step -> latents.cpu(), one character at a time")
        # (b) the engine at char-batch 1
        eng = DenoiseEngine(unet, None, n_img=1, height=512, width=512, num_inference_steps=steps, guidance_scale=7.5, enc_len=77 + T)
        for k, jb in enumerate(jobs):
            enc = story.job_conditioning([jb], shared, img_tok, cidx, ctx, dtype, dev)
            lat = story.job_latents([jb], adapter)
            if k == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            eng.set_conditioning(enc)
            hist = eng.run(lat)
            final = hist[-1].cpu()
        torch.cuda.synchronize()
        out["engine_char_batch_1"] = line(time.perf_counter() - t0, len(jobs) - 1)
        out["engine_char_batch_1"]["what"] = "DenoiseEngine(n_img=1): set_conditioning + 50 replays of one captured step + one D2H copy per character"
    assert torch.isfinite(final).all()
    return out


def other_configs_leg(args):
    import copy
    import gc
    out = {}
    try:
        out["drop_in char-batch 1"] = drop_in_leg(args)
    except Exception as e:                                    # noqa: BLE001 - a failure here must not cost the headline line
        out["drop_in char-batch 1"] = {"error": f"{type(e).__name__}: {e}"[:400]}
    gc.collect()
    torch.cuda.empty_cache()
    for key, plan, dtype, fn in (("configs[3] sd21 768px editing step", "sd21", "bf16", bench_sd21_editing),
                                 ("configs[4] sdxl 1024px ip-adapter-plus", "sdxl", "fp16", bench_sdxl)):
        a = copy.copy(args)
        a.plan, a.dtype, a.steps, a.warmup, a.ddim_steps = plan, dtype, 1, 1, (10 if plan == "sd21" else 6)
        try:
            r = fn(a)
            keep = ("metric", "value", "unit", "dtype", "images_per_s", "per_step_ms", "latent_backward_guidance_iteration_ms",
                    "latent_backward_guidance_iteration_graph_ms", "latent_backward_guidance_graph_note", "resampler_us_per_character", "resampler_us_per_character_graph_replay", "guidance")
            c = {k: r[k] for k in keep if k in r}
            c["workload"] = r["config"]["workload"]
            c["roofline"] = r["roofline"]
            out[key] = c
        except Exception as e:                                # noqa: BLE001 - a failure here must not cost the headline line
            out[key] = {"error": f"{type(e).__name__}: {e}"[:400]}
        gc.collect()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
