"""Kernel launches of GroundingDinoVisionFront and the memory-side traffic of tg_attention_swin, from rocprofv3 (profiles/grounding_dino_vision_findings.md).

Workloads (run each under the profiler, in a run of its own; Swin-T-sized synthetic weights, bf16, 800 x 800, batch 1):

    rocprofv3 --kernel-trace --output-format csv -d OUT/t1 -- python scripts/grounding_dino_vision_counters.py front 1
    rocprofv3 --kernel-trace --output-format csv -d OUT/t3 -- python scripts/grounding_dino_vision_counters.py front 3
    rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d OUT/fetch -- python scripts/grounding_dino_vision_counters.py attn
    rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d OUT/write -- python scripts/grounding_dino_vision_counters.py attn
    python scripts/grounding_dino_vision_counters.py summarise OUT profiles/grounding_dino_vision_counters.json

``front N``: N forwards + ``project`` with the same mask tensor; launches per steady-state forward = (kernels of the N = 3 run - kernels of the N = 1 run) / 2,
which cancels the weight upload and the first forward's position embeddings.  ``attn``: tg_attention_swin alone at the four stage shapes, shift 0 and 3,
on random q | k | v.  FETCH_SIZE / WRITE_SIZE are reported in KiB, FETCH_SIZE doubled on gfx950 (as scripts/pmc_traffic_summary.py); they count
memory-side L2 requests, Infinity-Cache hits included.
"""
import collections
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = [(200, 200, 3), (100, 100, 6), (50, 50, 12), (25, 25, 24)]


def front(n):
    import torch
    from transformers import GroundingDinoModel
    from scripts.grounding_dino_vision_timing import swin_t_config
    from theatergen_amd.grounding_dino import GroundingDinoVisionFront
    torch.manual_seed(0)
    model = GroundingDinoModel(swin_t_config()).eval()
    f = GroundingDinoVisionFront.from_state_dict(model.config, model.state_dict(), "cuda", torch.bfloat16)
    pv = torch.randn(1, 3, 800, 800, device="cuda", dtype=torch.bfloat16)
    mask = torch.ones(1, 800, 800, dtype=torch.long, device="cuda")
    for _ in range(n):
        feats, _ = f(pv, mask)
        f.project(feats)
    torch.cuda.synchronize()
    print("native op calls per forward:", f.op_calls // n)


def attn():
    import torch
    from theatergen_amd import ops
    torch.manual_seed(0)
    dt = torch.bfloat16
    for H, W, heads in STAGES:
        C, n = heads * 32, H * W
        qkv = torch.randn(n, 3 * C, device="cuda").to(dt)
        pads = [torch.randn(C, device="cuda").to(dt) for _ in range(3)]
        table = torch.randn(169, heads, device="cuda").to(dt)
        out = torch.empty(n, C, dtype=dt, device="cuda")
        for shift in (0, 3, 0, 3):
            ops.attention_swin(qkv, 3 * C, n * 3 * C, qkv[:, C:], 3 * C, n * 3 * C, qkv[:, 2 * C:], 3 * C, n * 3 * C, pads[0], pads[1], pads[2], table, 1, heads,
                               H, W, shift, 32 ** -0.5, out, C, n * C)
        torch.cuda.synchronize()


def _rows(d, suffix):
    for path in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        with open(path) as fh:
            yield from csv.DictReader(fh)


def summarise(out_dir, dest):
    counts = {}
    for tag in ("t1", "t3"):
        c = collections.Counter(r["Kernel_Name"] for r in _rows(os.path.join(out_dir, tag), "kernel_trace.csv"))
        counts[tag] = c
    per = {k: (counts["t3"][k] - counts["t1"].get(k, 0)) / 2 for k in counts["t3"]}
    per = {k: v for k, v in per.items() if v}
    res = {"front_kernel_launches_per_forward": sum(per.values()), "front_kernels_total": {t: sum(c.values()) for t, c in counts.items()},
           "front_launches_by_kernel": dict(sorted(((k[:120], v) for k, v in per.items()), key=lambda kv: -kv[1]))}
    # tg_attention_swin: one counter per pass, a dispatch's stage from its grid size (workgroups of 256 threads, four (window, head) pairs each)
    grid_of = {}
    for H, W, heads in STAGES:
        pairs = ((H + 6) // 7) * ((W + 6) // 7) * heads
        grid_of[(pairs + 3) // 4 * 256] = (f"{H}x{W}_h{heads}", 4 * H * W * heads * 32 * 2)
    traffic = {}
    for tag, name, factor in (("fetch", "FETCH_SIZE", 2048.0), ("write", "WRITE_SIZE", 1024.0)):
        for r in _rows(os.path.join(out_dir, tag), "counter_collection.csv"):
            if "attention_swin_kernel" not in r["Kernel_Name"] or r["Counter_Name"] != name:
                continue
            hit = grid_of.get(int(r["Grid_Size"]))
            if hit is None:
                continue
            t = traffic.setdefault(hit[0], {"algorithmic_bytes": hit[1], "FETCH_SIZE": [], "WRITE_SIZE": []})
            t[name].append(float(r["Counter_Value"]) * factor)
    for t in traffic.values():
        for name in ("FETCH_SIZE", "WRITE_SIZE"):
            v = t.pop(name)
            t[name.lower() + "_bytes_per_launch"] = sum(v) / len(v) if v else None
            t[name.lower() + "_dispatches"] = len(v)
        if t["fetch_size_bytes_per_launch"] is not None and t["write_size_bytes_per_launch"] is not None:
            t["moved_over_algorithmic"] = (t["fetch_size_bytes_per_launch"] + t["write_size_bytes_per_launch"]) / t["algorithmic_bytes"]
    res["attention_swin_traffic_batch1"] = traffic
    with open(dest, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "front_launches_by_kernel"}, indent=1))
    for k, v in list(res["front_launches_by_kernel"].items())[:25]:
        print(f"{v:7.1f}  {k}")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "front":
        front(int(sys.argv[2]))
    elif mode == "attn":
        attn()
    else:
        summarise(sys.argv[2], sys.argv[3])
