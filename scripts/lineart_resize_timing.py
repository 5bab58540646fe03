"""The lineart detector's SDXL call (a 1024 x 1024 image at detect_resolution = 384, image_resolution = 1024) and the two resize kernels it adds
(profiles/lineart_resize_findings.md):

  (a) ``ops.cv_area_u8`` 1024^2 -> 384^2 and ``ops.cv_linear_u8`` 384^2 -> 1024^2 (bytes, "pt", both) per launch: device events around 200 back-to-back
      launches, 5 samples, median, against the algorithmic bytes (source read + destination write);
  (b) the detector call end to end from an ndarray, "pt" and "np" outputs: the SDXL call, the identity 512^2 call, and an eager torch arm for the SDXL
      call (``F.interpolate`` area / bilinear around the tests' torch.nn restatement in bf16 on the device: other bytes, timing only).

    python scripts/lineart_resize_timing.py [--rounds 15] [--out profiles/lineart_resize_timing.json]

Same process, the arms alternate, medians with quartiles; a host clock around calls that end in a device synchronisation.  Needs a GPU.  Seeded weights
(the test suite's), seeded images: the timings do not depend on the values."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
DTYPE = torch.bfloat16
HBM_TBS = 6.3                                                                      # the achievable rate the other findings files divide by


def _quart(v, unit="ms"):
    v = sorted(v)
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [v[0], statistics.median(v), v[-1]]
    return {f"median_{unit}": round(statistics.median(v), 4), f"q1_{unit}": round(q[0], 4), f"q3_{unit}": round(q[2], 4), "n": len(v)}


def _per_launch_us(fn, launches=200, samples=5):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    got = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        got.append(e0.elapsed_time(e1) * 1000.0 / launches)
    return got


def kernels(out):
    from theatergen_amd import ops
    g = torch.Generator().manual_seed(0)
    for B in (1, 4):
        src = torch.randint(0, 256, (B, 1024, 1024, 3), generator=g, dtype=torch.uint8).to(DEV)
        m = torch.randint(0, 256, (B, 384, 384, 1), generator=g, dtype=torch.uint8).expand(-1, -1, -1, 3).contiguous().to(DEV)
        x = torch.empty((B, 3, 384, 384), dtype=DTYPE, device=DEV)
        u8 = torch.empty((B, 1024, 1024, 3), dtype=torch.uint8, device=DEV)
        pt = torch.empty((B, 3, 1024, 1024), dtype=DTYPE, device=DEV)
        px_s, px_d = 1024 * 1024, 384 * 384
        cases = [("cv_area_u8 1024^2 -> 384^2, bf16 network input", lambda: ops.cv_area_u8(src, (384, 384), DTYPE, out=x), B * (3 * px_s + 6 * px_d)),
                 ("cv_linear_u8 384^2 -> 1024^2, invert, uint8 out", lambda: ops.cv_linear_u8(m, (1024, 1024), invert=True, u8_out=u8), B * (px_d + 3 * px_s)),
                 ("cv_linear_u8 384^2 -> 1024^2, invert, bf16 'pt' out", lambda: ops.cv_linear_u8(m, (1024, 1024), invert=True, u8_out=False, out=pt),
                  B * (px_d + 6 * px_s)),
                 ("cv_linear_u8 384^2 -> 1024^2, invert, both outs", lambda: ops.cv_linear_u8(m, (1024, 1024), invert=True, u8_out=u8, out=pt),
                  B * (px_d + 9 * px_s)),
                 ("image_from_u8 1024^2, bf16 (for scale: the same bytes as the 'pt' store, no arithmetic)", lambda: ops.image_from_u8(u8, DTYPE, 0, out=pt),
                  B * 9 * px_s)]
        for name, fn, nbytes in cases:
            us = _per_launch_us(fn)
            bound = nbytes / (HBM_TBS * 1e12) * 1e6
            rec = dict(_quart(us, "us"), algorithmic_bytes=nbytes, byte_bound_us=round(bound, 3), times_the_byte_bound=round(statistics.median(us) / bound, 1))
            out[f"kernel, batch {B}: {name}"] = rec
            print(json.dumps({f"batch {B}: {name}": rec}), flush=True)


def detector(rounds, out):
    from tests import lineart_reference as LR
    from theatergen_amd.lineart import LineartDetector, LineartGenerator
    seeded = LR.seeded_generator()
    native = LineartGenerator()
    native.load_state_dict(seeded.state_dict())
    det = LineartDetector(native.to(device=DEV, dtype=DTYPE).eval())
    ref_dev = LR.rounded_copy(seeded, DTYPE, DTYPE).to(DEV)
    xl, mid = LR.sample_image(1, 1024, 1024), LR.sample_image(2, 512, 512)

    def eager(arr, output_type):
        x = torch.from_numpy(arr).to(DEV).permute(2, 0, 1)[None].float()
        x = F.interpolate(x, size=(384, 384), mode="area") / 255.0
        line = ref_dev(x.to(DTYPE)).float()
        t = (line * 255.0).clamp(0, 255).floor()
        big = 255.0 - F.interpolate(t, size=(1024, 1024), mode="bilinear", align_corners=False).round()
        if output_type == "pt":
            return (big / 255.0).to(DTYPE).expand(-1, 3, -1, -1).contiguous()
        return big[0, 0].to(torch.uint8)[:, :, None].expand(-1, -1, 3).contiguous().cpu().numpy()

    for output_type in ("pt", "np"):
        arms = [(f"SDXL call, 1024^2 at 384 / 1024, native, '{output_type}'", lambda: det(xl, detect_resolution=384, image_resolution=1024, output_type=output_type)),
                (f"identity call, 512^2 at 512 / 512, native, '{output_type}'", lambda: det(mid, output_type=output_type)),
                (f"SDXL call, eager torch arm (other bytes), '{output_type}'", lambda: eager(xl, output_type))]
        with torch.no_grad():
            for _, fn in arms:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in arms}
            for r in range(rounds):
                for name, fn in (arms if r % 2 == 0 else arms[::-1]):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1000.0)
        for name, v in times.items():
            out["detector: " + name] = _quart(v)
            print(json.dumps({name: out["detector: " + name]}), flush=True)
    # the network alone at the two sizes, device events: what the resizes are added to
    with torch.no_grad():
        for side in (384, 512):
            x = torch.rand((1, 3, side, side), device=DEV).to(DTYPE)
            out[f"network alone, {side}^2, bf16, per forward"] = _quart([u / 1000.0 for u in _per_launch_us(lambda: det.model(x), launches=10, samples=rounds)])


if __name__ == "__main__":
    argv = sys.argv[1:]

    def opt(flag, default):
        if flag in argv:
            i = argv.index(flag)
            v = argv[i + 1]
            del argv[i:i + 2]
            return v
        return default
    dest, rounds = opt("--out", os.path.join(ROOT, "profiles", "lineart_resize_timing.json")), int(opt("--rounds", 15))
    if not torch.cuda.is_available():
        raise SystemExit("lineart_resize_timing.py needs a GPU: a timing taken without one says nothing")
    out = {}
    kernels(out)
    detector(rounds, out)
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
