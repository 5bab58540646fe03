"""tests/golden/step_epilogue_parent.npz: inputs and outputs of the three step epilogues (tg_step_epilogue, tg_step_epilogue_sigma,
tg_step_epilogue_dpm) as the three hand-written kernels computed them on an MI355X, before they became one kernel body (csrc/tg_step.hip).

    THEATERGEN_HIP_LIB=<library of the commit to pin> python tests/golden/make_step_epilogue_parent.py

The stored file was recorded with the library of 36bf3ca, the last commit with ``step_epilogue_kernel`` in tg_elementwise.hip and
``step_epilogue_sigma_kernel`` / ``step_epilogue_dpm_kernel`` in tg_sdxl_flow.hip.  tests/test_step_epilogue_unify_gpu.py replays the stored inputs
through the current library and requires every output bit for bit.  Needs the GPU.  Regenerate only when a change of the step arithmetic is intended,
and say so in that change.

Every case walks ``STEPS`` consecutive calls on 2 x 4 x 5 x 3 latents (odd sizes: the img / pix index math and the per-image mask) with CFG scale
7.5 and ``frozen_steps = 2``, so the blend is on for two steps and off for the third.  One set of inputs serves all cases.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "step_epilogue_parent.npz")
N_IMG, C_, H, W = 2, 4, 5, 3
SHAPE = (N_IMG, C_, H, W)
STEPS, FROZEN_STEPS, G = 3, 2, 7.5
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}     # outputs are stored as their bit patterns

# entry: which epilogue; pred: DDIM prediction type; mask: None (no frozen latents), "shared" [h, w] or "per_image" [n_img, h, w]; mi: model_in dtype;
# noise: the ancestral table's dtype; plain: has_cfg=False, advance=False, no history (the scheduler.step() form), counter parked on row 1
CASES = {
    "ddim_eps_shared_bf16": dict(entry="ddim", pred=0, mask="shared", mi=torch.bfloat16),
    "ddim_v_per_image_f16": dict(entry="ddim", pred=1, mask="per_image", mi=torch.float16),
    "ddim_eps_per_image_f32": dict(entry="ddim", pred=0, mask="per_image", mi=torch.float32),
    "ddim_v_shared_f32": dict(entry="ddim", pred=1, mask="shared", mi=torch.float32),
    "ddim_plain": dict(entry="ddim", pred=0, mask=None, mi=None, plain=True),
    "euler_frozen_bf16": dict(entry="sigma", coef="coef_euler", noise=None, mask="shared", mi=torch.bfloat16),
    "euler_f32": dict(entry="sigma", coef="coef_euler", noise=None, mask=None, mi=torch.float32),
    "euler_a_bf16_noise_f32": dict(entry="sigma", coef="coef_euler_a", noise=torch.bfloat16, mask=None, mi=torch.float32),
    "euler_a_f32_noise_frozen_bf16": dict(entry="sigma", coef="coef_euler_a", noise=torch.float32, mask="per_image", mi=torch.bfloat16),
    # a 5-step table: rows 0, 1, 2 are first, second, second order; the state starts as NaN, which row 0 must not read
    "dpm_nan_state_frozen_bf16": dict(entry="dpm", mask="shared", mi=torch.bfloat16),
}
OUTPUTS = ("latents", "history", "model_in", "x0_prev", "counter")


def make_inputs():
    from theatergen_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    g = torch.Generator().manual_seed(20240)
    inp = {"noise_pred": torch.randn((STEPS, 2 * N_IMG, C_, H, W), generator=g), "latents": torch.randn(SHAPE, generator=g),
           "frozen": torch.randn((STEPS + 1,) + SHAPE, generator=g), "mask_shared": (torch.rand((H, W), generator=g) > 0.5).float(),
           "mask_per_image": (torch.rand((N_IMG, H, W), generator=g) > 0.5).float(), "noise": torch.randn((STEPS,) + SHAPE, generator=g)}
    inp["mask_shared"][0, 0], inp["mask_per_image"][1, 2, 1] = 0.25, 0.75            # fractional weights: both products of the blend matter
    inp["noise_bf16_bits"] = inp["noise"].to(torch.bfloat16).view(torch.int16)       # the table as an engine holds it, drawn in the model dtype
    for key, s, n in (("coef_ddim", DDIMScheduler(), STEPS), ("coef_euler", EulerDiscreteScheduler(), STEPS),
                      ("coef_euler_a", EulerAncestralDiscreteScheduler(), STEPS), ("coef_dpm", DPMSolverMultistepScheduler(), 5)):
        s.set_timesteps(n)
        inp[key] = s.coef_table()
    assert all(float(inp["coef_dpm"][i, 4]) != 0.0 for i in (1, 2)) and float(inp["coef_dpm"][0, 4]) == 0.0
    return inp


def replay(ops, name, inp, dev="cuda:0"):
    """the case's STEPS calls through ``ops`` -> {output: int tensor of bit patterns, stacked over the calls} (history: the buffer after the last)"""
    c = CASES[name]
    plain = c.get("plain", False)
    lat = inp["latents"].to(dev).clone()
    idx = torch.full((1,), 1 if plain else 0, dtype=torch.int32, device=dev)
    hist = None if plain else torch.zeros((STEPS + 1,) + SHAPE, device=dev)
    model_in = None if c["mi"] is None else torch.zeros((2 * N_IMG, C_, H, W), dtype=c["mi"], device=dev)
    frozen = mask = None
    if c["mask"] is not None:
        frozen, mask = inp["frozen"].to(dev), inp["mask_" + c["mask"]].to(dev)
    common = dict(has_cfg=not plain, advance=not plain, frozen=frozen, frozen_mask=mask, frozen_steps=FROZEN_STEPS if frozen is not None else 0,
                  history=hist, model_in=model_in)
    state = torch.full(SHAPE, float("nan"), device=dev) if c["entry"] == "dpm" else None
    noise = {None: None, torch.float32: inp["noise"], torch.bfloat16: inp["noise_bf16_bits"].view(torch.bfloat16)}[c.get("noise")]
    noise = None if noise is None else noise.to(dev)
    out = {k: [] for k in OUTPUTS}
    for i in range(STEPS):
        m = inp["noise_pred"][i].to(dev)
        m = m[:N_IMG].contiguous() if plain else m
        if c["entry"] == "ddim":
            ops.step_epilogue(m, lat, G, inp["coef_ddim"].to(dev), idx, prediction_type=c["pred"], **common)
        elif c["entry"] == "sigma":
            ops.step_epilogue_sigma(m, lat, G, inp[c["coef"]].to(dev), idx, noise=noise, **common)
        else:
            ops.step_epilogue_dpm(m, lat, state, G, inp["coef_dpm"].to(dev), idx, **common)
        torch.cuda.synchronize()
        out["latents"].append(lat.clone())
        out["counter"].append(idx.clone())
        if model_in is not None:
            out["model_in"].append(model_in.clone())
        if state is not None:
            out["x0_prev"].append(state.clone())
    if hist is not None:
        out["history"].append(hist)
    return {k: torch.stack(v).view(_BITS.get(v[0].dtype, v[0].dtype)).cpu() for k, v in out.items() if v}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from theatergen_amd import _lib, ops
    inp = make_inputs()
    arrays = {"in/" + k: v.numpy() for k, v in inp.items()}
    for name in CASES:
        for k, v in replay(ops, name, inp).items():
            arrays[f"{name}/{k}"] = v.numpy()
    np.savez_compressed(PATH, **arrays)
    print(f"{len(CASES)} cases, {len(arrays)} arrays, {os.path.getsize(PATH)} bytes from {_lib.LIB_PATH}")
