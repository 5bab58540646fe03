"""GPU: the one step-epilogue kernel body (csrc/tg_step.hip) computes what the three hand-written kernels it replaced computed, bit for bit.

 * ``test_bit_identical_to_the_parent_kernels``: tests/golden/step_epilogue_parent.npz holds inputs and the outputs the parent commit's library
   produced on an MI355X (tests/golden/make_step_epilogue_parent.py lists the cases: DDIM epsilon / v, shared / per-image mask, model_in bf16 / fp16 /
   fp32, the plain scheduler.step() form; Euler, Euler ancestral with a bf16 and an fp32 noise table, frozen on / off; DPM-Solver++ from a NaN state
   through one first-order and two second-order rows).  The stored inputs are replayed through the current library; latents, history, model_in, the DPM
   state and the step counter after every call must be ``torch.equal`` to the stored ones.
 * ``test_grid_stride_loop``: 2 x 4 x 264 x 256 = 540,672 elements is more than the 2048 x 256 threads a launch gets, so some threads take a second
   trip through the loop (the flagship SDXL shape sits exactly on the cap; nothing else in the suite goes over it).  One launch on both images must equal
   two launches on the single images.  Both sides are the new kernel: this guards the loop, the fixture guards the arithmetic.
"""
import numpy as np
import pytest
import torch

from tests.golden import make_step_epilogue_parent as gen

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 7.5


@pytest.fixture(scope="module")
def gold():
    z = np.load(gen.PATH)
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize("name", list(gen.CASES))
def test_bit_identical_to_the_parent_kernels(gold, name):
    from theatergen_amd import ops
    inp = {k[3:]: v for k, v in gold.items() if k.startswith("in/")}
    got = gen.replay(ops, name, inp, DEV)
    want = {k.split("/", 1)[1]: v for k, v in gold.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want), "the case writes the outputs the fixture holds"
    for k in ("latents", "x0_prev", "history"):
        if k in got:
            assert torch.isfinite(got[k].view(torch.float32)).all(), f"{name}: {k} is not finite"
    for k, v in want.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), \
            f"{name}: {k} differs from the parent's in {int((got[k] != v).sum())} of {v.numel()} values"


def _halves(t, dim):
    """copies of the two single-image slices of a tensor whose axis ``dim`` is the image axis (copies: a launch updates latents and state in place)"""
    return None if t is None else [t.narrow(dim, k, 1).clone(memory_format=torch.contiguous_format) for k in (0, 1)]


@pytest.mark.parametrize("entry", ["ddim", "sigma", "dpm"])
def test_grid_stride_loop(entry):
    from theatergen_amd import ops
    n, C, h, w, rows = 2, 4, 264, 256, 3
    assert n * C * h * w > 2048 * 256
    g = torch.Generator(device=DEV).manual_seed(7)

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(shape, generator=g, device=DEV).to(dtype)
    cfg = rnd(2, n, C, h, w)                                           # [uncond | cond][image]
    lat, frozen, mask = rnd(n, C, h, w), rnd(rows + 1, n, C, h, w), (torch.rand((h, w), generator=g, device=DEV) > 0.5).float()
    noise = rnd(rows, n, C, h, w, dtype=torch.bfloat16) if entry == "sigma" else None
    state = rnd(n, C, h, w) if entry == "dpm" else None
    z = gen.make_inputs()
    coef = z[{"ddim": "coef_ddim", "sigma": "coef_euler_a", "dpm": "coef_dpm"}[entry]].to(DEV)

    def launch(noise_pred, lat, frozen, noise, state):
        """row 1 of the table (a second-order one for DPM), blend on -> (latents, history row 2, model_in, state)"""
        k = lat.shape[0]
        idx = torch.ones(1, dtype=torch.int32, device=DEV)
        hist = torch.zeros((rows + 1, k, C, h, w), device=DEV)
        model_in = torch.zeros((2, k, C, h, w), dtype=torch.bfloat16, device=DEV)
        kw = dict(frozen=frozen, frozen_mask=mask, frozen_steps=2, history=hist, model_in=model_in)
        if entry == "ddim":
            ops.step_epilogue(noise_pred, lat, G, coef, idx, **kw)
        elif entry == "sigma":
            ops.step_epilogue_sigma(noise_pred, lat, G, coef, idx, noise=noise, **kw)
        else:
            ops.step_epilogue_dpm(noise_pred, lat, state, G, coef, idx, **kw)
        assert int(idx.item()) == 2 and not bool(hist[:2].any()) and not bool(hist[3:].any())
        return lat, hist[2], model_in, state

    parts = zip(_halves(cfg, 1), _halves(lat, 0), _halves(frozen, 1), _halves(noise, 1) or [None] * 2, _halves(state, 0) or [None] * 2)
    two = [launch(c.reshape(2, C, h, w), *rest) for c, *rest in parts]
    one = launch(cfg.reshape(2 * n, C, h, w), lat.clone(), frozen, noise, None if state is None else state.clone())
    assert not torch.equal(one[0], lat) and torch.isfinite(one[0]).all()
    for j, (what, dim) in enumerate((("latents", 0), ("history row", 0), ("model_in", 1), ("x0_prev", 0))):
        for k in (0, 1):
            assert one[j] is None or torch.equal(one[j].narrow(dim, k, 1), two[k][j]), f"{entry}: {what}, image {k}"
    assert torch.equal(one[2][0], one[2][1]), "both copies of the model input"
