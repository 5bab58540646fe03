"""CPU (no GPU): the host side of the DPM-Solver++ multistep sampler — timestep grids, refusals, the folded coefficient table against the direct-form
fp64 restatement (tests/dpm_solver_reference.py), the order rules, order 1 == DDIM, the solver's order on a model with a closed-form solution, and
the new C-ABI symbol's three declarations (header, binding, library)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import dpm_solver_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000


def _sched(**kw):
    from theatergen_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


def _table_chain(tab, x, outputs):
    """what the device does, in fp64: x0 = cx x + ce m, x' = A x + B x0 + C p (p only where C != 0)"""
    tab = tab.numpy()
    xs, p = [np.asarray(x, dtype=np.float64)], None
    for i, m in enumerate(outputs):
        cx, ce, A, B, C = tab[i, :5]
        x0 = cx * xs[-1] + ce * m
        nx = A * xs[-1] + B * x0
        if C != 0.0:
            nx = nx + C * p
        p = x0
        xs.append(nx)
    return xs


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("n", [4, 25, 50])
def test_timesteps(n):
    s = _sched()
    ts = s.set_timesteps(n)
    assert ts.dtype == torch.int64 and ts.numel() == n and s.num_inference_steps == n
    v = ts.tolist()
    assert all(a > b for a, b in zip(v, v[1:])), "strictly descending"
    assert v[0] == T - 1 and v[-1] == int(round((T - 1) / n))
    assert np.array_equal(ts.numpy(), R.timesteps(n))
    tr = _sched(timestep_spacing="trailing")
    assert np.array_equal(tr.set_timesteps(n).numpy(), R.timesteps(n, spacing="trailing"))
    assert np.array_equal(tr.timesteps.numpy(), np.arange(T, 0, -T / n).round() - 1)


def test_explicit_timesteps_and_surface():
    s = _sched()
    lead = R.timesteps(10, spacing="leading").tolist()
    ts = s.set_timesteps(timesteps=lead)
    assert ts.tolist() == lead and ts.dtype == torch.int64 and s.num_inference_steps == 10
    assert s.init_noise_sigma == 1.0 and s.order == 1 and s.config.solver_order == 2 and s.config.prediction_type == "epsilon"
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 5) is x
    for bad in ([10, 20], [20, 20, 10], [999, 0], [1000, 5], []):
        with pytest.raises(ValueError):
            s.set_timesteps(timesteps=bad)
    with pytest.raises(ValueError):
        s.set_timesteps(10, timesteps=lead)
    with pytest.raises(ValueError):
        s.set_timesteps()
    assert np.array_equal(s.alphas_cumprod.double().numpy(), R.alphas_cumprod())


def test_from_config():
    from types import SimpleNamespace
    from theatergen_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    d = DDIMScheduler(beta_schedule="linear", prediction_type="v_prediction")
    s = DPMSolverMultistepScheduler.from_config(d.config)
    assert s.config.prediction_type == "v_prediction" and s.config.beta_schedule == "linear" and s.config.timestep_spacing == "linspace"
    assert torch.equal(s.alphas_cumprod, d.alphas_cumprod)
    s2 = DPMSolverMultistepScheduler.from_config({"num_train_timesteps": 500, "beta_start": 0.0001, "beta_end": 0.02, "beta_schedule": "linear",
                                                  "prediction_type": "epsilon", "solver_order": 1, "timestep_spacing": "trailing"})
    assert s2.config.num_train_timesteps == 500 and s2.config.solver_order == 1 and s2.config.timestep_spacing == "trailing"
    assert s2.alphas_cumprod.numel() == 500
    s3 = DPMSolverMultistepScheduler.from_config(s2.config)
    assert vars(s3.config) == vars(s2.config)
    with pytest.raises(NotImplementedError, match="trained_betas"):
        DPMSolverMultistepScheduler.from_config(SimpleNamespace(trained_betas=[0.1, 0.2]))


@pytest.mark.parametrize("kw, word", [
    (dict(algorithm_type="dpmsolver"), "algorithm_type"), (dict(algorithm_type="sde-dpmsolver++"), "algorithm_type"),
    (dict(solver_type="heun"), "solver_type"), (dict(thresholding=True), "thresholding"), (dict(use_karras_sigmas=True), "use_karras_sigmas"),
    (dict(lambda_min_clipped=-5.1), "lambda_min_clipped"), (dict(variance_type="learned_range"), "variance_type"),
    (dict(trained_betas=[0.1, 0.2]), "trained_betas"), (dict(solver_order=3), "solver_order"), (dict(prediction_type="sample"), "prediction_type"),
    (dict(timestep_spacing="leading"), "timestep_spacing")])
def test_refusals(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _sched(**kw)


def _subset(s, n, after, rate):
    from theatergen_amd.schedule import get_fast_schedule
    s.set_timesteps(n)
    return get_fast_schedule(s.timesteps, after, rate)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("case", [4, 16, 25, "fast"])
def test_table_is_the_direct_form(pred, case):
    """fp64 chains: the folded row applied as A x + B x0 + C p == the restatement's lambda / h / r0 / D0 / D1 form, to 1e-12 relative"""
    s = _sched(prediction_type=pred)
    if case == "fast":
        ts = _subset(s, 16, 4, 2)
        assert 4 < len(ts) < 16
        tab = s.coef_table(ts, dtype=torch.float64)
    else:
        ts = s.set_timesteps(case)
        tab = s.coef_table(dtype=torch.float64)
    ts = [int(t) for t in torch.as_tensor(ts).tolist()]
    assert tab.dtype == torch.float64 and tab.shape == (len(ts), 8) and torch.all(tab[:, 5:] == 0)
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3, 5))
    outs = [rng.standard_normal((3, 5)) for _ in ts]
    a = R.alphas_cumprod()
    ref = R.chain(a, ts, x, lambda xx, t, i: outs[i], prediction_type=pred)
    got = _table_chain(tab, x, outs)
    for i in range(1, len(ts) + 1):
        assert _rel(got[i], ref[i]) <= 1e-12, (i, _rel(got[i], ref[i]))
    # the fp32 table is the fp64 one rounded once
    assert torch.equal(s.coef_table(ts), tab.to(torch.float32)) and s.coef_table(ts).dtype == torch.float32


def test_row_orders():
    s = _sched()
    s.set_timesteps(4)
    c = s.coef_table()[:, 4]
    assert float(c[0]) == 0.0 and float(c[1]) != 0.0 and float(c[2]) != 0.0 and float(c[3]) == 0.0
    s.set_timesteps(16)
    c = s.coef_table()[:, 4]
    assert float(c[0]) == 0.0 and all(float(v) != 0.0 for v in c[1:]), "n >= 15: the last step stays second order"
    s14 = _sched(lower_order_final=False)
    s14.set_timesteps(4)
    assert float(s14.coef_table()[3, 4]) != 0.0
    s1 = _sched(solver_order=1)
    s1.set_timesteps(16)
    assert torch.all(s1.coef_table()[:, 4] == 0)
    for i, n, want in [(0, 4, 1), (1, 4, 2), (3, 4, 1), (13, 14, 1), (14, 15, 2)]:
        assert R.order_of(i, n) == want and s._order_of(i, n) == want


@pytest.mark.parametrize("n", [10, 50])
def test_order_1_is_ddim(n):
    """solver_order = 1 on DDIM's leading grid == the closed-form DDIM update with final_alpha = a_0, to 1e-12"""
    s = _sched(solver_order=1)
    lead = R.timesteps(n, spacing="leading").tolist()
    s.set_timesteps(timesteps=lead)
    tab = s.coef_table(dtype=torch.float64)
    a = R.alphas_cumprod()
    rng = np.random.default_rng(3)
    x = rng.standard_normal(64)
    outs = [rng.standard_normal(64) for _ in lead]
    got = _table_chain(tab, x, outs)
    ref = x
    for i, t in enumerate(lead):
        ref = R.ddim_step(a, t, lead[i + 1] if i + 1 < n else 0, ref, outs[i])
        assert _rel(got[i + 1], ref) <= 1e-12, (i, _rel(got[i + 1], ref))


def _closed_form_error(n, S, solver_order):
    s = _sched(solver_order=solver_order)
    ts = [int(t) for t in s.set_timesteps(n).tolist()]
    a = R.alphas_cumprod()
    model = R.gaussian_eps(a, S)
    tab = s.coef_table(dtype=torch.float64).numpy()
    x, p = np.float64(1.3), None
    for i, t in enumerate(ts):
        cx, ce, A, B, C = tab[i, :5]
        x0 = cx * x + ce * model(x, t)
        nx = A * x + B * x0 + (C * p if C != 0.0 else 0.0)
        x, p = nx, x0
    return abs(x - R.gaussian_exact(a, S, 1.3, ts[0], 0))


@pytest.mark.parametrize("S", [1.0, 2.0])
def test_solver_order_on_the_closed_form_model(S):
    """data ~ N(0, S^2): exact eps and exact flow are known.  2M beats order 1 at every n, and its error falls strictly with n.  (S = 0.5 is left
    out on purpose: there the jump to t = 0 dominates and the inequality fails at n = 20 and 25.)"""
    e2 = {n: _closed_form_error(n, S, 2) for n in (10, 25, 50, 100)}
    e1 = {n: _closed_form_error(n, S, 1) for n in (10, 25, 50, 100)}
    print(f"S={S}: 2M {e2}  order 1 {e1}")
    for n in (10, 25, 50, 100):
        assert e2[n] < e1[n], (n, e2[n], e1[n])
    assert e2[25] > e2[50] > e2[100]
    # the restatement walks the same chain
    a = R.alphas_cumprod()
    ts = R.timesteps(25).tolist()
    xr = R.chain(a, ts, np.float64(1.3), R.gaussian_eps(a, S))[-1]
    assert abs(abs(xr - R.gaussian_exact(a, S, 1.3, ts[0], 0)) - e2[25]) <= 1e-12


def test_symbol_header_binding_and_library_agree():
    from theatergen_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    m = re.search(r"^int\s+tg_step_epilogue_dpm\s*\(([^;]*)\);", header, flags=re.M)
    assert m, "tg_step_epilogue_dpm is not declared in include/theatergen_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    names = [re.split(r"[\s\*]+", p)[-1] for p in params]
    assert names == ["noise_pred", "latents", "x0_prev", "n_img", "chw", "hw", "has_cfg", "guidance_scale", "coef", "step_idx", "advance", "frozen",
                     "frozen_mask", "mask_per_img", "frozen_steps", "history", "model_in", "model_in_dtype", "stream"]
    res, args = _lib.SIGNATURES["tg_step_epilogue_dpm"]
    assert res is _lib.i32 and len(args) == len(params)
    for p, a in zip(params, args):
        want = _lib.vp if "*" in p else _lib.f32 if p.startswith("float") else _lib.i32
        assert a is want, (p, a)
    assert re.search(r"#define\s+TG_ABI_VERSION\s+308\b", header) and _lib.ABI_VERSION == 308
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    assert h.tg_version() == 308 and len(h.tg_step_epilogue_dpm.argtypes) == len(params)
    # host-side argument validation, no launch: a missing state tensor is refused by name
    assert h.tg_step_epilogue_dpm(None, None, None, 1, 16, 4, 1, 7.5, None, None, 1, None, None, 0, 0, None, None, 0, None) == -1
    assert b"tg_step_epilogue_dpm" in h.tg_last_error()
    assert h.tg_step_epilogue_dpm(16, 32, None, 1, 16, 4, 1, 7.5, 48, 64, 1, None, None, 0, 0, None, None, 0, None) == -1
    assert h.tg_step_epilogue_dpm(16, 32, 32, 1, 16, 4, 1, 7.5, 48, 64, 1, None, None, 0, 0, None, None, 0, None) == -1
    assert b"x0_prev" in h.tg_last_error()
