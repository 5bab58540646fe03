"""Independent numpy-fp64 restatement of the DPM-Solver++ multistep sampler (data prediction, midpoint second-order update), in the DIRECT form:
lambda, h, r0, D0 / D1 — not the folded ``[cx, ce, A, B, C]`` row the device applies.  Shared by tests/test_dpm_solver_cpu.py and
tests/test_dpm_solver_gpu.py; imports nothing from the package under test.

    a = alphas_cumprod, alpha_t = sqrt(a_t), sigma_t = sqrt(1 - a_t), lambda_t = ln alpha_t - ln sigma_t
    walked list s_0 > s_1 > ... > s_{n-1}; step i: s = s_i -> t = s_{i+1}, after the last step t = 0
    D0 = x0(x, m) at s;  h = lambda_t - lambda_s
    order 1:  x' = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) D0
    order 2:  x' = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) D0 - 0.5 alpha_t (exp(-h) - 1) D1,   D1 = (D0 - D0_prev) / r0,
              r0 = (lambda_s - lambda_{s_{i-1}}) / h

Also the closed-form model the order tests run on: data ~ N(0, S^2) has the exact noise prediction eps*(x, t) = sigma_t x / (a_t S^2 + 1 - a_t) and the
exact probability-flow solution x_t = x_T sqrt((a_t S^2 + 1 - a_t) / (a_T S^2 + 1 - a_T)).
"""
import numpy as np


def alphas_cumprod(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear"):
    """the fp32 table every scheduler of the package starts from (fp32 linspace, square, fp32 running product), returned as fp64"""
    import torch
    if beta_schedule == "scaled_linear":
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    else:
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    return torch.cumprod(1.0 - betas, dim=0).double().numpy()


def timesteps(n, T=1000, spacing="linspace"):
    if spacing == "linspace":
        return np.linspace(0, T - 1, n + 1).round()[::-1][:-1].astype(np.int64)
    if spacing == "trailing":
        return (np.arange(T, 0, -T / n).round() - 1).astype(np.int64)
    if spacing == "leading":                                  # DDIM's grid (steps_offset = 1): handed to the solver as an explicit list
        return ((np.arange(0, n) * (T // n)).round()[::-1] + 1).astype(np.int64)
    raise ValueError(spacing)


def order_of(i, n, solver_order=2, lower_order_final=True):
    if i == 0:
        return 1
    if i == n - 1 and lower_order_final and n < 15:
        return 1
    return solver_order


def _ast(a, t):
    return np.sqrt(a[t]), np.sqrt(1.0 - a[t])


def data_prediction(a, s, x, m, prediction_type="epsilon"):
    al, sg = _ast(a, s)
    if prediction_type == "epsilon":
        return (x - sg * m) / al
    if prediction_type == "v_prediction":
        return al * x - sg * m
    raise ValueError(prediction_type)


def step(a, ts, i, x, m, d0_prev, prediction_type="epsilon", solver_order=2, lower_order_final=True):
    """one update of the walked list ``ts`` at position i: returns (x', D0).  ``d0_prev`` is only touched on a second-order step."""
    a = np.asarray(a, dtype=np.float64)
    x, m = np.asarray(x, dtype=np.float64), np.asarray(m, dtype=np.float64)
    n = len(ts)
    s, t = int(ts[i]), (int(ts[i + 1]) if i + 1 < n else 0)
    al_s, sg_s = _ast(a, s)
    al_t, sg_t = _ast(a, t)
    lam_s, lam_t = np.log(al_s) - np.log(sg_s), np.log(al_t) - np.log(sg_t)
    h = lam_t - lam_s
    d0 = data_prediction(a, s, x, m, prediction_type)
    out = (sg_t / sg_s) * x - al_t * (np.exp(-h) - 1.0) * d0
    if order_of(i, n, solver_order, lower_order_final) == 2:
        al_p, sg_p = _ast(a, int(ts[i - 1]))
        r0 = (lam_s - (np.log(al_p) - np.log(sg_p))) / h
        d1 = (d0 - np.asarray(d0_prev, dtype=np.float64)) / r0
        out = out - 0.5 * al_t * (np.exp(-h) - 1.0) * d1
    return out, d0


def chain(a, ts, x, model, prediction_type="epsilon", solver_order=2, lower_order_final=True):
    """walk the whole list; ``model(x, t, i)`` returns the model output at timestep t (step i).  Returns the list of states [x_0 .. x_n]."""
    xs, d0 = [np.asarray(x, dtype=np.float64)], None
    for i in range(len(ts)):
        nx, d0 = step(a, ts, i, xs[-1], model(xs[-1], int(ts[i]), i), d0, prediction_type, solver_order, lower_order_final)
        xs.append(nx)
    return xs


def ddim_step(a, s, t, x, eps):
    """closed-form deterministic DDIM update s -> t (epsilon prediction, eta = 0)"""
    al_s, sg_s = _ast(a, s)
    al_t, sg_t = _ast(a, t)
    return al_t * (x - sg_s * eps) / al_s + sg_t * eps


# ---- the closed-form model: data ~ N(0, S^2) ---------------------------------------------------------------------------------------------------------
def gaussian_eps(a, S):
    def model(x, t, i=None):
        return np.sqrt(1.0 - a[t]) * x / (a[t] * S * S + 1.0 - a[t])
    return model


def gaussian_exact(a, S, x_T, T_from, t_to=0):
    var = lambda t: a[t] * S * S + 1.0 - a[t]
    return x_T * np.sqrt(var(t_to) / var(T_from))
