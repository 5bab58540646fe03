"""DDIM scheduler (host side) with the diffusers call surface the reference loops use
(``set_timesteps`` / ``timesteps`` / ``init_noise_sigma`` / ``scale_model_input`` / ``step(...).prev_sample`` /
``add_noise`` / ``alphas_cumprod``: reference ``models/pipelines.py:382, 409-410, 447, 629-631``; constructed
at ``generate.py:68-76``).  The schedule constants are host scalars; the per-step update itself runs on the
GPU in ``tg_step_epilogue`` (CFG + DDIM + frozen-mask blend fused), fed by ``coef_table()``.

diffusers==0.21.4 semantics (not under /root/reference -> parity unpinned, see oracle/ddim.py): betas =
linspace(sqrt(b0), sqrt(b1), T, fp32)**2, "leading" timestep spacing + steps_offset, eta = 0, no clipping.

Also here, with the same call surface: the Euler / Euler-ancestral pair of the SDXL flow (``tg_step_epilogue_sigma``) and the opt-in
DPM-Solver++ multistep sampler (``DPMSolverMultistepScheduler``, ``tg_step_epilogue_dpm``).
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import ops


def _device_step(launch, model_output, sample, return_dict):
    """The tail every ``step()`` here shares: fp32 contiguous copies, ``launch(model_output, out)`` updates ``out`` in place on the GPU, the result goes
    back to the sample's dtype as ``.prev_sample`` (or a 1-tuple)."""
    out = sample.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
    launch(model_output.detach().to(torch.float32).contiguous(), out)
    out = out.to(sample.dtype)
    return SimpleNamespace(prev_sample=out) if return_dict else (out,)


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 clip_sample=False, set_alpha_to_one=False, steps_offset=1, prediction_type="epsilon"):
        if clip_sample:
            raise ValueError("clip_sample=True is not supported (the reference uses clip_sample=False)")
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise ValueError(f"unknown beta_schedule {beta_schedule}")
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, steps_offset=steps_offset,
                                      prediction_type=prediction_type, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._coef_cache = {}

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ratio = T // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        self.timesteps = torch.from_numpy(ts)
        self._coef_cache = {}
        return self.timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _alphas(self, t):
        t = int(t)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return a_t, a_prev

    def coef_table(self, timesteps=None):
        """fp32 [n_steps, 4] = sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev) (fp32 math like diffusers)."""
        ts = self.timesteps if timesteps is None else timesteps
        rows = []
        for t in ts.tolist():
            a_t, a_prev = self._alphas(t)
            rows.append(torch.stack([a_t ** 0.5, (1 - a_t) ** 0.5, a_prev ** 0.5, (1 - a_prev) ** 0.5]))
        return torch.stack(rows).to(torch.float32).contiguous()

    def step(self, model_output, timestep, sample, eta=0.0, return_dict=True, **kw):
        """Drop-in ``scheduler.step``: one DDIM update on the GPU (no CFG, no mask)."""
        if eta != 0.0:
            raise ValueError("only eta = 0 (deterministic DDIM) is supported")
        dev = sample.device
        t = int(timestep)
        key = (t, dev)
        if key not in self._coef_cache:
            a_t, a_prev = self._alphas(t)
            coef = torch.stack([a_t ** 0.5, (1 - a_t) ** 0.5, a_prev ** 0.5, (1 - a_prev) ** 0.5]).reshape(1, 4)
            self._coef_cache[key] = (coef.to(dev, torch.float32), torch.zeros(1, dtype=torch.int32, device=dev))
        coef, idx = self._coef_cache[key]
        pred = 0 if self.config.prediction_type == "epsilon" else 1
        return _device_step(lambda m, out: ops.step_epilogue(m, out, 0.0, coef, idx, has_cfg=False, advance=False, prediction_type=pred),
                            model_output, sample, return_dict)

    def add_noise_coeffs(self, timesteps):
        a = self.alphas_cumprod[timesteps]
        return a ** 0.5, (1 - a) ** 0.5

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers ``add_noise``: ``sqrt(a_t) x0 + sqrt(1 - a_t) noise`` broadcast over a vector of timesteps, as the
        stage-2 path calls it with ALL 50 timesteps at once (reference models/pipelines.py:629-631: [1, C, h, w] latents
        -> [50, C, h, w]).  One ``tg_add_noise`` launch on the device; result in the dtype of ``original_samples``.

        Deliberate deviation: diffusers 0.21.4 casts ``alphas_cumprod`` to the sample dtype and rounds both products
        and their sum in half precision; here the two products and the sum are formed in fp32 and rounded ONCE to the sample
        dtype — at most one storage-dtype ulp away from the reference, closer to the exact value (the oracle,
        ``oracle/ddim.py::add_noise``, is fp32 as well; parity tests state 1 ulp / rel 2^-8 bf16, 2^-11 fp16 for this op)."""
        ts = torch.as_tensor(timesteps).reshape(-1).to("cpu", torch.long)
        ca, cb = self.add_noise_coeffs(ts)
        dev = original_samples.device
        x0 = original_samples.detach().to(torch.float32).contiguous()
        nz = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        if x0.shape[0] not in (1, ts.numel()) or nz.shape != x0.shape:
            raise ValueError("add_noise: samples / noise must have batch 1 (broadcast over the timesteps) or one row per timestep")
        if x0.shape[0] == 1:
            out = ops.add_noise(x0[0], nz[0], ca.to(dev, torch.float32), cb.to(dev, torch.float32))
        else:
            rows = [ops.add_noise(x0[i], nz[i], ca[i:i + 1].to(dev, torch.float32), cb[i:i + 1].to(dev, torch.float32))[0]
                    for i in range(ts.numel())]
            out = torch.stack(rows)
        return out.to(original_samples.dtype)


class _SigmaScheduler:
    """Host side of diffusers 0.21.4 ``EulerDiscreteScheduler`` / ``EulerAncestralDiscreteScheduler`` (epsilon prediction, linear sigma
    interpolation, no Karras sigmas): the SDXL base pipeline's scheduler and the T2I-Adapter pipeline's (reference ``models/pipelines.py:
    255-453`` stage 1, ``:592-857`` stage 2).  sigma = sqrt((1 - a) / a), interpolated at the timesteps, then 0 appended (fp32).

    The step index is the position of ``t`` in ``self.timesteps`` (``(timesteps == t).nonzero()``), so a loop that REPLACES ``timesteps``
    with a fast schedule (``models/pipelines.py:381-384``) still walks ``sigmas`` of the full table one row per step: step i uses
    ``sigmas[i]`` and ``sigmas[i + 1]``.  ``coef_table`` reproduces that for the device epilogue (``tg_step_epilogue_sigma``)."""
    order = 1
    ancestral = False

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="epsilon",
                 interpolation_type="linear", use_karras_sigmas=False, timestep_spacing="leading", steps_offset=1, trained_betas=None, **kw):
        name = type(self).__name__
        if prediction_type != "epsilon":
            raise NotImplementedError(f"{name}: prediction_type {prediction_type!r} is not supported (epsilon only, as the SDXL base checkpoint)")
        if use_karras_sigmas:
            raise NotImplementedError(f"{name}: Karras sigmas are not supported")
        if interpolation_type != "linear":
            raise NotImplementedError(f"{name}: interpolation_type {interpolation_type!r} is not supported (linear only)")
        if timestep_spacing not in ("leading", "linspace", "trailing"):
            raise NotImplementedError(f"{name}: timestep_spacing {timestep_spacing!r} is not supported (leading / linspace / trailing)")
        if trained_betas is not None:
            raise NotImplementedError(f"{name}: trained_betas are not supported")
        if kw:
            raise NotImplementedError(f"{name}: unsupported arguments {sorted(kw)}")
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise ValueError(f"unknown beta_schedule {beta_schedule}")
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                                      prediction_type=prediction_type, interpolation_type=interpolation_type, use_karras_sigmas=False,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset)
        sig = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.sigmas = torch.cat([sig.flip(0), torch.zeros(1)]).to(torch.float32)
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self.num_inference_steps = None

    @property
    def init_noise_sigma(self):
        m = self.sigmas.max()
        return m if self.config.timestep_spacing in ("linspace", "trailing") else (m ** 2 + 1) ** 0.5

    def set_timesteps(self, num_inference_steps, device=None):
        T, n, sp = self.config.num_train_timesteps, num_inference_steps, self.config.timestep_spacing
        if n > T:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = n
        if sp == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float64)[::-1].copy()
        elif sp == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float64) + self.config.steps_offset
        else:
            ts = np.arange(T, 0, -T / n).round().copy().astype(np.float64) - 1
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts.astype(np.float32))
        return self.timesteps

    def index_for_timestep(self, timestep, timesteps=None):
        ts = self.timesteps if timesteps is None else torch.as_tensor(timesteps)
        hit = (ts.to(torch.float32) == float(timestep)).nonzero()
        if hit.numel() != 1:
            raise ValueError(f"{type(self).__name__}: timestep {float(timestep)} occurs {hit.numel()} times in the schedule (needs exactly once)")
        return int(hit[0, 0])

    def model_input_divisor(self, index):
        """``sqrt(sigma_index^2 + 1)`` (fp32): ``scale_model_input`` divides by it"""
        return (self.sigmas[index] ** 2 + 1) ** 0.5

    def scale_model_input(self, sample, timestep):
        """``sample / sqrt(sigma^2 + 1)`` (host-side drop-in; the engine folds it into the step epilogue)"""
        return sample / self.model_input_divisor(self.index_for_timestep(timestep)).to(sample.device)

    def _update(self, k):
        """(eps weight, sigma_up) of step index k, fp32 tensor math like diffusers"""
        s, s_to = self.sigmas[k], self.sigmas[k + 1]
        if not self.ancestral:
            return s_to - s, torch.zeros((), dtype=torch.float32)
        s_up = (s_to ** 2 * (s ** 2 - s_to ** 2) / s ** 2) ** 0.5
        s_down = (s_to ** 2 - s_up ** 2) ** 0.5
        return s_down - s, s_up

    def coef_table(self, timesteps=None):
        """fp32 [n_steps, 4], one row per step of ``timesteps`` (default: ``self.timesteps``; a fast schedule is the replaced list):
        (eps weight, sigma_up, scale of the NEXT step's model input = 1 / sqrt(sigma_next^2 + 1), sigma_i).  Step i's index is its position
        in ``timesteps``; the scale of the last row is the one of sigma = sigmas[n] (never read: no model input follows the last step).  The
        scale is the fp32 reciprocal: PyTorch divides a tensor by a scalar as a multiply by it."""
        ts = self.timesteps if timesteps is None else torch.as_tensor(timesteps)
        n = int(ts.numel())
        if n + 1 > self.sigmas.numel():
            raise ValueError("coef_table: more timesteps than the sigma table has steps (call set_timesteps first)")
        rows = []
        for i, t in enumerate(ts.tolist()):
            k = self.index_for_timestep(t, ts)
            ce, su = self._update(k)
            rows.append(torch.stack([ce, su, 1.0 / self.model_input_divisor(min(k + 1, self.sigmas.numel() - 1)), self.sigmas[k]]))
        return torch.stack(rows).to(torch.float32).contiguous()

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, **kw):
        """Drop-in ``scheduler.step`` on the GPU (``tg_step_epilogue_sigma`` without CFG): the ancestral noise is
        ``randn(model_output.shape, dtype=model_output.dtype, generator=generator)``, as diffusers draws it."""
        if s_churn != 0.0 or s_noise != 1.0:
            raise NotImplementedError(f"{type(self).__name__}.step: s_churn / s_noise are not supported (the SDXL flow uses s_churn = 0)")
        dev = sample.device
        k = self.index_for_timestep(timestep)
        ce, su = self._update(k)
        coef = torch.stack([ce, su, torch.ones(()), self.sigmas[k]]).reshape(1, 4).to(dev, torch.float32)
        noise = torch.randn(model_output.shape, dtype=model_output.dtype, device=dev, generator=generator) if (self.ancestral or generator is not None) else None
        idx = torch.zeros(1, dtype=torch.int32, device=dev)
        return _device_step(lambda m, out: ops.step_epilogue_sigma(m, out, 0.0, coef, idx, has_cfg=False, advance=False,
                                                                   noise=noise.contiguous() if self.ancestral else None),
                            model_output, sample, return_dict)

    def add_noise(self, original_samples, noise, timesteps):
        """``x0 + sigma(t) * noise`` broadcast over a vector of timesteps (sigma looked up by the position of t in ``self.timesteps``): one
        ``tg_add_noise`` launch, fp32 math rounded once to the sample dtype (as ``DDIMScheduler.add_noise``)."""
        ts = torch.as_tensor(timesteps).reshape(-1).cpu()
        sig = torch.stack([self.sigmas[self.index_for_timestep(t)] for t in ts.tolist()]).to(torch.float32)
        dev = original_samples.device
        x0 = original_samples.detach().to(torch.float32).contiguous()
        nz = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        if x0.shape[0] not in (1, ts.numel()) or nz.shape != x0.shape:
            raise ValueError("add_noise: samples / noise must have batch 1 (broadcast over the timesteps) or one row per timestep")
        one = torch.ones_like(sig).to(dev)
        if x0.shape[0] == 1:
            out = ops.add_noise(x0[0], nz[0], one, sig.to(dev))
        else:
            out = torch.stack([ops.add_noise(x0[i], nz[i], one[i:i + 1], sig[i:i + 1].to(dev))[0] for i in range(ts.numel())])
        return out.to(original_samples.dtype)


class EulerDiscreteScheduler(_SigmaScheduler):
    """``x' = x + eps (sigma_{i+1} - sigma_i)`` (s_churn = 0): stage 1 of the SDXL flow"""
    ancestral = False


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """``x' = x + eps (sigma_down - sigma_i) + sigma_up noise_i``: stage 2 of the SDXL flow (the T2I-Adapter pipeline's scheduler)"""
    ancestral = True


class DPMSolverMultistepScheduler:
    """DPM-Solver++ multistep, data prediction, midpoint second-order update ("2M"): the scheduler the reference's loader offers as
    ``load_sd(use_dpm_multistep_scheduler=True)`` (``models/models.py:16, 36-37``).  A DIFFERENT sampler from the reference's default DDIM chain: one
    extra state tensor (the previous step's data prediction), no extra UNet call; typically walked with 20-25 steps.

    Schedule (all host math in fp64 on the fp32 ``alphas_cumprod`` DDIMScheduler has, rounded to fp32 once in ``coef_table``): a = alphas_cumprod,
    alpha_t = sqrt(a_t), sigma_t = sqrt(1 - a_t), lambda_t = ln alpha_t - ln sigma_t.  The walked list is s_0 > s_1 > ... > s_{n-1}; step i goes from
    s = s_i to t = s_{i+1}, the last one to t = 0 (a_0, not 1).  Data prediction: epsilon x0 = (x - sigma_s m) / alpha_s, v x0 = alpha_s x - sigma_s m.
    With h = lambda_t - lambda_s and E = -alpha_t expm1(-h):
        order 1:  x' = (sigma_t / sigma_s) x + E x0
        order 2:  x' = (sigma_t / sigma_s) x + E x0 + E / (2 r0) (x0 - x0_prev),   r0 = (lambda_s - lambda_{s_{i-1}}) / h
    Step 0 is first order; so is the last step when ``lower_order_final`` and n < 15; every other step has order ``solver_order``.

    The update itself runs on the GPU (``tg_step_epilogue_dpm``) from one ``coef_table`` row per step.  diffusers is not a dependency: this is the
    0.21.4 ``dpmsolver++`` / ``midpoint`` scheme restated; everything else that class offers is refused by name."""
    order = 1                                  # UNet evaluations per step (the diffusers attribute): a multistep solver needs one

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None, solver_order=2,
                 prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
                 solver_type="midpoint", lower_order_final=True, use_karras_sigmas=False, lambda_min_clipped=-float("inf"), variance_type=None,
                 timestep_spacing="linspace", steps_offset=0):
        name = type(self).__name__
        if trained_betas is not None:
            raise NotImplementedError(f"{name}: trained_betas are not supported")
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"{name}: algorithm_type {algorithm_type!r} is not supported (dpmsolver++ only)")
        if solver_type != "midpoint":
            raise NotImplementedError(f"{name}: solver_type {solver_type!r} is not supported (midpoint only)")
        if thresholding:
            raise NotImplementedError(f"{name}: thresholding is not supported")
        if use_karras_sigmas:
            raise NotImplementedError(f"{name}: use_karras_sigmas is not supported")
        if lambda_min_clipped != -float("inf"):
            raise NotImplementedError(f"{name}: lambda_min_clipped other than -inf is not supported")
        if variance_type is not None:
            raise NotImplementedError(f"{name}: variance_type {variance_type!r} is not supported (the model output carries no variance)")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"{name}: solver_order {solver_order!r} is not supported (1 or 2)")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"{name}: prediction_type {prediction_type!r} is not supported (epsilon or v_prediction)")
        if timestep_spacing not in ("linspace", "trailing"):
            raise NotImplementedError(f"{name}: timestep_spacing {timestep_spacing!r} is not supported (linspace or trailing; pass any other grid, "
                                      "DDIM's 'leading' one included, as set_timesteps(timesteps=...))")
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise ValueError(f"unknown beta_schedule {beta_schedule}")
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.init_noise_sigma = 1.0
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                                      trained_betas=None, solver_order=solver_order, prediction_type=prediction_type, thresholding=False,
                                      dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
                                      algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
                                      use_karras_sigmas=False, lambda_min_clipped=-float("inf"), variance_type=None,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(1, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._clear_state()

    _CONFIG_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "prediction_type")
    _OWN_KEYS = ("solver_order", "thresholding", "dynamic_thresholding_ratio", "sample_max_value", "algorithm_type", "solver_type", "lower_order_final",
                 "use_karras_sigmas", "lambda_min_clipped", "variance_type", "timestep_spacing", "steps_offset")

    @classmethod
    def from_config(cls, config, **overrides):
        """``DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`` (the idiom of reference ``models/models.py:48``): betas, prediction type and
        ``num_train_timesteps`` of any scheduler's config (a namespace or a dict).  The solver's own arguments (spacing included) are read only from a
        config that is this class's (one that carries ``solver_order``): a DDIM config's "leading" spacing describes DDIM's grid, not this one's."""
        get = config.get if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
        miss = object()
        keys = cls._CONFIG_KEYS + (cls._OWN_KEYS if get("solver_order", miss) is not miss else ())
        kw = {k: get(k, miss) for k in keys}
        kw = {k: v for k, v in kw.items() if v is not miss}
        kw.update(overrides)
        return cls(**kw)

    def _clear_state(self):
        self._x0_prev = None        # step(): the previous data prediction, fp32 on the device
        self._taken = 0             # step(): updates made since set_timesteps
        self._last_index = None
        self._dev_tables = {}

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        T = self.config.num_train_timesteps
        if (num_inference_steps is None) == (timesteps is None):
            raise ValueError("set_timesteps: pass exactly one of num_inference_steps and timesteps")
        if timesteps is not None:
            ts = np.asarray(torch.as_tensor(timesteps).cpu().numpy() if torch.is_tensor(timesteps) else timesteps)
            if ts.ndim != 1 or ts.size == 0 or not np.all(ts == np.round(ts)):
                raise ValueError("set_timesteps: timesteps must be a non-empty list of integers")
            ts = ts.astype(np.int64)
        else:
            n = int(num_inference_steps)
            if n < 1 or n > T - 1:
                raise ValueError("num_inference_steps must be in [1, num_train_timesteps - 1]")
            if self.config.timestep_spacing == "linspace":
                ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
            else:
                ts = (np.arange(T, 0, -T / n).round() - 1).astype(np.int64)
        if ts.min() < 1 or ts.max() > T - 1 or np.any(np.diff(ts) >= 0):
            raise ValueError(f"set_timesteps: timesteps must be strictly descending integers in [1, {T - 1}]")
        self.num_inference_steps = int(ts.size)
        self.timesteps = torch.from_numpy(ts)
        self._clear_state()
        return self.timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _order_of(self, i, n):
        if i == 0 or (i == n - 1 and self.config.lower_order_final and n < 15):
            return 1
        return self.config.solver_order

    def _rows64(self, ts, orders=None):
        """numpy fp64 [n, 8] rows (cx, ce, A, B, C, 0, 0, 0) of the walked list ``ts``"""
        a = self.alphas_cumprod.to(torch.float64).numpy()
        n = len(ts)
        if n == 0 or min(ts) < 0 or max(ts) >= len(a) or any(ts[i + 1] >= ts[i] for i in range(n - 1)):
            raise ValueError("coef_table: timesteps must be strictly descending integers of the training schedule")
        alpha, sigma = np.sqrt(a), np.sqrt(1.0 - a)
        lam = np.log(alpha) - np.log(sigma)
        rows = np.zeros((n, 8), dtype=np.float64)
        for i in range(n):
            s, t = ts[i], (ts[i + 1] if i + 1 < n else 0)
            h = lam[t] - lam[s]
            e = -alpha[t] * np.expm1(-h)
            if self.config.prediction_type == "epsilon":
                rows[i, 0], rows[i, 1] = 1.0 / alpha[s], -sigma[s] / alpha[s]
            else:
                rows[i, 0], rows[i, 1] = alpha[s], -sigma[s]
            rows[i, 2], rows[i, 3] = sigma[t] / sigma[s], e
            if (self._order_of(i, n) if orders is None else orders[i]) == 2:
                r0 = (lam[s] - lam[ts[i - 1]]) / h
                rows[i, 3], rows[i, 4] = e + e / (2.0 * r0), -e / (2.0 * r0)
        return rows

    def coef_table(self, timesteps=None, dtype=torch.float32):
        """[n_steps, 8] rows ``(cx, ce, A, B, C, 0, 0, 0)`` for the device epilogue: x0 = cx x + ce m, x' = A x + B x0 + C x0_prev; C is exactly 0 on
        first-order rows.  ``timesteps`` (default ``self.timesteps``) is the list actually WALKED: a fast schedule passes its subset, so t of step i is the
        next kept timestep, r0 follows the real lambda spacing and the order rules count the walked steps.  fp64 math; ``dtype=torch.float64`` keeps it."""
        ts = [int(t) for t in (self.timesteps if timesteps is None else torch.as_tensor(timesteps)).tolist()]
        return torch.from_numpy(self._rows64(ts)).to(dtype).contiguous()

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, **kw):
        """Drop-in ``scheduler.step`` on the GPU (``tg_step_epilogue_dpm`` without CFG or mask).  The multistep state lives here: the previous data
        prediction and the number of updates made, both cleared by ``set_timesteps``.  ``timestep`` is looked up in ``self.timesteps``; the steps must be
        walked in order, and the first call after ``set_timesteps`` is a first-order update wherever in the list it starts."""
        if kw:
            raise NotImplementedError(f"{type(self).__name__}.step: unsupported arguments {sorted(kw)}")
        dev = sample.device
        hit = (self.timesteps == int(timestep)).nonzero()
        if hit.numel() != 1:
            raise ValueError(f"{type(self).__name__}.step: timestep {int(timestep)} is not in the schedule (call set_timesteps first)")
        i = int(hit[0, 0])
        if self._taken and i != self._last_index + 1:
            raise ValueError(f"{type(self).__name__}.step: the multistep update needs the steps in order (step {self._last_index} was followed by {i}); "
                             "set_timesteps(...) starts a new chain")
        if dev not in self._dev_tables:
            ts = [int(t) for t in self.timesteps.tolist()]
            first = torch.from_numpy(self._rows64(ts, orders=[1] * len(ts))).to(dev, torch.float32).contiguous()
            self._dev_tables[dev] = (self.coef_table().to(dev), first, torch.arange(len(ts), dtype=torch.int32, device=dev))
        table, first, index = self._dev_tables[dev]
        if self._x0_prev is None or self._x0_prev.shape != sample.shape or self._x0_prev.device != dev:
            if self._taken:
                raise ValueError(f"{type(self).__name__}.step: the sample changed shape or device inside a chain")
            self._x0_prev = torch.empty(sample.shape, dtype=torch.float32, device=dev)
        res = _device_step(lambda m, out: ops.step_epilogue_dpm(m, out, self._x0_prev, 0.0, table if self._taken else first, index[i:i + 1],
                                                                has_cfg=False, advance=False),
                           model_output, sample, return_dict)
        self._taken += 1
        self._last_index = i
        return res

    add_noise_coeffs = DDIMScheduler.add_noise_coeffs
    add_noise = DDIMScheduler.add_noise          # sqrt(a_t) x0 + sqrt(1 - a_t) noise: the same forward process, one shared implementation
