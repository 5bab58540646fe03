"""DDIM scheduler (host side) with the diffusers call surface the reference loops use
(``set_timesteps`` / ``timesteps`` / ``init_noise_sigma`` / ``scale_model_input`` / ``step(...).prev_sample`` /
``add_noise`` / ``alphas_cumprod``: reference ``models/pipelines.py:382, 409-410, 447, 629-631``; constructed
at ``generate.py:68-76``).  The schedule constants are host scalars; the per-step update itself runs on the
GPU in ``tg_step_epilogue`` (CFG + DDIM + frozen-mask blend fused), fed by ``coef_table()``.

diffusers==0.21.4 semantics (not under /root/reference -> parity unpinned, see oracle/ddim.py): betas =
linspace(sqrt(b0), sqrt(b1), T, fp32)**2, "leading" timestep spacing + steps_offset, eta = 0, no clipping.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import ops


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
        out = sample.detach().to(torch.float32).clone()
        ops.step_epilogue(model_output.to(torch.float32).contiguous(), out, 0.0, coef, idx, has_cfg=False, advance=False,
                          prediction_type=0 if self.config.prediction_type == "epsilon" else 1)
        out = out.to(sample.dtype)
        if not return_dict:
            return (out,)
        return SimpleNamespace(prev_sample=out)

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
        out = sample.detach().to(torch.float32).clone()
        ops.step_epilogue_sigma(model_output.to(torch.float32).contiguous(), out, 0.0, coef, torch.zeros(1, dtype=torch.int32, device=dev),
                                has_cfg=False, advance=False, noise=noise.contiguous() if self.ancestral else None)
        out = out.to(sample.dtype)
        if not return_dict:
            return (out,)
        return SimpleNamespace(prev_sample=out)

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
