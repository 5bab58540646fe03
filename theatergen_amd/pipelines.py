"""The two denoising loops that call the hot path, restructured for MI355X (reference ``models/pipelines.py``).

Reference loop bodies: stage 1 ``generate_semantic_guidance`` :406-453 (``cat([latents]*2)`` -> UNet -> CFG :441-442
-> ``scheduler.step`` :447 -> ``latents_all.append(latents.cpu())`` :449-453) and stage 2
``final_image_generation`` :742-835 (same + frozen-mask replace :833-834); IP embeds ``prepare_ip_embeds`` :860-950.

Here one step = ONE captured hipGraph (UNet CFG call + fused CFG/DDIM/mask epilogue): the timestep table, DDIM
coefficient table and step counter live on the device, the epilogue writes the next UNet input and the per-step
history row itself, so the 50-step loop is 50 graph replays with no host<->device traffic (the reference syncs
and copies latents to the CPU every step).  Any number of independent character images ride in the batch
dimension (CFG batch 2*n: all uncond rows first, then all cond rows = ``noise_pred.chunk(2)`` order).
"""
import os
import weakref
from collections import namedtuple

import torch

from . import ops
from .attention_processor import IPAttnProcessor, register_replay_stream, scale_vector, tensor_version, unregister_replay_stream
from .scheduler import DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
from .unet import DeviceSchedule


DEFAULT_GUIDANCE_ATTN_KEYS = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]     # reference pipelines.py:21


class SDPipe:
    """Minimal pipeline object: what ``IPAdapter`` and the latent utilities read from ``adapter.pipe``
    (``.unet``, ``.scheduler``, ``.controlnet``; reference ``ip_adapter.py:74``, ``utils/latents.py:261``)."""

    def __init__(self, unet, scheduler=None, controlnet=None):
        self.unet = unet
        self.scheduler = scheduler if scheduler is not None else DDIMScheduler(prediction_type=unet.config.prediction_type)
        self.controlnet = controlnet
        self.vae_scale_factor = 8

    def to(self, device, dtype=None):
        self.unet.to(device=device, dtype=dtype) if dtype is not None else self.unet.to(device)
        return self


def prepare_ip_embeds(prompt_embeds, negative_prompt_embeds, image_prompt_embeds, uncond_image_prompt_embeds):
    """Text + image tokens along the sequence axis, negatives first (reference pipelines.py:230-233, 369-370, 937-948).
    Inputs [n, 77, D] / [n, T, D]; returns [2n, 77+T, D] = [all negative rows ; all positive rows]."""
    pos = torch.cat([prompt_embeds, image_prompt_embeds.to(prompt_embeds.dtype)], dim=1)
    neg = torch.cat([negative_prompt_embeds, uncond_image_prompt_embeds.to(prompt_embeds.dtype)], dim=1)
    return torch.cat([neg, pos], dim=0)


_engine_ids = iter(range(1, 1 << 30))


# What the engine has to know about a sampler, resolved once per engine from the scheduler's class: the dtype of the walked timestep list, the extra
# device state its step keeps ("x0_prev": fp32 like the latents; "step_noise": [steps, n_img, C, h, w] in the model dtype; None), whether the model
# input is scaled (step 0 by ``in_div0`` in ``_reset``, the later ones by the epilogue) and the step-epilogue launch, called as
# ``epilogue(engine, noise_pred, **the frozen / history / model_in arguments every epilogue takes)``.
_Sampler = namedtuple("_Sampler", "kind t_dtype state scales_input epilogue")


def _ddim_epilogue(e, noise_pred, **kw):
    ops.step_epilogue(noise_pred, e.latents, e.g, e.coef, e.step_idx, prediction_type=e.pred_type, **kw)


def _sigma_epilogue(e, noise_pred, **kw):
    ops.step_epilogue_sigma(noise_pred, e.latents, e.g, e.coef, e.step_idx, noise=e.step_noise, **kw)


def _dpm_epilogue(e, noise_pred, **kw):
    ops.step_epilogue_dpm(noise_pred, e.latents, e.x0_prev, e.g, e.coef, e.step_idx, **kw)


# DDIM: the reference's own update; Euler / Euler ancestral (the SDXL flow): sigma-parameterised update, tg_step_epilogue_sigma; DPM-Solver++
# multistep (opt-in, models/models.py:36-37): tg_step_epilogue_dpm with one extra state tensor.  The first class the scheduler is an instance of wins.
_SAMPLERS = ((EulerAncestralDiscreteScheduler, _Sampler("euler_a", torch.float32, "step_noise", True, _sigma_epilogue)),
             (EulerDiscreteScheduler, _Sampler("euler", torch.float32, None, True, _sigma_epilogue)),
             (DPMSolverMultistepScheduler, _Sampler("dpm", torch.int64, "x0_prev", False, _dpm_epilogue)),
             (DDIMScheduler, _Sampler("ddim", torch.int64, None, False, _ddim_epilogue)))


class DenoiseEngine:
    """Batched CFG denoiser for ``n_img`` independent character images on one GPU.

    ``run()`` returns ``latents_all`` fp32 [steps+1, n_img, C, h, w] (row 0 = the input latents), the
    ``torch.stack(latents_all)`` of reference pipelines.py:488 for every image of the batch."""

    def __init__(self, unet, scheduler=None, n_img=1, height=512, width=512, num_inference_steps=50, guidance_scale=7.5,
                 enc_len=81, use_graph=True, controlnet=None, controlnet_enc_len=77, timesteps=None):
        """``timesteps`` (optional): a SUBSET of ``scheduler.set_timesteps(num_inference_steps)`` to walk instead of all of them — the reference's fast
        schedule (``utils/schedule.py:4-8`` applied at ``models/pipelines.py:383-384``); as in the reference the DDIM update of a kept step still jumps by
        the full schedule's stride (``prev_t = t - 1000 // num_inference_steps``).  A ``DPMSolverMultistepScheduler`` gets the subset as the walked list:
        each step goes to the next KEPT timestep and r0 follows the real lambda spacing."""
        self.unet = unet
        self.ws_slot = next(_engine_ids)      # private kernel scratch: engines may replay concurrently on different streams
        # stage 2 (reference pipelines.py:759-818): every step the ControlNet runs on the same model input with the TEXT
        # embeddings and the (step-invariant) control image; its residuals enter the UNet call
        self.controlnet = controlnet
        self.scheduler = scheduler if scheduler is not None else DDIMScheduler(prediction_type=unet.config.prediction_type)
        self.n_img = n_img
        self.h, self.w = height // 8, width // 8
        self.steps = num_inference_steps
        self.g = guidance_scale
        self.use_graph = use_graph
        dev, dt, cfg = unet.device, unet.dtype, unet.config
        self.dev, self.dt = dev, dt
        C = cfg.in_channels
        self.sampler = next((rec for cls, rec in _SAMPLERS if isinstance(self.scheduler, cls)), None)
        if self.sampler is None:
            raise TypeError(f"DenoiseEngine: unsupported scheduler {type(self.scheduler).__name__}; the step epilogues exist for theatergen_amd.scheduler."
                            "DDIMScheduler, EulerDiscreteScheduler, EulerAncestralDiscreteScheduler and DPMSolverMultistepScheduler")
        self.kind = self.sampler.kind
        self.scheduler.set_timesteps(num_inference_steps)
        self.timesteps = self.scheduler.timesteps.clone() if timesteps is None else torch.as_tensor(timesteps, dtype=self.sampler.t_dtype).clone()
        num_inference_steps = self.steps = int(self.timesteps.numel())
        self.t_table = self.timesteps.to(device=dev, dtype=torch.float32)
        self.coef = self.scheduler.coef_table(self.timesteps).to(dev)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sched = DeviceSchedule(self.t_table, self.step_idx)
        self.latents = torch.zeros((n_img, C, self.h, self.w), dtype=torch.float32, device=dev)
        self.model_in = torch.zeros((2 * n_img, C, self.h, self.w), dtype=dt, device=dev)
        self.enc = torch.zeros((2 * n_img, enc_len, cfg.cross_attention_dim), dtype=dt, device=dev)
        self.history = torch.zeros((num_inference_steps + 1, n_img, C, self.h, self.w), dtype=torch.float32, device=dev)
        self.cn_enc = self.cn_cond = None
        self.cn_scale = 1.0
        if controlnet is not None:
            self.cn_enc = torch.zeros((2 * n_img, controlnet_enc_len, cfg.cross_attention_dim), dtype=dt, device=dev)
            self.cn_cond = torch.zeros((2 * n_img, 3, height, width), dtype=dt, device=dev)
        self.frozen = None
        self.frozen_mask = None
        self.frozen_steps = 0
        self.added = None
        self.graph = None
        self._graph_sig = None
        self.pred_type = 0 if self.scheduler.config.prediction_type == "epsilon" else 1
        self._tproj_table = None
        self._tproj_key = None
        self.adapter_feats = None      # T2I-Adapter features: static CFG-duplicated token-major buffers (set_adapter)
        # Euler ancestral: the per-step noise table (set_step_noise)
        self.step_noise = torch.zeros((self.steps, n_img, C, self.h, self.w), dtype=dt, device=dev) if self.sampler.state == "step_noise" else None
        self._noise_set = False
        # DPM: the multistep state, allocated once (a captured graph holds its address); _reset leaves it alone, row 0 never reads it
        self.x0_prev = torch.zeros_like(self.latents) if self.sampler.state == "x0_prev" else None
        # scale_model_input of step 0 (the epilogue writes the later ones): x / sqrt(sigma_0^2 + 1); None where the sampler does not scale
        self.in_div0 = (float(self.scheduler.model_input_divisor(self.scheduler.index_for_timestep(self.timesteps[0], self.timesteps)))
                        if self.sampler.scales_input else None)

    # ---- conditioning -----------------------------------------------------------------------------------
    def set_conditioning(self, encoder_hidden_states, added_cond_kwargs=None):
        """[2*n_img, L, D] (negatives first).  Copied into the engine's static buffer; the step-invariant text /
        image K, V^T of every IP cross-attention layer are re-projected once here (not once per step)."""
        if tuple(encoder_hidden_states.shape) != tuple(self.enc.shape):
            raise ValueError(f"conditioning shape {tuple(encoder_hidden_states.shape)} != engine shape {tuple(self.enc.shape)}")
        self.enc.copy_(encoder_hidden_states)
        if added_cond_kwargs is not None:
            if self.added is None:
                self.added = {k: v.to(self.dev).clone() for k, v in added_cond_kwargs.items()}
            else:
                for k, v in added_cond_kwargs.items():
                    self.added[k].copy_(v)
        self._refresh_kv()

    def set_control(self, controlnet_prompt_embeds, control_image, conditioning_scale=1.0):
        """ControlNet inputs of reference pipelines.py:761-778: text embeddings [2*n_img, L, D] (negatives first) and the
        prepared control image [2*n_img, 3, H, W] in [0, 1]; both are copied into static buffers (graph replay) and the
        conditioning embedding is recomputed once here, not once per step."""
        if self.controlnet is None:
            raise RuntimeError("DenoiseEngine was built without a controlnet")
        self.cn_enc.copy_(controlnet_prompt_embeds)
        self.cn_cond.copy_(control_image)
        if self.graph is not None and float(conditioning_scale) != self.cn_scale:
            self.graph = None          # the scale is a launch constant of the zero-conv epilogues
        self.cn_scale = float(conditioning_scale)
        self.controlnet.cond_embedding(self.cn_cond, static=True)

    def set_adapter(self, features, conditioning_scale=1.0):
        """T2I-Adapter features of the ``n_img`` images (``T2IAdapter(..., token_major=True)`` ``_Act``s with batch n_img, or NCHW tensors):
        ``state * conditioning_scale`` then ``cat([state] * 2)`` (CFG; reference models/pipelines.py:673-677) into static token-major buffers the
        captured step adds into the UNet (``down_block_additional_residuals`` every step, no mid residual).  ``None`` removes them."""
        from .unet import _Act
        if features is None:
            if self.adapter_feats is not None:
                self.adapter_feats, self.graph = None, None
            return
        acts = []
        for f in features:
            if not isinstance(f, _Act):
                b, c, h, w = f.shape
                t = ops.transpose(f.to(self.dt).contiguous(), b, c, h * w).reshape(b * h * w, c)
                f = _Act(t, b, h, w, c)
            if f.b != self.n_img or f.t.dtype != self.dt:
                raise ValueError(f"set_adapter: features must have batch {self.n_img} and dtype {self.dt}")
            acts.append(f)
        geo = [(f.h, f.w, f.c) for f in acts]
        if self.adapter_feats is None or [(f.h, f.w, f.c) for f in self.adapter_feats] != geo:
            self.adapter_feats = [_Act(torch.empty((2 * f.b * f.hw, f.c), dtype=self.dt, device=self.dev), 2 * f.b, f.h, f.w, f.c) for f in acts]
            self.graph = None                                       # a captured step holds the old buffers' addresses
        for dst, f in zip(self.adapter_feats, acts):
            ops.scale_repeat(f.t.contiguous(), conditioning_scale, 2, out=dst.t)

    def set_step_noise(self, table):
        """Euler ancestral: the noise of every step, [steps, n_img, C, h, w] (``randn(model_output.shape, dtype=model_output.dtype, generator=g)``
        drawn per step by the caller in the reference's generator order), copied into the static table the captured step reads"""
        if self.kind != "euler_a":
            raise RuntimeError("set_step_noise: only an Euler-ancestral engine draws noise in its step")
        self.step_noise.copy_(table.reshape(self.step_noise.shape))
        self._noise_set = True

    def _ip_processors(self):
        return [p for p in self.unet.attn_processors.values() if isinstance(p, IPAttnProcessor)]

    def set_ip_scale(self, scales):
        """The IP-Adapter scale of the engine's images: one number (every image, the reference's ``set_scale``) or ``n_img`` values, one per image — the
        reference generates a character whose database PNG exists at 0.4 and a first appearance at 0 (models/pipelines.py:183-199), and a batch of
        characters mixes the two.  Per-image values are written as ``[s ; s]`` to every IP processor of the UNet, unconditional half first: ``set_scale``
        covers both halves of the classifier-free-guidance batch.  New VALUES replay the captured step (the kernels read them from the device); going
        from the one-value form to the per-image form, or to another ``n_img``, re-captures it once (``_signature``)."""
        vec = scale_vector(scales)
        if vec is not None:
            if len(vec) != self.n_img:
                raise ValueError(f"set_ip_scale: {len(vec)} values for an engine of n_img = {self.n_img} (one number, or one value per image)")
            scales = vec + vec
        for p in self._ip_processors():
            p.scale = scales

    def _refresh_kv(self):
        self.unet.register_conditioning(self.enc)              # cache keyed by the tensor OBJECT self.enc (never its address)

    def set_frozen(self, frozen_latents, frozen_mask, frozen_steps):
        """Stage-2 frozen-mask replace (reference pipelines.py:733-738, 833-834): ``frozen_latents`` fp32
        [steps+1, n_img, C, h, w], ``frozen_mask`` fp32 [h, w] or [n_img, h, w]."""
        if self.graph is not None and (self.frozen is None) != (frozen_latents is None):
            self.graph = None          # epilogue signature changed: re-capture
        if frozen_latents is None:
            self.frozen = self.frozen_mask = None
            self.frozen_steps = 0
            return
        if self.frozen is None:
            self.frozen = torch.empty_like(self.history)
            self.frozen_mask = torch.empty((self.n_img, self.h, self.w), dtype=torch.float32, device=self.dev)
        self.frozen.copy_(frozen_latents)
        self.frozen_mask.copy_(frozen_mask.to(torch.float32).expand(self.n_img, self.h, self.w))
        if self.graph is not None and frozen_steps != self.frozen_steps:
            self.graph = None          # frozen_steps is a launch constant
        self.frozen_steps = int(frozen_steps)

    def _ensure_time_proj(self):
        """The UNet's time path (sinusoidal embedding -> TimestepEmbedding MLP -> SiLU -> all ResBlock ``time_emb_proj`` as one GEMM: models/unet_2d_condition.py:
        315-328, 829-856, diffusers ResnetBlock2D) depends on the timestep ONLY: one row per step of this engine's schedule is computed once, with the very launches
        ``unet.time_embed`` issues per step (same shapes: bit-identical rows), and a step gathers its row by the device step counter — 1 launch instead of 5 per step.
        Rebuilt when the schedule or any of the weights involved change; SDXL's ``text_time`` conditioning enters the embedding, there the per-step path stays."""
        unet = self.unet
        if unet.config.addition_embed_type is not None or os.environ.get("TG_TPROJ_TABLE", "1") == "0":
            if self._tproj_table is not None:
                self._tproj_table, self._tproj_key, self.graph = None, None, None
            return
        te = unet.time_embedding
        ps = [te.linear_1.weight, te.linear_1.bias, te.linear_2.weight, te.linear_2.bias]
        for r in unet._resnets:
            ps += [r.time_emb_proj.weight, r.time_emb_proj.bias]
        key = tuple((p.data_ptr(), tensor_version(p)) for p in ps) + (self.t_table.data_ptr(), tensor_version(self.t_table), unet.dtype)
        if key == self._tproj_key:
            return
        B = 2 * self.n_img
        idx = torch.zeros(1, dtype=torch.int32, device=self.dev)
        rows = []
        with torch.no_grad(), ops.workspace_slot(self.ws_slot):
            for s in range(self.steps):
                idx.fill_(s)
                rows.append(unet.time_embed(DeviceSchedule(self.t_table, idx), B, None)[1].clone())
        self._tproj_table = torch.stack(rows).contiguous()                # [steps, B, sum(cout)]
        self._tproj_key = key
        self.graph = None                                                  # a captured step holds the old table's address

    # ---- one step ---------------------------------------------------------------------------------------
    def _step(self):
        with ops.workspace_slot(self.ws_slot):
            self._step_body()

    def _step_body(self):
        down = mid = None
        if self.controlnet is not None:
            down, mid = self.controlnet(self.model_in, self.sched, self.cn_enc, self.cn_cond, conditioning_scale=self.cn_scale,
                                        return_dict=False, token_major=True)
        tp = None
        if self._tproj_table is not None:
            tp = torch.index_select(self._tproj_table, 0, self.step_idx)[0]        # this step's row, by the DEVICE step counter (graph-replayable)
        if self.adapter_feats is not None:
            down = self.adapter_feats                                          # T2I-Adapter mode: mid stays None
        noise_pred = self.unet(self.model_in, self.sched, self.enc, added_cond_kwargs=self.added, return_dict=False,
                               out_dtype=torch.float32, down_block_additional_residuals=down,
                               mid_block_additional_residual=mid, time_proj=tp, shared_pair=self.added is None)[0]
        self.sampler.epilogue(self, noise_pred, advance=True, frozen=self.frozen, frozen_mask=self.frozen_mask, frozen_steps=self.frozen_steps,
                              history=self.history, model_in=self.model_in)

    def _signature(self):
        """Launch constants baked into a captured graph: the frozen-mask configuration and the guidance scale.  The IP scale VALUES
        are NOT among them: ``IPAttnProcessor.scale`` is read from device memory by the attention kernel, so
        ``IPAdapter.set_scale`` between characters (reference pipelines.py:196, 213) and the per-step gating of
        ``ip_adapter/custom_pipelines.py:328-333`` replay the same graph.  Their FORM is: per IP processor, how many values a step of this batch
        reads (``scale_count``: 1, or 2 n_img once ``set_ip_scale`` was given per-image values) is baked into the captured launches, and with it which
        of the processor's buffers they read (one per length, never freed or moved), so a change of it re-captures.  A per-batch-item scale of
        another length than this engine's batch (another engine's, on a shared UNet) has no meaning here: ValueError."""
        procs, B = self._ip_processors(), 2 * self.n_img
        for p in procs:
            if isinstance(p.scale, tuple) and len(p.scale) != B:
                raise ValueError(f"DenoiseEngine (n_img = {self.n_img}): an IP processor of the UNet holds {len(p.scale)} per-batch-item scales, a step "
                                 f"of this engine has batch {B}; call set_ip_scale on THIS engine (or assign a number) before running it")
        ip_form = tuple(p.scale_count(B) for p in procs)
        return self.frozen is not None, self.frozen_steps, self.g, ip_form

    def _check_replayable(self):
        """after a ``before_step`` hook, before the replay it precedes: what the captured step baked in must still hold.  A hook may assign new VALUES
        (numbers, or vectors of the form the step was captured in); one that changes the form — per-image scales on an engine captured with a number,
        a vector of another length — would have the replay read a buffer the new values were not written to."""
        if self.use_graph and self._signature() != self._graph_sig:
            raise RuntimeError("DenoiseEngine: a before_step hook changed what the captured step bakes in (the FORM of the IP scale: one number / one "
                               "value per image, or the frozen-mask / guidance constants); the replay would not see it.  Put the engine into that "
                               "form before run() — set_ip_scale([...]) — and let the hook assign values of the same form")

    def _reset(self, latents):
        self.latents.copy_(latents.to(device=self.dev, dtype=torch.float32))
        self.history[0].copy_(self.latents)
        x0 = self.latents if self.in_div0 is None else self.latents / self.in_div0     # scale_model_input of step 0
        self.model_in[:self.n_img].copy_(x0)                     # dtype cast on copy = the `.half()` of pipelines.py:414
        self.model_in[self.n_img:].copy_(x0)
        self.step_idx.zero_()

    def _capture(self):
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(s):
            self._step()                                          # warm-up: allocator, packed weights, K/V caches
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        self.graph = g

    def _ensure_graph(self, latents):
        self._ensure_time_proj()
        sig = self._signature()
        if self.use_graph and (self.graph is None or sig != self._graph_sig):
            self._reset(latents)
            self._capture()
            self._graph_sig = sig

    @staticmethod
    def run_concurrent(engines, latents_list, before_step=None):
        """Independent denoising chains (e.g. the two halves of a story's character batch) replayed CONCURRENTLY, one HIP
        stream per engine: the second chain's kernels fill the partially filled grid rounds, small-grid layers and
        launch gaps of the first (+4 % images/s for 2 x 4 images vs 1 x 8 on MI355X).  Engines may share one UNet; each
        has its own conditioning buffers, K / V^T caches, kernel scratch slot and captured graph.  Returns the histories.
        The IP scale lives with the processor (= per UNet): one number, or one value per batch item of the step (``set_ip_scale``; engines that share
        a UNet then need the same ``n_img``).  ``before_step(i)`` (optional) runs on the host before round i of replays is queued — the per-step
        ``set_scale`` gating of ``ip_adapter/custom_pipelines.py:328-333``: the assignment fences its write (a fill, or the copy of a vector) against
        the engine streams (``attention_processor.fenced_fill`` / ``fenced_copy``), so round i - 1 still reads the old values and round i the new ones.
        A hook may change VALUES, not the form the steps were captured in (RuntimeError before the round is queued)."""
        dev = engines[0].dev
        with torch.no_grad():
            for e, lat in zip(engines, latents_list):
                if not e.use_graph:
                    raise RuntimeError("run_concurrent needs graph engines")
                e._ensure_graph(lat)
            cur = torch.cuda.current_stream(dev)
            streams = [e._stream() for e in engines]
            for e, lat, st in zip(engines, latents_list, streams):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    e._reset(lat)
            for i in range(engines[0].steps):
                if before_step is not None:
                    before_step(i)
                    for e in engines:
                        e._check_replayable()
                for e, st in zip(engines, streams):
                    with torch.cuda.stream(st):
                        e.graph.replay()
            for st in streams:
                cur.wait_stream(st)
        return [e.history for e in engines]

    def _stream(self):
        if getattr(self, "_own_stream", None) is None:
            # registered: host-side writes of device scalars the captured step reads (IPAttnProcessor.scale) fence against it
            self._own_stream = register_replay_stream(torch.cuda.Stream(device=self.dev), self.dev)
            weakref.finalize(self, unregister_replay_stream, self._own_stream)
        return self._own_stream

    def run(self, latents, before_step=None):
        """latents [n_img, C, h, w] (any float dtype / device) -> latents_all fp32 [steps+1, n_img, C, h, w] on the GPU.
        ``before_step(i)`` (optional) runs on the host before step i is launched — the place of the per-step
        ``set_scale(0.0)`` / ``set_scale(s)`` gating of reference ``ip_adapter/custom_pipelines.py:328-333``; the IP scale is read from
        device memory, so the same captured graph replays whatever VALUES it is set to.  A hook that changes its FORM (per-image values on an engine
        captured with one number, a vector of another length) raises RuntimeError before the step is replayed: ``set_ip_scale`` comes before ``run``."""
        if self.kind == "euler_a" and not self._noise_set:
            raise RuntimeError("DenoiseEngine (Euler ancestral): set_step_noise(...) before run(): the step noise is drawn on the host in the reference's order")
        with torch.no_grad():
            self._ensure_graph(latents)
            self._reset(latents)
            for i in range(self.steps):
                if before_step is not None:
                    before_step(i)
                    self._check_replayable()
                if self.use_graph:
                    self.graph.replay()
                else:
                    self._step()
        return self.history


def denoise_single_object(adapter, prompt_embeds, negative_prompt_embeds, input_latents, scale, clip_image_embeds=None,
                          image_prompt_embeds=None, uncond_image_prompt_embeds=None, num_inference_steps=50,
                          guidance_scale=7.5, engine=None):
    """Stage-1 per-character generation core (reference ``generate_semantic_guidance`` SD-1.5 branch, :183-247 image
    prompt + scale, :369-453 loop, :488 stack): returns ``(latents [1,C,h,w], latents_all [steps+1,1,C,h,w])``.  ``scale``: one number, or one value
    per row of ``prompt_embeds`` (a batch of characters, each at its own IP scale: ``DenoiseEngine.set_ip_scale``)."""
    per_image = scale_vector(scale)
    if per_image is None:
        adapter.set_scale(scale)
    if image_prompt_embeds is None:
        image_prompt_embeds, uncond_image_prompt_embeds = adapter.get_image_embeds(clip_image_embeds=clip_image_embeds)
    enc = prepare_ip_embeds(prompt_embeds.to(adapter.pipe.unet.dtype), negative_prompt_embeds.to(adapter.pipe.unet.dtype),
                            image_prompt_embeds, uncond_image_prompt_embeds)
    n = prompt_embeds.shape[0]
    if engine is None:
        engine = DenoiseEngine(adapter.pipe.unet, adapter.pipe.scheduler, n_img=n, height=input_latents.shape[-2] * 8,
                               width=input_latents.shape[-1] * 8, num_inference_steps=num_inference_steps,
                               guidance_scale=guidance_scale, enc_len=enc.shape[1])
    if per_image is not None:
        engine.set_ip_scale(per_image)
    engine.set_conditioning(enc)
    latents_all = engine.run(input_latents)
    return latents_all[-1], latents_all


# ---- the reference's two stage functions, same signatures and return tuples, on the engine ------------------------------------------------------
SINGLE_OBJECT_NEGATIVE_PROMPT = "background, multiple objects, incomplete, lowres, bad anatomy, low quality, obscured"      # models/pipelines.py:225
PLACEHOLDER_IMAGE = "model.png"                                                                                            # models/pipelines.py:195


def _own_unet(adapter, what):
    from .unet import UNet2DConditionModel
    unet = adapter.pipe.unet
    if not isinstance(unet, UNet2DConditionModel):
        raise TypeError(f"theatergen_amd.pipelines.{what}: adapter.pipe.unet must be a theatergen_amd.unet.UNet2DConditionModel (INTEGRATION.md level 1: "
                        f"UNet2DConditionModel.from_state_dict(config.sd15(), diffusers_unet.state_dict(), ...)), got {type(unet).__name__}")
    return unet


def _engine_of(adapter, unet=None, scheduler=None, **kw):
    """one engine (static buffers + captured step graph) per loop geometry, kept on the adapter: the characters of a run replay the same graph.
    Keyed on the UNet and the scheduler (identity and kind) too: stage 2 of the SDXL flow runs ``controlnetpipe.unet`` with the Euler-ancestral
    scheduler of ``controlnetpipe``, stage 1 ``adapter.pipe.unet`` with its Euler scheduler (default: ``adapter.pipe``'s)."""
    unet = adapter.pipe.unet if unet is None else unet
    scheduler = adapter.pipe.scheduler if scheduler is None else scheduler
    cache = adapter.__dict__.setdefault("_tg_engines", {})
    key = tuple(sorted((k, (tuple(v.tolist()) if k == "timesteps" and v is not None else (id(v) if k == "controlnet" else v))) for k, v in kw.items()))
    key += (("unet", id(unet)), ("scheduler", id(scheduler), type(scheduler).__name__))
    eng = cache.get(key)
    if eng is None or eng.unet is not unet or eng.scheduler is not scheduler:
        eng = cache[key] = DenoiseEngine(unet, scheduler, **kw)
    return eng


def _to_pil(image):
    """``image_processor.postprocess(image, output_type='pil', do_denormalize=[True])[0]`` (models/pipelines.py:475): NCHW in [-1, 1] -> PIL RGB"""
    from PIL import Image
    import numpy as np
    arr = (image[0].float() / 2 + 0.5).clamp(0, 1).permute(1, 2, 0).cpu().numpy()
    return Image.fromarray((arr * 255).round().astype(np.uint8))


def _text_and_image_rows(adapter, prompt, negative_prompt, pil_image):
    """[negative rows ; positive rows] = text tokens followed by the IP-Adapter image tokens (models/pipelines.py:204-233, 369-370, 864-948)"""
    img, unc = adapter.get_image_embeds(pil_image=pil_image, clip_image_embeds=None)
    pos, neg = adapter.pipe.encode_prompt(prompt, device=adapter.device, num_images_per_prompt=1, do_classifier_free_guidance=True,
                                          negative_prompt=negative_prompt)[:2]
    return prepare_ip_embeds(pos, neg, img.to(pos.device), unc.to(pos.device))


def generate_semantic_guidance(task, fg_seed_now, basever, ip_prompt, database_path, id, adapter, model_dict, latents, input_embeddings,
                               num_inference_steps, bboxes, phrases, object_positions, guidance_scale=7.5, semantic_guidance_kwargs=None,
                               return_cross_attn=False, return_saved_cross_attn=False, saved_cross_attn_keys=None, return_cond_ca_only=False,
                               return_token_ca_only=None, offload_guidance_cross_attn_to_cpu=False, offload_cross_attn_to_cpu=False,
                               offload_latents_to_cpu=True, return_box_vis=False, show_progress=True, save_all_latents=False,
                               dynamic_num_inference_steps=False, fast_after_steps=None, fast_rate=2, use_boxdiff=False, use_adapter=False,
                               obj_id=False, have_reffer=0):
    """Stage 1, one character (reference ``models/pipelines.py:175-490``; caller ``theatergen.py:108-135``): same arguments, same side effects (the
    character's first image becomes its reference PNG, :476-477), same return tuple ``(latents, image[, saved_attns][, image][, latents_all])``.

    What runs where.  Host, as in the reference: the reference image / placeholder and its IP scale (:183-199), the prompt strings (:216-225),
    ``adapter.get_image_embeds`` and ``adapter.pipe.encode_prompt``.  Device: the whole loop :406-453 is ``num_inference_steps`` replays of ONE captured
    step (UNet CFG call + fused CFG / DDIM epilogue + history row) — no ``.cpu()`` per step; the 51 latents come back in one copy when
    ``offload_latents_to_cpu`` asks for them on the host.  ``cross_attention_kwargs`` is ``None`` in the reference's UNet call (:428), so no map is
    ever saved: ``saved_attns`` is the reference's list of empty dicts.  ``basever='xl'``: the SDXL branch (``_semantic_guidance_xl``).  Unsupported
    here, loudly: ``return_cross_attn`` (an attribute no diffusers output has)."""
    from PIL import Image
    from . import schedule as tg_schedule
    if basever == "xl":
        _check_xl_stage1(adapter)
    if return_cross_attn:
        raise NotImplementedError("return_cross_attn reads unet_output.cross_attention_probs_* (models/pipelines.py:431-434), which the UNet call of "
                                  "the reference never fills; the saved-map side channel is save_attn_to_dict")
    if not obj_id:
        raise RuntimeError("generate_semantic_guidance: obj_id is required (without it the reference has no prompt embeddings to run on, models/pipelines.py:183-233)")
    unet = _own_unet(adapter, "generate_semantic_guidance")
    # ---- image prompt of the character: its database PNG, or the placeholder with the adapter switched off (:183-199)
    try:
        image = Image.open(database_path + str(obj_id) + ".png")
        scale, have_reffer = 0.4, 1
    except (OSError, ValueError):
        image = Image.open(PLACEHOLDER_IMAGE)
        scale, have_reffer = 0, 0
    adapter.set_scale(scale)
    prompt = ("single object, " if task == "editing" else "full-body picture of ") + str(ip_prompt)
    if basever == "xl":
        return _semantic_guidance_xl(adapter, unet, prompt, image, have_reffer, database_path, obj_id, fg_seed_now, num_inference_steps, guidance_scale,
                                     fast_after_steps, fast_rate, return_saved_cross_attn, return_box_vis, save_all_latents, offload_latents_to_cpu)
    enc = _text_and_image_rows(adapter, prompt, SINGLE_OBJECT_NEGATIVE_PROMPT, image)
    # ---- the loop
    scheduler = adapter.pipe.scheduler
    timesteps = None
    if fast_after_steps is not None:
        scheduler.set_timesteps(num_inference_steps)
        timesteps = tg_schedule.get_fast_schedule(scheduler.timesteps, fast_after_steps, fast_rate)
    h8, w8 = latents.shape[-2], latents.shape[-1]
    eng = _engine_of(adapter, n_img=latents.shape[0], height=8 * h8, width=8 * w8, num_inference_steps=num_inference_steps,
                     guidance_scale=guidance_scale, enc_len=enc.shape[1], timesteps=timesteps)
    eng.set_conditioning(enc.to(eng.dev, eng.dt))
    hist = eng.run(latents)
    out = hist[-1].to(unet.dtype)                                # the reference's `latents.half()` (:461), in the UNet's storage dtype
    vae = adapter.pipe.vae
    decoded = vae.decode(out / vae.config.scaling_factor, return_dict=False)[0].detach()
    post = getattr(getattr(adapter.pipe, "image_processor", None), "postprocess", None)
    images = post(decoded, output_type="pil", do_denormalize=[True])[0] if post is not None else _to_pil(decoded)
    if have_reffer == 0:
        images.save(database_path + str(obj_id) + ".png")       # the character's first appearance becomes its reference (:476-477)
    ret = [out, images]
    if return_saved_cross_attn:
        ret.append([{} for _ in range(eng.steps)])
    if return_box_vis:
        ret.append(images)
    if save_all_latents:
        allv = hist.to(latents.dtype).clone()
        ret.append(allv.cpu() if offload_latents_to_cpu else allv)
    return tuple(ret)


def generate_characters(task, fg_seeds, basever, ip_prompts, database_path, adapter, latents, num_inference_steps, obj_ids, guidance_scale=7.5,
                        fast_after_steps=None, fast_rate=2, save_all_latents=False, offload_latents_to_cpu=True):
    """Stage 1 of the non-XL branches for a LIST of characters in ONE engine run — what ``generate_semantic_guidance`` does once per character
    (reference ``models/pipelines.py:175-490``), with the characters in the batch dimension of the captured step.  ``ip_prompts`` / ``obj_ids`` /
    ``fg_seeds``: one entry per character; ``latents`` [n, C, h, w]: their initial latents (the reference draws them before the call and ``fg_seeds``
    play no further part in its non-XL branch: they are only checked for length).

    Per character, on the host, as in the reference: the database PNG and IP scale 0.4 — or the placeholder and scale 0 for a first appearance
    (:183-199) —, the prompt prefix (:216-225), ``adapter.get_image_embeds`` and ``adapter.pipe.encode_prompt``.  Then ONE ``set_ip_scale`` with the
    list of scales (the kernels read each image's own value), ONE ``run``, one decode per image, and each first appearance is saved as its reference
    PNG (:476-477).  Afterwards the adapter's scale is the LAST character's number, as after the reference's loop over the same characters.  Returns a list with, per character, the tuple ``generate_semantic_guidance`` returns for it: ``(latents [1, C, h, w], image[,
    latents_all [steps + 1, 1, C, h, w]])``.

    Refused: ``basever='xl'`` (its stage 1 draws its own latents: NotImplementedError); two entries with the same ``obj_id`` and no PNG yet
    (ValueError: one at a time, the second would have been generated with the first's image as its reference)."""
    from PIL import Image
    from . import schedule as tg_schedule
    if basever == "xl":
        raise NotImplementedError("generate_characters: the SDXL stage 1 draws its own latents per character (models/pipelines.py:251-300); "
                                  "run generate_semantic_guidance(..., basever='xl') per character")
    n = len(obj_ids)
    if n == 0 or len(ip_prompts) != n or len(fg_seeds) != n or latents.shape[0] != n:
        raise ValueError(f"generate_characters: {n} obj_ids, {len(ip_prompts)} ip_prompts, {len(fg_seeds)} fg_seeds, latents batch {latents.shape[0]}: "
                         "one entry per character")
    if any(not o for o in obj_ids):
        raise RuntimeError("generate_characters: every character needs an obj_id (models/pipelines.py:183-233)")
    unet = _own_unet(adapter, "generate_characters")
    images_in, scales, new = [], [], []
    for o in obj_ids:
        try:
            images_in.append(Image.open(database_path + str(o) + ".png"))
            scales.append(0.4)
            new.append(False)
        except (OSError, ValueError):
            if any(isnew and str(prev) == str(o) for prev, isnew in zip(obj_ids, new)):
                raise ValueError(f"generate_characters: obj_id {o!r} appears twice and has no reference image yet ({database_path + str(o)}.png): in the "
                                 "reference the second generation uses the first's image; generate them in two calls") from None
            images_in.append(None)
            scales.append(0)
            new.append(True)
    if any(new):
        placeholder = Image.open(PLACEHOLDER_IMAGE)
        images_in = [placeholder if im is None else im for im in images_in]
    prefix = "single object, " if task == "editing" else "full-body picture of "
    rows = [_text_and_image_rows(adapter, prefix + str(p), SINGLE_OBJECT_NEGATIVE_PROMPT, im) for p, im in zip(ip_prompts, images_in)]     # each [2, L, D]
    enc = torch.cat([r[:1] for r in rows] + [r[1:] for r in rows], dim=0)                       # negatives first
    scheduler = adapter.pipe.scheduler
    timesteps = None
    if fast_after_steps is not None:
        scheduler.set_timesteps(num_inference_steps)
        timesteps = tg_schedule.get_fast_schedule(scheduler.timesteps, fast_after_steps, fast_rate)
    h8, w8 = latents.shape[-2], latents.shape[-1]
    eng = _engine_of(adapter, n_img=n, height=8 * h8, width=8 * w8, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                     enc_len=enc.shape[1], timesteps=timesteps)
    eng.set_ip_scale(scales)
    eng.set_conditioning(enc.to(eng.dev, eng.dt))
    hist = eng.run(latents)
    # what the reference's loop over these characters leaves behind: the LAST character's number (queued after the replays; the per-image buffer keeps
    # its length, so the next call replays the same graph).  The paths that take the scale as a host constant — stage-2 guidance: attention-map
    # capture, the reverse pass — refuse a vector; they must find a number on this UNet afterwards, as after generate_semantic_guidance
    adapter.set_scale(scales[-1])
    out = hist[-1].to(unet.dtype)
    vae = adapter.pipe.vae
    post = getattr(getattr(adapter.pipe, "image_processor", None), "postprocess", None)
    results = []
    for i, o in enumerate(obj_ids):
        decoded = vae.decode(out[i:i + 1] / vae.config.scaling_factor, return_dict=False)[0].detach()
        image = post(decoded, output_type="pil", do_denormalize=[True])[0] if post is not None else _to_pil(decoded)
        if new[i]:
            image.save(database_path + str(o) + ".png")
        ret = [out[i:i + 1], image]
        if save_all_latents:
            allv = hist[:, i:i + 1].to(latents.dtype).clone()
            ret.append(allv.cpu() if offload_latents_to_cpu else allv)
        results.append(tuple(ret))
    return results


def _check_xl_stage1(adapter):
    """up front, before any encoding: the SDXL branch of stage 1 needs this package's SDXL UNet (``text_time`` plan) and Euler scheduler"""
    from .unet import UNet2DConditionModel
    unet = getattr(adapter.pipe, "unet", None)
    if not isinstance(unet, UNet2DConditionModel) or unet.config.addition_embed_type != "text_time":
        raise NotImplementedError("theatergen_amd.pipelines.generate_semantic_guidance('xl'): adapter.pipe.unet must be a theatergen_amd UNet2DConditionModel "
                                  "with an SDXL (addition_embed_type='text_time') plan, e.g. from_state_dict(config.sdxl(), ...)")
    if not isinstance(adapter.pipe.scheduler, EulerDiscreteScheduler) or isinstance(adapter.pipe.scheduler, EulerAncestralDiscreteScheduler):
        raise NotImplementedError("theatergen_amd.pipelines.generate_semantic_guidance('xl'): adapter.pipe.scheduler must be a "
                                  f"theatergen_amd.scheduler.EulerDiscreteScheduler (the SDXL base scheduler), got {type(adapter.pipe.scheduler).__name__}")


def _xl_added_cond(pooled, negative_pooled, height, width, dev, dtype):
    """``added_cond_kwargs`` of the SDXL loops (models/pipelines.py:321-345, 677-691): pooled rows [negative ; positive], time ids (H, W, 0, 0, H, W) twice"""
    text_embeds = torch.cat([negative_pooled, pooled], dim=0).to(dev, dtype)
    ids = torch.tensor([[float(height), float(width), 0.0, 0.0, float(height), float(width)]], dtype=torch.float32)
    return {"text_embeds": text_embeds, "time_ids": torch.cat([ids, ids], dim=0).repeat(pooled.shape[0], 1).to(dev)}


def _decode_pil(pipe, vae, latents):
    """``vae.decode(latents / scaling_factor)`` in the VAE's own dtype -> ``pipe.image_processor.postprocess(image, output_type='pil')`` (a list)"""
    vdt = getattr(vae, "dtype", latents.dtype)
    decoded = vae.decode(latents.to(vdt) / vae.config.scaling_factor, return_dict=False)[0].detach()
    post = getattr(getattr(pipe, "image_processor", None), "postprocess", None)
    return post(decoded, output_type="pil") if post is not None else [_to_pil(decoded[i:i + 1]) for i in range(decoded.shape[0])]


def _semantic_guidance_xl(adapter, unet, prompt, image, have_reffer, database_path, obj_id, fg_seed_now, num_inference_steps, guidance_scale,
                          fast_after_steps, fast_rate, return_saved_cross_attn, return_box_vis, save_all_latents, offload_latents_to_cpu):
    """Stage 1, SDXL (models/pipelines.py:204-214, 255-366, 372-453, 459-477).  The caller's ``latents`` are not used: the start latents are
    ``randn([1, 4, H/8, W/8], generator=Generator(device).manual_seed(fg_seed_now), dtype=embeds dtype) * init_noise_sigma`` with H = W =
    ``sample_size * vae_scale_factor``; Euler steps; a fast schedule replaces ``timesteps`` and keeps the full ``sigmas`` (step i uses sigmas[i])."""
    from . import schedule as tg_schedule
    pipe = adapter.pipe
    scheduler = pipe.scheduler
    dev, dtype = unet.device, unet.dtype
    img, unc = adapter.get_image_embeds(pil_image=image, clip_image_embeds=None)
    pos, neg, pooled, neg_pooled = pipe.encode_prompt(prompt, num_images_per_prompt=1, do_classifier_free_guidance=True,
                                                      negative_prompt=SINGLE_OBJECT_NEGATIVE_PROMPT)
    enc = prepare_ip_embeds(pos, neg, img.to(pos.device), unc.to(pos.device))
    height = width = unet.config.sample_size * pipe.vae_scale_factor
    scheduler.set_timesteps(num_inference_steps)
    generator = torch.Generator(dev).manual_seed(fg_seed_now)
    lat0 = torch.randn((1, unet.config.in_channels, height // 8, width // 8), generator=generator, device=dev, dtype=enc.dtype)
    lat0 = lat0 * scheduler.init_noise_sigma.to(dev)                                                      # prepare_latents (:307-316)
    timesteps = None
    if fast_after_steps is not None:
        timesteps = tg_schedule.get_fast_schedule(scheduler.timesteps, fast_after_steps, fast_rate)
    eng = _engine_of(adapter, unet=unet, scheduler=scheduler, n_img=1, height=height, width=width, num_inference_steps=num_inference_steps,
                     guidance_scale=guidance_scale, enc_len=enc.shape[1], timesteps=timesteps)
    eng.set_conditioning(enc.to(dev, dtype), _xl_added_cond(pooled, neg_pooled, height, width, dev, dtype))
    hist = eng.run(lat0)
    out = hist[-1].to(dtype)                                                                              # `latents.half()` (:457)
    images = _decode_pil(pipe, pipe.vae, out)[0]
    if have_reffer == 0:
        images.save(database_path + str(obj_id) + ".png")
    ret = [out, images]
    if return_saved_cross_attn:
        ret.append([{} for _ in range(eng.steps)])
    if return_box_vis:
        ret.append(images)
    if save_all_latents:
        allv = hist.to(lat0.dtype).clone()
        ret.append(allv.cpu() if offload_latents_to_cpu else allv)
    return tuple(ret)


def _adapter_image(image, height, width):
    """diffusers ``_preprocess_adapter_image``: PIL -> Lanczos resize to (width, height) -> [0, 1] fp32 NCHW (an ndarray or a tensor as given)"""
    import numpy as np
    from PIL import Image
    if torch.is_tensor(image):
        return image
    if not isinstance(image, Image.Image):
        image = Image.fromarray(np.asarray(image))
    arr = np.array(image.resize((width, height), resample=Image.LANCZOS))
    arr = arr[None, ..., None] if arr.ndim == 2 else arr[None]
    return torch.from_numpy(arr.astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous()


def _check_xl_stage2(adapter, controlnetpipe):
    """up front, before any encoding: what the SDXL branch of stage 2 runs on must be this package's"""
    from .t2i_adapter import T2IAdapter
    from .unet import UNet2DConditionModel
    unet = getattr(controlnetpipe, "unet", None)
    if not isinstance(unet, UNet2DConditionModel) or unet.config.addition_embed_type != "text_time":
        raise NotImplementedError("theatergen_amd.pipelines.final_image_generation('xl'): controlnetpipe.unet must be a theatergen_amd UNet2DConditionModel "
                                  "with an SDXL (addition_embed_type='text_time') plan")
    if not isinstance(getattr(controlnetpipe, "adapter", None), T2IAdapter):
        raise NotImplementedError("theatergen_amd.pipelines.final_image_generation('xl'): controlnetpipe.adapter must be a theatergen_amd.t2i_adapter.T2IAdapter, "
                                  f"got {type(getattr(controlnetpipe, 'adapter', None)).__name__}")
    if not isinstance(getattr(controlnetpipe, "scheduler", None), EulerAncestralDiscreteScheduler):
        raise NotImplementedError("theatergen_amd.pipelines.final_image_generation('xl'): controlnetpipe.scheduler must be a "
                                  "theatergen_amd.scheduler.EulerAncestralDiscreteScheduler")
    if not isinstance(adapter.pipe.scheduler, EulerDiscreteScheduler) or isinstance(adapter.pipe.scheduler, EulerAncestralDiscreteScheduler):
        raise NotImplementedError("theatergen_amd.pipelines.final_image_generation('xl'): adapter.pipe.scheduler must be a "
                                  "theatergen_amd.scheduler.EulerDiscreteScheduler (its timesteps, add_noise and init_noise_sigma are used)")


def _final_image_xl(processor, controlnetpipe, overall_prompt, overall_negative_prompt, height, width, bg_seed, inp_mask, input_img, adapter, latents_all,
                    num_inference_steps, frozen_steps, guidance_scale):
    """Stage 2, SDXL (models/pipelines.py:592-700, 733-857): T2I-Adapter-XL + ``controlnetpipe.unet`` + Euler-ancestral steps, text rows only."""
    import numpy as np
    unet, t2i, euler_a, euler = controlnetpipe.unet, controlnetpipe.adapter, controlnetpipe.scheduler, adapter.pipe.scheduler
    dev, dtype = unet.device, unet.dtype
    generator = torch.Generator(dev).manual_seed(bg_seed)
    euler.set_timesteps(num_inference_steps)
    euler_a.set_timesteps(num_inference_steps)
    if not torch.equal(euler.timesteps, euler_a.timesteps):
        raise ValueError("final_image_generation('xl'): adapter.pipe.scheduler and controlnetpipe.scheduler must have the same timesteps")
    h8, w8 = int(height / 8), int(width / 8)
    m = np.array(inp_mask.resize((h8, w8)).convert("L")).astype(np.float32) / 255.0
    m[m > 0] = 1
    my_mask = torch.from_numpy(1 - m).to(device=dev, dtype=torch.float32)
    img = torch.from_numpy(np.array(input_img).astype(np.float32) / 255.0)[None].permute(0, 3, 1, 2)
    myimage = (2.0 * img - 1.0).to(device=dev, dtype=dtype)
    vae = controlnetpipe.vae
    # generator A (bg_seed): posterior sample, re-noising noise, the background draw the SDXL branch never uses (:617-632)
    init_latents = vae.config.scaling_factor * vae.encode(myimage).latent_dist.sample(generator=generator)
    noise = torch.randn(init_latents.shape, generator=generator, device=dev, dtype=dtype)
    my_latents = euler.add_noise(init_latents, noise, euler.timesteps).unsqueeze(1)                      # [steps, 1, C, h, w]
    torch.randn((1, unet.config.in_channels, h8, w8), generator=generator, device=dev, dtype=dtype)
    control_image = processor(np.array(input_img), detect_resolution=384, image_resolution=1024)
    adapter_input = _adapter_image(control_image, height, width).to(device=dev, dtype=dtype)
    pos, neg, pooled, neg_pooled = controlnetpipe.encode_prompt(prompt=overall_prompt, num_images_per_prompt=1, do_classifier_free_guidance=True,
                                                                negative_prompt=overall_negative_prompt)
    # generator B (bg_seed again): the start latents, then one ancestral draw per step (:654-667, extra_step_kwargs)
    generator = torch.Generator(dev).manual_seed(bg_seed)
    start = torch.randn((1, unet.config.in_channels, h8, w8), generator=generator, device=dev, dtype=pos.dtype) * euler_a.init_noise_sigma.to(dev)
    step_noise = torch.stack([torch.randn((1, unet.config.in_channels, h8, w8), generator=generator, device=dev, dtype=dtype)
                              for _ in range(len(euler.timesteps))])
    feats = t2i(adapter_input, token_major=True)
    latents_all[0] = start.to(latents_all.device, latents_all.dtype)
    latents_all[1:] = my_latents.to(latents_all.device, latents_all.dtype)
    enc = torch.cat([neg, pos], dim=0).to(dev, dtype)
    eng = _engine_of(adapter, unet=unet, scheduler=euler_a, n_img=1, height=height, width=width, num_inference_steps=num_inference_steps,
                     guidance_scale=guidance_scale, enc_len=enc.shape[1], timesteps=euler.timesteps)
    eng.set_conditioning(enc, _xl_added_cond(pooled, neg_pooled, height, width, dev, dtype))
    eng.set_adapter(feats, 0.8)                                                                           # adapter_conditioning_scale (:674-675)
    eng.set_step_noise(step_noise)
    eng.set_frozen(latents_all.to(dev, torch.float32), my_mask, frozen_steps)
    latents = eng.run(start)[-1].to(dtype)
    return latents, _decode_pil(controlnetpipe, vae, latents)


def _control_image(controlnetpipe, control_image, width, height, device, dtype):
    """``controlnetpipe.prepare_image(...)`` of :712-722 (CFG: the image twice) or, for a pipeline object without it, the same preparation:
    resize to (width, height) with LANCZOS, [0, 1], NCHW"""
    if hasattr(controlnetpipe, "prepare_image"):
        return controlnetpipe.prepare_image(image=control_image, width=width, height=height, batch_size=1, num_images_per_prompt=1, device=device,
                                            dtype=dtype, do_classifier_free_guidance=True, guess_mode=False)
    import numpy as np
    from PIL import Image
    if torch.is_tensor(control_image):
        t = control_image.to(device=device, dtype=dtype)
        t = t if t.dim() == 4 else t[None]
    else:
        pil = control_image if isinstance(control_image, Image.Image) else Image.fromarray(np.asarray(control_image))
        arr = np.asarray(pil.convert("RGB").resize((width, height), resample=Image.LANCZOS)).astype(np.float32) / 255.0
        t = torch.from_numpy(arr).permute(2, 0, 1)[None].to(device=device, dtype=dtype)
    return torch.cat([t] * 2)


@torch.no_grad()
def final_image_generation(basever, processor, controlnetpipe, tpipe, overall_prompt, overall_negative_prompt, bg_prompt, single_obj_img_list, objects,
                           repeat_ind, height, width, bg_seed, inp_mask, input_img, adapter, model_dict, latents_all, frozen_mask, bg_input_embeddings,
                           input_embeddings, num_inference_steps, frozen_steps, guidance_scale=7.5, bboxes=None, phrases=None, object_positions=None,
                           semantic_guidance_kwargs=None, offload_guidance_cross_attn_to_cpu=False, use_boxdiff=False):
    """Stage 2, the final image (reference ``models/pipelines.py:592-857``, SD-1.5 branch; caller ``theatergen.py:448-484``): same arguments, returns
    ``(latents, images uint8 [1, H, W, 3])``.  As in the reference: the frozen latents are the pasted image VAE-encoded and re-noised at ALL timesteps
    (:617-631) and OVERWRITE the caller's ``latents_all`` (:737-738); the frozen mask is the inverted, re-binarised 64 x 64 resize of ``inp_mask``
    (:605-614), not the ``frozen_mask`` argument; the start latents are fresh background noise (:632); IP scale 0.1 on the first character's image
    (:700-701); ControlNet at scale 1 on ``processor(input_img)`` every step (:705-731, 762-778).  All random draws come from the DEVICE generator
    seeded with ``bg_seed`` (:594, 625-632), in the reference's order.  Device: one captured step (ControlNet + UNet + CFG / DDIM / frozen-mask
    replace) replayed ``num_inference_steps`` times; no per-step ``.cpu()`` (:835).  ``basever='xl'``: the SDXL branch (``_final_image_xl``),
    returns ``(latents, list of PIL images)`` as the reference does."""
    import numpy as np
    if basever == "xl":
        _check_xl_stage2(adapter, controlnetpipe)
        return _final_image_xl(processor, controlnetpipe, overall_prompt, overall_negative_prompt, height, width, bg_seed, inp_mask, input_img, adapter,
                               latents_all, num_inference_steps, frozen_steps, guidance_scale)
    unet = _own_unet(adapter, "final_image_generation")
    from .controlnet import ControlNetModel
    controlnet = controlnetpipe.controlnet
    if not isinstance(controlnet, ControlNetModel):
        raise TypeError("theatergen_amd.pipelines.final_image_generation: controlnetpipe.controlnet must be a theatergen_amd.controlnet.ControlNetModel "
                        f"(INTEGRATION.md, stage 2), got {type(controlnet).__name__}")
    vae, scheduler, dtype, dev = adapter.pipe.vae, adapter.pipe.scheduler, unet.dtype, unet.device
    generator = torch.Generator(dev).manual_seed(bg_seed)
    text_embeddings, uncond_embeddings, cond_embeddings = input_embeddings
    scheduler.set_timesteps(num_inference_steps)
    h8, w8 = int(height / 8), int(width / 8)
    # frozen mask: 1 where a character was pasted (inp_mask is 0 there)
    m = np.array(inp_mask.resize((h8, w8)).convert("L")).astype(np.float32) / 255.0
    m[m > 0] = 1
    my_mask = torch.from_numpy(1 - m).to(device=dev, dtype=torch.float32)
    # frozen latents: the pasted image through the VAE encoder, re-noised at every timestep
    img = torch.from_numpy(np.array(input_img).astype(np.float32) / 255.0)[None].permute(0, 3, 1, 2)
    myimage = (2.0 * img - 1.0).to(device=dev, dtype=dtype)
    init_latents = vae.config.scaling_factor * vae.encode(myimage).latent_dist.sample(generator=generator)
    noise = torch.randn(init_latents.shape, generator=generator, device=dev, dtype=dtype)
    my_latents = scheduler.add_noise(init_latents, noise, scheduler.timesteps).unsqueeze(1)                    # [steps, 1, C, h, w]
    my_bg = torch.randn((1, unet.config.in_channels, h8, w8), generator=generator, device=dev, dtype=dtype) * float(scheduler.init_noise_sigma)
    # conditioning: overall prompt + the first character's image tokens at scale 0.1; ControlNet sees the text rows only
    ip_embeds = _text_and_image_rows(adapter, overall_prompt, overall_negative_prompt, single_obj_img_list[0])
    adapter.set_scale(0.1)
    imagetight = _control_image(controlnetpipe, processor(np.array(input_img)), width, height, dev, dtype)
    latents_all[0] = my_bg.to(latents_all.device, latents_all.dtype)
    latents_all[1:] = my_latents.to(latents_all.device, latents_all.dtype)
    eng = _engine_of(adapter, n_img=1, height=int(imagetight.shape[-2]), width=int(imagetight.shape[-1]), num_inference_steps=num_inference_steps,
                     guidance_scale=guidance_scale, enc_len=ip_embeds.shape[1], controlnet=controlnet, controlnet_enc_len=text_embeddings.shape[1])
    eng.set_conditioning(ip_embeds.to(dev, dtype))
    eng.set_control(text_embeddings.to(dev, dtype), imagetight.to(dev, dtype), 1.0)
    eng.set_frozen(latents_all.to(dev, torch.float32), my_mask, frozen_steps)
    latents = eng.run(my_bg)[-1].to(dtype)
    image = vae.decode(1 / 0.18215 * latents).sample
    image = (image.float() / 2 + 0.5).clamp(0, 1).detach().cpu().permute(0, 2, 3, 1).numpy()
    return latents, (image * 255).round().astype("uint8")


@torch.no_grad()
def generate_final_images(basever, processor, controlnetpipe, overall_prompts, overall_negative_prompts, single_obj_img_lists, height, width, bg_seeds,
                          inp_masks, input_imgs, adapter, latents_all_list, input_embeddings_list, num_inference_steps, frozen_steps, guidance_scale=7.5):
    """Stage 2 of the non-XL branches for a LIST of turns in ONE engine run — what ``final_image_generation`` does once per turn (reference
    ``models/pipelines.py:592-857``; the caller's loop ``theatergen.py:448-484`` needs nothing from one turn in the next), with the turns in the batch
    dimension of the captured ControlNet + UNet step.  One entry per turn in every list; returns a list with, per turn, the pair
    ``final_image_generation`` returns for it: ``(latents [1, C, h, w], images uint8 ndarray [1, H, W, 3])``.

    Per turn, on the host, as in the single call: the frozen mask from ``inp_masks[i]``, ``processor(np.array(input_imgs[i]))`` and the control
    image preparation, the conditioning rows of ``overall_prompts[i]`` with the image tokens of ``single_obj_img_lists[i][0]``; the three random
    draws (posterior noise, re-noising noise, background latents) come from ``torch.Generator(device).manual_seed(bg_seeds[i])`` in the reference's
    order with the single call's shapes and dtype, so they are bit-equal to what the single call draws for that turn alone.
    ``latents_all_list[i]`` is overwritten as the single call overwrites ``latents_all`` (row 0 the background noise, rows 1.. the frozen rows).
    IP scale 0.1 as one number.  Shared by the turns: one upload of the pasted images as uint8 HWC and one ``tg_image_from_u8``, one VAE encode,
    one ``add_noise``, one engine (``n_img`` = the number of turns; rows ``[neg_0 .. neg_{n-1} ; pos_0 .. pos_{n-1}]``), one ``run``, one VAE decode,
    one ``tg_image_to_u8`` and one device-to-host copy of ``[n, H, W, 3]`` bytes.

    Refused before any device work or side effect: ``basever='xl'`` (NotImplementedError: its stage 2 runs another UNet, scheduler and adapter, run
    ``final_image_generation(..., basever='xl')`` per turn); lists of unequal length or an empty list, turns whose images, masks, text embeddings or
    ``latents_all`` differ in shape (ValueError); a foreign ControlNet / UNet (TypeError, the single call's messages).  The LENGTH of the conditioning
    rows (text + image tokens) and the size of the prepared control images are only known once every turn's ``encode_prompt`` / ``get_image_embeds`` /
    ``processor`` has run: turns that differ there are a ValueError after that per-turn work, still before ``set_scale``, the ``latents_all_list``
    writes and the engine."""
    import numpy as np
    if basever == "xl":
        raise NotImplementedError("generate_final_images: the SDXL stage 2 runs controlnetpipe.unet with a T2I-Adapter and Euler-ancestral steps "
                                  "(models/pipelines.py:654-700); run final_image_generation(..., basever='xl') per turn")
    lists = {"overall_prompts": overall_prompts, "overall_negative_prompts": overall_negative_prompts, "single_obj_img_lists": single_obj_img_lists,
             "bg_seeds": bg_seeds, "inp_masks": inp_masks, "input_imgs": input_imgs, "latents_all_list": latents_all_list,
             "input_embeddings_list": input_embeddings_list}
    n = len(overall_prompts)
    if n == 0 or any(len(v) != n for v in lists.values()):
        raise ValueError("generate_final_images: " + ", ".join(f"{len(v)} {k}" for k, v in lists.items()) + ": one entry per turn, at least one turn")
    pasted = [np.asarray(im) for im in input_imgs]
    if any(a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 for a in pasted):
        raise ValueError("generate_final_images: every input image must be uint8 RGB [H, W, 3], got " + ", ".join(f"{a.dtype} {a.shape}" for a in pasted))
    if any(a.shape != pasted[0].shape for a in pasted):
        raise ValueError("generate_final_images: the turns' input images differ in size: " + ", ".join(str(a.shape[:2]) for a in pasted))
    if any(tuple(m.size) != tuple(inp_masks[0].size) for m in inp_masks):
        raise ValueError("generate_final_images: the turns' masks differ in size: " + ", ".join(str(tuple(m.size)) for m in inp_masks))
    if any(not lst for lst in single_obj_img_lists):
        raise ValueError("generate_final_images: every turn needs its first character image (single_obj_img_lists[i][0])")
    texts = [emb[0] for emb in input_embeddings_list]
    if any(tuple(t.shape) != tuple(texts[0].shape) for t in texts):
        raise ValueError("generate_final_images: the turns' text embeddings differ in shape: " + ", ".join(str(tuple(t.shape)) for t in texts))
    if any(tuple(la.shape) != tuple(latents_all_list[0].shape) for la in latents_all_list):
        raise ValueError("generate_final_images: the turns' latents_all differ in shape: " + ", ".join(str(tuple(la.shape)) for la in latents_all_list))
    unet = _own_unet(adapter, "generate_final_images")
    from .controlnet import ControlNetModel
    controlnet = controlnetpipe.controlnet
    if not isinstance(controlnet, ControlNetModel):
        raise TypeError("theatergen_amd.pipelines.generate_final_images: controlnetpipe.controlnet must be a theatergen_amd.controlnet.ControlNetModel "
                        f"(INTEGRATION.md, stage 2), got {type(controlnet).__name__}")
    vae, scheduler, dtype, dev = adapter.pipe.vae, adapter.pipe.scheduler, unet.dtype, unet.device
    h8, w8 = int(height / 8), int(width / 8)
    # ---- per turn, on the host: frozen mask, conditioning rows, control image (the single call's expressions and call order)
    masks, rows, controls = [], [], []
    for i in range(n):
        m = np.array(inp_masks[i].resize((h8, w8)).convert("L")).astype(np.float32) / 255.0
        m[m > 0] = 1
        masks.append(torch.from_numpy(1 - m))
        rows.append(_text_and_image_rows(adapter, overall_prompts[i], overall_negative_prompts[i], single_obj_img_lists[i][0]))          # [2, L, D]
        controls.append(_control_image(controlnetpipe, processor(np.array(input_imgs[i])), width, height, dev, dtype))               # [2, 3, H, W]
    if any(tuple(r.shape) != tuple(rows[0].shape) for r in rows):
        raise ValueError("generate_final_images: the turns' conditioning rows differ in length: " + ", ".join(str(tuple(r.shape)) for r in rows))
    if any(tuple(c.shape) != tuple(controls[0].shape) for c in controls):
        raise ValueError("generate_final_images: the turns' control images differ in size: " + ", ".join(str(tuple(c.shape)) for c in controls))
    adapter.set_scale(0.1)
    scheduler.set_timesteps(num_inference_steps)
    # ---- frozen latents: the n pasted images cross to the device as bytes, one encode, every turn's draws from its own device generator
    u8 = torch.from_numpy(np.ascontiguousarray(np.stack(pasted))).to(dev)
    dist = vae.encode(ops.image_from_u8(u8, dtype, range_mode=1)).latent_dist
    gens = [torch.Generator(dev).manual_seed(s) for s in bg_seeds]
    post_shape = (1, dist.parameters.shape[1] // 2) + tuple(dist.parameters.shape[2:])
    post_noise = torch.cat([torch.randn(post_shape, generator=g, device=dev, dtype=dtype) for g in gens])
    init_latents = vae.config.scaling_factor * dist.sample(noise=post_noise)                                                        # [n, C, h, w]
    noise = torch.cat([torch.randn(post_shape, generator=g, device=dev, dtype=dtype) for g in gens])
    my_latents = scheduler.add_noise(init_latents[None], noise[None], scheduler.timesteps)                                          # [steps, n, C, h, w]
    my_bg = torch.cat([torch.randn((1, unet.config.in_channels, h8, w8), generator=g, device=dev, dtype=dtype) for g in gens]) * float(scheduler.init_noise_sigma)
    for i, la in enumerate(latents_all_list):
        la[0] = my_bg[i:i + 1].to(la.device, la.dtype)
        la[1:] = my_latents[:, i:i + 1].to(la.device, la.dtype)
    # ---- one engine, the turns in its batch dimension: negatives first, in turn order
    enc = torch.cat([r[:1] for r in rows] + [r[1:] for r in rows], dim=0)
    cn_enc = torch.cat([t[:1] for t in texts] + [t[1:] for t in texts], dim=0)
    cn_cond = torch.cat([c[:1] for c in controls] + [c[1:] for c in controls], dim=0)
    eng = _engine_of(adapter, n_img=n, height=int(cn_cond.shape[-2]), width=int(cn_cond.shape[-1]), num_inference_steps=num_inference_steps,
                     guidance_scale=guidance_scale, enc_len=enc.shape[1], controlnet=controlnet, controlnet_enc_len=cn_enc.shape[1])
    eng.set_conditioning(enc.to(dev, dtype))
    eng.set_control(cn_enc.to(dev, dtype), cn_cond.to(dev, dtype), 1.0)
    eng.set_frozen(torch.cat([la.to(dev, torch.float32) for la in latents_all_list], dim=1), torch.stack(masks).to(device=dev, dtype=torch.float32),
                   frozen_steps)
    latents = eng.run(my_bg)[-1].to(dtype)
    images = ops.image_to_u8(vae.decode(1 / 0.18215 * latents).sample).cpu().numpy()                                                # [n, H, W, 3] bytes
    return [(latents[i:i + 1], images[i:i + 1]) for i in range(n)]


@torch.no_grad()
def decode(vae, latents):
    """reference ``models/pipelines.py:163-173``: ``vae.decode(latents / 0.18215)`` -> ``(image / 2 + 0.5).clamp(0, 1)`` -> uint8 ``[n, H, W, 3]`` on the host"""
    image = vae.decode(1 / 0.18215 * latents).sample
    image = (image.float() / 2 + 0.5).clamp(0, 1).detach().cpu().permute(0, 2, 3, 1).numpy()
    return (image * 255).round().astype("uint8")


@torch.no_grad()
def generate(adapter, model_dict, latents, input_embeddings, num_inference_steps, guidance_scale=7.5, no_set_timesteps=False, scheduler_key='scheduler'):
    """reference ``models/pipelines.py:493-521``: the plain CFG loop over WHATEVER scheduler ``adapter.pipe.scheduler`` is (DDIM, DPM-Solver++ multistep,
    Euler), then ``decode``; returns ``(latents, images uint8 [n, H, W, 3])``.  ``input_embeddings`` = ``(text_embeddings [2n, L, D] negatives first,
    uncond, cond)``; only the first is read, as there.  On the engine: ``len(timesteps)`` replays of one captured step, no per-step host work.
    ``no_set_timesteps=True`` walks the scheduler's CURRENT ``timesteps`` (a caller's own grid) and leaves them in place; their number must be
    ``num_inference_steps`` (``ValueError``), since the engine's tables are built for that count.  ``scheduler_key`` is accepted and unused, as there."""
    unet = _own_unet(adapter, "generate")
    scheduler = adapter.pipe.scheduler
    text_embeddings = input_embeddings[0]
    timesteps = None
    if no_set_timesteps:
        timesteps = scheduler.timesteps.clone()
        if int(timesteps.numel()) != int(num_inference_steps):
            raise ValueError(f"generate(no_set_timesteps=True): the scheduler holds {int(timesteps.numel())} timesteps, num_inference_steps is {num_inference_steps}")
    h8, w8 = latents.shape[-2], latents.shape[-1]
    eng = _engine_of(adapter, n_img=latents.shape[0], height=8 * h8, width=8 * w8, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                     enc_len=text_embeddings.shape[1], timesteps=timesteps)
    if timesteps is not None and not torch.equal(scheduler.timesteps, timesteps):
        scheduler.timesteps = timesteps                              # building the engine's tables called set_timesteps: the caller's grid stays
    eng.set_conditioning(text_embeddings.to(eng.dev, eng.dt))
    out = eng.run(latents)[-1].to(latents.dtype, copy=True)          # a copy: the history row is the engine's buffer, the next run rewrites it
    return out, decode(adapter.pipe.vae, out.to(unet.dtype))


def latent_backward_guidance(*args, **kwargs):
    """reference ``models/pipelines.py:62-128`` (same signature); implemented in ``theatergen_amd.backward``"""
    from .backward import latent_backward_guidance as impl
    return impl(*args, **kwargs)
