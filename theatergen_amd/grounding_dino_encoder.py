"""GroundingDINO's fusion / deformable encoder on the native kernels (``transformers``' ``GroundingDinoEncoder``; reference ``utils/detector.py``: the
``detect`` step of the character loop).

Token-major, storage dtype (bf16 / fp16) throughout.  Per layer, following ``transformers`` 5.x, quirks included:

* FUSION (``GroundingDinoFusionLayer``): LayerNorm on both sides; one GEMM per side gives q | V^T (vision) and k | V^T (text) of the bidirectional
  attention (4 heads of dim 256 at GroundingDINO-T size); ``ops.attention_wide`` runs vision -> text with the text key mask and text -> vision with
  the vision key mask (the score matrix of the second is the transpose of the first: the text "keys" are its queries and the vision "queries" its
  keys; the query side is a handful of tokens, so the key range is split until the grid fills the chip).  Both output projections carry the layer-scale vectors
  ``vision_param`` / ``text_param`` folded into their weights and biases at load, and the residual is the NORMED features, as in ``transformers``.
  ``transformers`` subtracts the global / row max of the scores and clamps them to +-50 000 before its softmaxes: both are softmax-invariant while
  the spread of a row's scores stays under 50 000 (scores here are O(10)), so neither is reproduced.
* TEXT ENHANCER: q | k from x + pos (the sinusoidal embedding of ``text_position_ids``, computed once per forward in fp32 torch and shared by the
  layers, cast to the ids' dtype as ``transformers`` does: q | k = x W^T + pos W^T, the second product added through the GEMM's residual), v^T
  from x, ``ops.attention`` with ``text_self_attention_masks`` as an additive fp32 mask, output projection + residual, LayerNorm, fc1 + ReLU,
  fc2 + residual, LayerNorm.
  The mask is ``transformers``' arithmetic on what ``GroundingDinoEncoder.forward`` receives: a True entry is a large negative bias, and a row that is
  True everywhere attends uniformly (there the bias absorbs the scores in fp32; -1e30 does here what finfo.min does there).
* DEFORMABLE: x + pos, one GEMM gives offsets | logits, one GEMM the values, ``ops.msdeform_attn`` with the padding mask (a masked token samples as
  zeros: no pass over the values), output projection + residual, LayerNorm, fc1 + ReLU, fc2 + residual, LayerNorm.

Every "+ residual, LayerNorm" of the text enhancer and the deformable layer is ``ops.layernorm_add``: the sublayer's output and the residual are
added in fp32 inside the LayerNorm kernel.  A residual GEMM epilogue would round the sum to the storage dtype before the statistics: on the text states
that rounding alone took the fp16 maximum error from 0.9e-3 to 1.5e-3 of the largest element.

Reference points are ``GroundingDinoEncoder.get_reference_points`` in fp32 torch on the device, cached per ``valid_ratios`` tensor.  Nothing in
``forward`` synchronises with the host.  Parameter names are those of ``transformers.GroundingDinoModel`` under ``encoder.``.  Inference only.
"""
import math

import torch
import torch.nn as nn

from . import ops

PREFIX = "encoder."
_BIG = 1e30          # additive mask of the text enhancer: finite, so mask * log2(e) stays in fp32 range and an all-masked row is uniform, not NaN

_LINEAR = {
    "text_enhancer_layer": ["self_attn.query", "self_attn.key", "self_attn.value", "self_attn.out_proj", "fc1", "fc2", "layer_norm_before",
                            "layer_norm_after"],
    "fusion_layer": ["layer_norm_vision", "layer_norm_text", "attn.vision_proj", "attn.text_proj", "attn.values_vision_proj",
                     "attn.values_text_proj", "attn.out_vision_proj", "attn.out_text_proj"],
    "deformable_layer": ["self_attn.sampling_offsets", "self_attn.attention_weights", "self_attn.value_proj", "self_attn.output_proj",
                         "self_attn_layer_norm", "fc1", "fc2", "final_layer_norm"],
}


def expected_names(config):
    """The parameter names ``from_state_dict`` takes: ``GroundingDinoModel``'s state dict under ``encoder.``."""
    names = []
    for i in range(int(config.encoder_layers)):
        for part, lins in _LINEAR.items():
            for lin in lins:
                names += [f"{PREFIX}layers.{i}.{part}.{lin}.{s}" for s in ("weight", "bias")]
        names += [f"{PREFIX}layers.{i}.fusion_layer.vision_param", f"{PREFIX}layers.{i}.fusion_layer.text_param"]
    return set(names)


def check_config(config):
    """NotImplementedError naming the field for a config outside the kernels' envelope"""
    d, heads, ffn = int(config.d_model), int(config.encoder_attention_heads), int(config.encoder_ffn_dim)
    bad = []
    if heads < 1 or d % heads or d // heads != 32:
        bad.append(f"d_model / encoder_attention_heads = {d} / {heads} (deformable head dim 32)")
    if int(config.encoder_n_points) != 4:
        bad.append(f"encoder_n_points {config.encoder_n_points} (4)")
    if not 1 <= int(config.num_feature_levels) <= 4:
        bad.append(f"num_feature_levels {config.num_feature_levels} (1 .. 4)")
    h2 = heads // 2
    if h2 < 1 or (ffn // 2) % h2 or (ffn // 2) // h2 != 256:
        bad.append(f"encoder_ffn_dim / encoder_attention_heads = {ffn} / {heads} (fusion head dim 256)")
    if h2 < 1 or d % h2 or (d // h2) % 8 or d // h2 > 160:
        bad.append(f"d_model / (encoder_attention_heads / 2) = {d} / {h2} (text-enhancer head dim: a multiple of 8 up to 160)")
    if getattr(config, "activation_function", "relu") != "relu":
        bad.append(f"activation_function {config.activation_function} (relu)")
    if bad:
        raise NotImplementedError("GroundingDinoFusionEncoder: " + "; ".join(bad) + " has no kernel")


def _pad8(n):
    return (int(n) + 7) // 8 * 8


class GroundingDinoFusionEncoder:
    """``forward(**kwargs of GroundingDinoEncoder.forward)`` -> ``GroundingDinoEncoderOutput`` with tensors in the storage dtype."""

    def __init__(self, config, params, device="cuda", dtype=torch.bfloat16):
        check_config(config)
        want = expected_names(config)
        missing, unexpected = sorted(want - set(params)), sorted(set(params) - want)
        if missing or unexpected:
            raise RuntimeError(f"state dict mismatch: missing {missing[:5]}... unexpected {unexpected[:5]}...")
        if dtype not in (torch.bfloat16, torch.float16):
            raise RuntimeError(f"GroundingDinoFusionEncoder: storage dtype {dtype} unsupported (bf16 / fp16)")
        self.config = config
        self.device, self.dtype = torch.device(device), dtype
        self.d = int(config.d_model)
        self.heads = int(config.encoder_attention_heads)
        self.levels = int(config.num_feature_levels)
        self.E = int(config.encoder_ffn_dim) // 2
        self.eps = float(getattr(config, "layer_norm_eps", 1e-5))
        f32 = {k: v.detach().to(device=self.device, dtype=torch.float32) for k, v in params.items()}
        st = lambda t: t.to(dtype).contiguous()                                                       # noqa: E731
        self.layers = []
        for i in range(int(config.encoder_layers)):
            g = lambda name: f32[f"{PREFIX}layers.{i}.{name}"]                                       # noqa: E731
            wb = lambda name: (st(g(name + ".weight")), st(g(name + ".bias")))                       # noqa: E731
            cat = lambda names, s: st(torch.cat([g(n + s) for n in names], 0))                       # noqa: E731
            fu, te, de = "fusion_layer.", "text_enhancer_layer.", "deformable_layer."
            vp, tp = g(fu + "vision_param"), g(fu + "text_param")
            self.layers.append(dict(
                ln_v=wb(fu + "layer_norm_vision"), ln_t=wb(fu + "layer_norm_text"),
                w_vis=cat([fu + "attn.vision_proj", fu + "attn.values_vision_proj"], ".weight"),
                b_vis=cat([fu + "attn.vision_proj", fu + "attn.values_vision_proj"], ".bias"),
                w_txt=cat([fu + "attn.text_proj", fu + "attn.values_text_proj"], ".weight"),
                b_txt=cat([fu + "attn.text_proj", fu + "attn.values_text_proj"], ".bias"),
                # layer scale folded in fp32, rounded once: vision_param * (W o + b) = (diag(vision_param) W) o + vision_param * b
                wo_v=st(vp[:, None] * g(fu + "attn.out_vision_proj.weight")), bo_v=st(vp * g(fu + "attn.out_vision_proj.bias")),
                wo_t=st(tp[:, None] * g(fu + "attn.out_text_proj.weight")), bo_t=st(tp * g(fu + "attn.out_text_proj.bias")),
                te_wqkv=cat([te + "self_attn.query", te + "self_attn.key", te + "self_attn.value"], ".weight"),
                te_bqkv=cat([te + "self_attn.query", te + "self_attn.key", te + "self_attn.value"], ".bias"),
                te_wqk=cat([te + "self_attn.query", te + "self_attn.key"], ".weight"),
                te_o=wb(te + "self_attn.out_proj"), te_ln1=wb(te + "layer_norm_before"), te_fc1=wb(te + "fc1"), te_fc2=wb(te + "fc2"),
                te_ln2=wb(te + "layer_norm_after"),
                de_wol=cat([de + "self_attn.sampling_offsets", de + "self_attn.attention_weights"], ".weight"),
                de_bol=cat([de + "self_attn.sampling_offsets", de + "self_attn.attention_weights"], ".bias"),
                de_v=wb(de + "self_attn.value_proj"), de_o=wb(de + "self_attn.output_proj"), de_ln1=wb(de + "self_attn_layer_norm"),
                de_fc1=wb(de + "fc1"), de_fc2=wb(de + "fc2"), de_ln2=wb(de + "final_layer_norm")))
        self._ref_cache = {}
        self._buffers = {}
        self.op_calls = 0              # calls into the native library so far (a tally kept here, not a count of kernel launches)
        self.fusion_key_splits = None  # None: _text_to_vision_splits' own rule; an int is passed on as ``key_splits`` (0 = the library's planner)
        self.taps = None               # a list: receives ("fusion", layer, vision, text) after every fusion layer (the tests' per-stage checks)

    @classmethod
    def from_state_dict(cls, config, state_dict, device="cuda", dtype=torch.bfloat16):
        """``state_dict``: the ``encoder.`` entries of a ``GroundingDinoModel`` state dict (a whole state dict of that model or of
        ``GroundingDinoForObjectDetection`` is filtered to them).  A missing or unexpected name is a RuntimeError."""
        pre = "model." if any(k.startswith("model." + PREFIX) for k in state_dict) else ""
        sub = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre + PREFIX)}
        return cls(config, sub, device, dtype)

    # ---- per-forward constants ---------------------------------------------------------------------------------------------------------------
    def reference_points(self, shapes, valid_ratios):
        """``GroundingDinoEncoder.get_reference_points`` -> fp32 [B, Nv, L, 2], cached per ``valid_ratios`` TENSOR (same object, same ``_version``): comparing
        contents would need a host synchronisation; a caller who passes a new tensor each time pays the small fp32 torch computation."""
        key = (id(valid_ratios), valid_ratios._version, tuple(shapes))
        hit = self._ref_cache.get(key)
        if hit is None or hit[0] is not valid_ratios:
            if len(self._ref_cache) >= 8:
                self._ref_cache.clear()
            vr = valid_ratios.to(device=self.device, dtype=torch.float32)
            pts = []
            for level, (h, w) in enumerate(shapes):
                ry, rx = torch.meshgrid(torch.linspace(0.5, h - 0.5, h, dtype=torch.float32, device=self.device),
                                        torch.linspace(0.5, w - 0.5, w, dtype=torch.float32, device=self.device), indexing="ij")
                ry = ry.reshape(-1)[None] / (vr[:, None, level, 1] * h)
                rx = rx.reshape(-1)[None] / (vr[:, None, level, 0] * w)
                pts.append(torch.stack((rx, ry), -1))
            ref = (torch.cat(pts, 1)[:, :, None] * vr[:, None]).contiguous()
            hit = (valid_ratios, ref)
            self._ref_cache[key] = hit
        return hit[1]

    def text_position_embedding(self, position_ids):
        """``encode_sinusoidal_position_embedding(text_position_ids[..., None], num_pos_feats=d_model)`` in fp32 -> [B * Lt, d] in the storage dtype.
        As there, the result is cast to the dtype of ``position_ids``: the integer ids ``GroundingDinoModel`` passes TRUNCATE the embedding to -1 / 0 / 1
        (cos(0) = 1 survives, almost everything else becomes 0).  The golden pins it."""
        ids = position_ids.to(self.device)
        dim_t = torch.arange(self.d, dtype=torch.float32, device=self.device)
        dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / self.d)
        e = ids[..., None] * (2 * math.pi) / dim_t
        e = torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-2).to(ids.dtype)
        return e.reshape(-1, self.d).to(self.dtype).contiguous()

    def _zeros(self, name, shape):
        """a persistent zero-initialised buffer per (name, shape): the kernels that write it never touch its padding, which stays zero"""
        key = (name,) + tuple(shape)
        buf = self._buffers.get(key)
        if buf is None:
            if len(self._buffers) >= 32:
                self._buffers.clear()
            buf = torch.zeros(shape, dtype=self.dtype, device=self.device)
            self._buffers[key] = buf
        return buf

    def _text_to_vision_splits(self, B, Lt, n_keys):
        """Key splits of the text -> vision attention.  Its unsplit grid is ceil(Lt / 128) x heads x batch workgroups (4 at batch 1) that would each walk
        all n_keys / 32 key tiles (416 at 800 x 800).  The library's planner (``key_splits=0``) stops at 8 splits, a cap chosen for the VAE's 64-workgroup
        grids; here the splits are what fills the 256 CUs once, every split keeping at least 4 tiles.  ``fusion_key_splits`` overrides (0 = the planner)."""
        if self.fusion_key_splits is not None:
            return int(self.fusion_key_splits)
        blocks = ((Lt + 127) // 128) * (self.heads // 2) * B
        return max(1, min(256 // max(blocks, 1), (n_keys // 32) // 4, 64))

    # ---- the three parts of a layer ------------------------------------------------------------------------------------------------------------
    def _fusion(self, ly, v, t, B, Nv, Lt, kmask_v, kmask_t):
        d, E, Hf = self.d, self.E, self.heads // 2
        Nvp, Ltp = _pad8(Nv), _pad8(Lt)
        yv = ops.layernorm(v, ly["ln_v"][0], ly["ln_v"][1], self.eps)
        yt = ops.layernorm(t, ly["ln_t"][0], ly["ln_t"][1], self.eps)
        # q (vision) / k (text) rows with 8 spare rows behind the last batch item: a key tile of the padded length reads past an item's rows (into the
        # next item's, or the spare ones), and those keys are masked.  V^T columns [len, padded len) stay zero: 0 * V must not be NaN
        qv = self._zeros("fu_qv", (B * Nv + 8, E))
        kt = self._zeros("fu_kt", (B * Lt + 8, E))
        vvt = self._zeros("fu_vvt", (B, E, Nvp))
        vtt = self._zeros("fu_vtt", (B, E, Ltp))
        ops.gemm(yv, ly["w_vis"], B * Nv, 2 * E, d, bias=ly["b_vis"], rows_per_batch=Nv, out=qv[:B * Nv], n_split=E, out_t=vvt, ldt=Nvp)
        ops.gemm(yt, ly["w_txt"], B * Lt, 2 * E, d, bias=ly["b_txt"], rows_per_batch=Lt, out=kt[:B * Lt], n_split=E, out_t=vtt, ldt=Ltp)
        scale = 256 ** -0.5
        ov = torch.empty((B * Nv, E), dtype=self.dtype, device=self.device)
        ot = torch.empty((B * Lt, E), dtype=self.dtype, device=self.device)
        ops.attention_wide(qv, E, Nv * E, kt, E, Lt * E, vtt, Ltp, E * Ltp, Ltp, B, Hf, 256, Nv, scale, ov, E, Nv * E, key_mask=kmask_t)
        ops.attention_wide(kt, E, Lt * E, qv, E, Nv * E, vvt, Nvp, E * Nvp, Nvp, B, Hf, 256, Lt, scale, ot, E, Lt * E,
                           key_splits=self._text_to_vision_splits(B, Lt, Nvp), key_mask=kmask_v)
        v = ops.linear(ov, ly["wo_v"], ly["bo_v"], res=yv)
        t = ops.linear(ot, ly["wo_t"], ly["bo_t"], res=yt)
        self.op_calls += 8
        return v, t

    def _text_enhancer(self, ly, t, pos, B, Lt, add_mask):
        d, Ht = self.d, self.heads // 2
        hd = d // Ht
        ldt = _pad8(Lt)
        qk0 = torch.empty((B * Lt, 2 * d), dtype=self.dtype, device=self.device)
        vt = self._zeros("te_vt", (B, d, ldt))
        ops.gemm(t, ly["te_wqkv"], B * Lt, 3 * d, d, bias=ly["te_bqkv"], rows_per_batch=Lt, out=qk0, n_split=2 * d, out_t=vt, ldt=ldt)
        qk = ops.linear(pos, ly["te_wqk"], None, res=qk0)
        o = torch.empty((B * Lt, d), dtype=self.dtype, device=self.device)
        ops.attention(qk, 2 * d, Lt * 2 * d, qk[:, d:], 2 * d, Lt * 2 * d, vt, ldt, d * ldt, Lt, B, Ht, hd, Lt, float(hd) ** -0.5, o, d, Lt * d,
                      mask=add_mask)
        t = ops.layernorm_add(ops.linear(o, ly["te_o"][0], ly["te_o"][1]), t, ly["te_ln1"][0], ly["te_ln1"][1], self.eps)
        y = ops.relu(ops.linear(t, ly["te_fc1"][0], ly["te_fc1"][1]))
        y = ops.linear(y, ly["te_fc2"][0], ly["te_fc2"][1])
        self.op_calls += 9
        return ops.layernorm_add(y, t, ly["te_ln2"][0], ly["te_ln2"][1], self.eps)

    def _deformable(self, ly, v, pos, B, Nv, shapes, ref, vmask):
        d, L = self.d, self.levels
        n_off = self.heads * L * 8
        xq = ops.add(v, pos)
        ol = ops.linear(xq, ly["de_wol"], ly["de_bol"])                                              # offsets | logits
        val = ops.linear(v, ly["de_v"][0], ly["de_v"][1])
        o = torch.empty((B * Nv, d), dtype=self.dtype, device=self.device)
        ops.msdeform_attn(val, d, Nv * d, shapes, ol, ol.stride(0), ol[:, n_off:], ol.stride(0), ref, B, self.heads, Nv, o, d, Nv * d,
                          value_mask=vmask)
        v = ops.layernorm_add(ops.linear(o, ly["de_o"][0], ly["de_o"][1]), v, ly["de_ln1"][0], ly["de_ln1"][1], self.eps)
        y = ops.relu(ops.linear(v, ly["de_fc1"][0], ly["de_fc1"][1]))
        y = ops.linear(y, ly["de_fc2"][0], ly["de_fc2"][1])
        self.op_calls += 10
        return ops.layernorm_add(y, v, ly["de_ln2"][0], ly["de_ln2"][1], self.eps)

    # ---- forward -----------------------------------------------------------------------------------------------------------------------------------
    def forward(self, vision_features, vision_attention_mask, vision_position_embedding, spatial_shapes=None, spatial_shapes_list=None,
                level_start_index=None, valid_ratios=None, text_features=None, text_attention_mask=None, text_position_embedding=None,
                text_self_attention_masks=None, text_position_ids=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                **kwargs):
        from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoEncoderOutput
        if output_attentions:
            raise NotImplementedError("GroundingDinoFusionEncoder: output_attentions=True (no attention matrix exists in memory)")
        if not vision_features.is_cuda:
            raise RuntimeError("theatergen_amd GroundingDINO encoder runs on the GPU only (no CPU fallback)")
        if spatial_shapes_list is None or valid_ratios is None or text_features is None or text_self_attention_masks is None:
            raise ValueError("GroundingDinoFusionEncoder.forward: spatial_shapes_list, valid_ratios, text_features and text_self_attention_masks are "
                             "required")
        if text_position_embedding is not None and text_position_ids is None:
            raise NotImplementedError("GroundingDinoFusionEncoder: text_position_embedding without text_position_ids")
        shapes = [(int(h), int(w)) for h, w in spatial_shapes_list]
        if len(shapes) != self.levels:
            raise ValueError(f"GroundingDinoFusionEncoder: {len(shapes)} levels given, the config has {self.levels}")
        B, Nv, d = vision_features.shape
        Lt = int(text_features.shape[1])
        if d != self.d or sum(h * w for h, w in shapes) != Nv or text_features.shape[0] != B or text_features.shape[2] != d:
            raise ValueError(f"GroundingDinoFusionEncoder: vision {tuple(vision_features.shape)} / text {tuple(text_features.shape)} do not match "
                             f"d_model {self.d} and the levels {shapes}")
        with torch.no_grad():
            dev, dt = self.device, self.dtype
            v = vision_features.to(device=dev, dtype=dt).reshape(B * Nv, d).contiguous()
            t = text_features.to(device=dev, dtype=dt).reshape(B * Lt, d).contiguous()
            pos_v = vision_position_embedding.to(device=dev, dtype=dt).reshape(B * Nv, d).contiguous()
            if text_position_ids is None:
                text_position_ids = torch.arange(Lt, device=dev, dtype=torch.float32)[None].expand(B, Lt)
            pos_t = self.text_position_embedding(text_position_ids)
            ref = self.reference_points(shapes, valid_ratios)
            # masks, once per forward: True / 1 = padding
            vpad = (vision_attention_mask.to(dev).bool() if vision_attention_mask is not None
                    else torch.zeros((B, Nv), dtype=torch.bool, device=dev))
            tpad = (text_attention_mask.to(dev).bool() if text_attention_mask is not None
                    else torch.zeros((B, Lt), dtype=torch.bool, device=dev))
            vmask = vpad.to(torch.uint8).contiguous()
            kmask_v = torch.ones((B, _pad8(Nv)), dtype=torch.uint8, device=dev)
            kmask_v[:, :Nv] = vmask
            kmask_t = torch.ones((B, _pad8(Lt)), dtype=torch.uint8, device=dev)
            kmask_t[:, :Lt] = tpad.to(torch.uint8)
            add_mask = (text_self_attention_masks.to(dev).bool().to(torch.float32) * -_BIG).reshape(B, 1, Lt, Lt).contiguous()

            vis_states, txt_states = [], []
            shape_v, shape_t = (B, Nv, d), (B, Lt, d)
            for i, ly in enumerate(self.layers):
                if output_hidden_states:
                    vis_states.append(v.reshape(shape_v))
                    txt_states.append(t.reshape(shape_t))
                v, t = self._fusion(ly, v, t, B, Nv, Lt, kmask_v, kmask_t)
                if self.taps is not None:
                    self.taps.append(("fusion", i, v.reshape(shape_v), t.reshape(shape_t)))
                t = self._text_enhancer(ly, t, pos_t, B, Lt, add_mask)
                v = self._deformable(ly, v, pos_v, B, Nv, shapes, ref, vmask)
                if self.taps is not None:
                    self.taps.append(("layer", i, v.reshape(shape_v), t.reshape(shape_t)))
            v, t = v.reshape(shape_v), t.reshape(shape_t)
            if output_hidden_states:
                vis_states.append(v)
                txt_states.append(t)
        out = GroundingDinoEncoderOutput(last_hidden_state_vision=v, last_hidden_state_text=t,
                                         vision_hidden_states=tuple(vis_states) if output_hidden_states else None,
                                         text_hidden_states=tuple(txt_states) if output_hidden_states else None, attentions=None)
        if return_dict is not None and not return_dict:
            return tuple(x for x in (v, t, out.vision_hidden_states, out.text_hidden_states) if x is not None)
        return out

    __call__ = forward

    # ---- transformers integration --------------------------------------------------------------------------------------------------------------
    def attach(self, hf_model):
        """Make a ``transformers`` ``GroundingDinoModel`` / ``GroundingDinoForObjectDetection`` use this encoder: its ``encoder`` is replaced by a thin
        module that casts in, runs this encoder and casts out to the dtype of the model behind it.  Composes with ``GroundingDinoVisionFront.attach``."""
        core = hf_model.model if hasattr(hf_model, "model") and hasattr(hf_model.model, "encoder") else hf_model
        if not hasattr(core, "encoder") or not hasattr(core, "decoder"):
            raise TypeError("attach: a transformers GroundingDinoModel or GroundingDinoForObjectDetection expected")
        p0 = next(iter(core.decoder.parameters()), None)
        core.encoder = _EncoderModule(self, p0.dtype if p0 is not None else self.dtype)
        return hf_model


class _EncoderModule(nn.Module):
    def __init__(self, encoder, out_dtype):
        super().__init__()
        self._encoder, self.out_dtype = [encoder], out_dtype       # a list: the encoder is no nn.Module and is not to be registered

    def forward(self, **kwargs):
        out = self._encoder[0].forward(**kwargs)
        cast = lambda x: None if x is None else tuple(y.to(self.out_dtype) for y in x) if isinstance(x, tuple) else x.to(self.out_dtype)   # noqa: E731
        if isinstance(out, tuple):
            return tuple(cast(x) for x in out)
        return type(out)(last_hidden_state_vision=cast(out.last_hidden_state_vision), last_hidden_state_text=cast(out.last_hidden_state_text),
                         vision_hidden_states=cast(out.vision_hidden_states), text_hidden_states=cast(out.text_hidden_states), attentions=None)
