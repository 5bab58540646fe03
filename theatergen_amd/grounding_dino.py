"""GroundingDINO's vision front on the native kernels: the Swin backbone, the ``input_proj_vision`` levels and the sine position embeddings
(reference ``utils/detector.py``: the ``detect`` step of the character loop, one Swin-T forward per character).

Token-major throughout, tokens in IMAGE order.  Patch embedding = ``pixel_unshuffle(4)`` + one K = 48 GEMM + LayerNorm.  A Swin block is LayerNorm, ONE
q | k | v projection GEMM, ``ops.attention_swin`` (pad to a multiple of 7, roll, window partition, learned bias, shift mask and their inverses are
address arithmetic inside the kernel: no window-ordered copy of the tokens exists), o_proj + residual, LayerNorm, fc1 + exact GELU, fc2 + residual.
Patch merging gathers the 2 x 2 neighbours by torch indexing (data movement), then LayerNorm and the bias-free reduction GEMM.  The projection levels are
1 x 1 convolutions as GEMMs (the extra level: the stride-2 3 x 3 implicit GEMM) + GroupNorm(32).  The position embeddings depend on the mask only: fp32
torch on the device, cached per mask.

Odd blocks shift by 3 at every resolution, as ``transformers``' ``SwinBackbone`` runs them (``always_partition=True``: the window and the shift are not
clamped to a small stage).  A stage whose smaller side is below 7 is a ValueError.

Parameter names are those of ``transformers.GroundingDinoModel`` under ``backbone.`` and ``input_proj_vision.``.  The text encoder, the fusion encoder and
the decoder stay the caller's ``transformers`` modules: ``attach`` makes such a model use this front.
"""
import math

import torch
import torch.nn as nn

from . import ops
from .weights_pack import pack_conv3x3

BACKBONE = "backbone.conv_encoder.model."
WINDOW = 7


def _swin_cfg(config):
    bc = config.backbone_config
    get = (lambda k, d=None: bc.get(k, d)) if isinstance(bc, dict) else (lambda k, d=None: getattr(bc, k, d))
    return dict(embed_dim=int(get("embed_dim")), depths=list(get("depths")), num_heads=list(get("num_heads")), window=int(get("window_size", 7)),
                patch=int(get("patch_size", 4)), eps=float(get("layer_norm_eps", 1e-5)), mlp_ratio=float(get("mlp_ratio", 4.0)),
                out_indices=list(get("out_indices")), channels=int(get("num_channels", 3)))


def expected_names(config):
    """The parameter names ``from_state_dict`` takes: ``GroundingDinoModel``'s state dict under ``backbone.`` and ``input_proj_vision.``."""
    sc = _swin_cfg(config)
    names = []
    sw = BACKBONE + "swin."
    names += [sw + "embeddings.patch_embeddings.projection." + s for s in ("weight", "bias")]
    names += [sw + "embeddings.norm." + s for s in ("weight", "bias")]
    for i, depth in enumerate(sc["depths"]):
        for j in range(depth):
            blk = f"{sw}encoder.layers.{i}.blocks.{j}."
            for lin in ("attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.o_proj", "layernorm_before", "layernorm_after",
                        "mlp.fc1", "mlp.fc2"):
                names += [blk + lin + ".weight", blk + lin + ".bias"]
            names.append(blk + "attention.relative_position_bias.relative_position_bias_table")
        if i + 1 < len(sc["depths"]):
            ds = f"{sw}encoder.layers.{i}.downsample."
            names += [ds + "reduction.weight", ds + "norm.weight", ds + "norm.bias"]
    names += [sw + "layernorm.weight", sw + "layernorm.bias"]                  # SwinModel's final norm: in the state dict, unused by the backbone
    for idx in sc["out_indices"]:
        names += [f"{BACKBONE}hidden_states_norms.stage{idx}.{s}" for s in ("weight", "bias")]
    for level in range(int(config.num_feature_levels)):
        names += [f"input_proj_vision.{level}.{m}.{s}" for m in (0, 1) for s in ("weight", "bias")]
    return set(names)


class GroundingDinoVisionFront:
    """``forward(pixel_values, pixel_mask)`` returns what ``GroundingDinoConvModel.forward`` returns; ``project(features)`` the ``d_model`` levels."""

    def __init__(self, config, params, device="cuda", dtype=torch.bfloat16):
        sc = _swin_cfg(config)
        bad = []
        if sc["window"] != WINDOW:
            bad.append(f"window_size {sc['window']}")
        if sc["patch"] != 4 or sc["channels"] != 3:
            bad.append(f"patch_size {sc['patch']} / num_channels {sc['channels']}")
        for i, h in enumerate(sc["num_heads"]):
            if sc["embed_dim"] * 2 ** i != 32 * h:
                bad.append(f"stage {i}: head dim {sc['embed_dim'] * 2 ** i}/{h}")
        if getattr(config, "position_embedding_type", "sine") != "sine":
            bad.append(f"position_embedding_type {config.position_embedding_type}")
        if bad:
            raise NotImplementedError(f"GroundingDinoVisionFront: {', '.join(bad)} has no kernel; supported: Swin with window 7, head dim 32, patch 4, "
                                      "sine position embeddings")
        want = expected_names(config)
        missing, unexpected = sorted(want - set(params)), sorted(set(params) - want)
        if missing or unexpected:
            raise RuntimeError(f"state dict mismatch: missing {missing[:5]}... unexpected {unexpected[:5]}...")
        self.config, self.sc = config, sc
        self.device, self.dtype = torch.device(device), dtype
        self.d_model = int(config.d_model)
        self.levels = int(config.num_feature_levels)
        self.temperature = float(getattr(config, "positional_embedding_temperature", 20))
        p = {k: v.detach().to(device=self.device, dtype=dtype).contiguous() for k, v in params.items()}
        sw = BACKBONE + "swin."
        C0 = sc["embed_dim"]
        self.patch_w = p[sw + "embeddings.patch_embeddings.projection.weight"].reshape(C0, 48).contiguous()       # flattening c * 16 + kh * 4 + kw
        self.patch_b = p[sw + "embeddings.patch_embeddings.projection.bias"]
        self.embed_norm = (p[sw + "embeddings.norm.weight"], p[sw + "embeddings.norm.bias"])
        self.stages = []
        for i, depth in enumerate(sc["depths"]):
            blocks = []
            for j in range(depth):
                blk = f"{sw}encoder.layers.{i}.blocks.{j}."
                a = blk + "attention."
                blocks.append(dict(
                    ln1=(p[blk + "layernorm_before.weight"], p[blk + "layernorm_before.bias"]),
                    wqkv=torch.cat([p[a + "q_proj.weight"], p[a + "k_proj.weight"], p[a + "v_proj.weight"]], 0).contiguous(),
                    bqkv=torch.cat([p[a + "q_proj.bias"], p[a + "k_proj.bias"], p[a + "v_proj.bias"]], 0).contiguous(),
                    pads=(p[a + "q_proj.bias"], p[a + "k_proj.bias"], p[a + "v_proj.bias"]),
                    table=p[a + "relative_position_bias.relative_position_bias_table"],
                    wo=p[a + "o_proj.weight"], bo=p[a + "o_proj.bias"],
                    ln2=(p[blk + "layernorm_after.weight"], p[blk + "layernorm_after.bias"]),
                    w1=p[blk + "mlp.fc1.weight"], b1=p[blk + "mlp.fc1.bias"], w2=p[blk + "mlp.fc2.weight"], b2=p[blk + "mlp.fc2.bias"],
                    shift=0 if j % 2 == 0 else WINDOW // 2))
            ds = None
            if i + 1 < len(sc["depths"]):
                d = f"{sw}encoder.layers.{i}.downsample."
                ds = dict(norm=(p[d + "norm.weight"], p[d + "norm.bias"]), w=p[d + "reduction.weight"])
            self.stages.append(dict(blocks=blocks, heads=sc["num_heads"][i], down=ds))
        self.out_norms = {idx: (p[f"{BACKBONE}hidden_states_norms.stage{idx}.weight"], p[f"{BACKBONE}hidden_states_norms.stage{idx}.bias"])
                          for idx in sc["out_indices"]}
        self.proj = []
        for level in range(self.levels):
            w = p[f"input_proj_vision.{level}.0.weight"]
            k3 = w.shape[-1] == 3
            self.proj.append(dict(k3=k3, cin=int(w.shape[1]), w=pack_conv3x3(w) if k3 else w.reshape(w.shape[0], w.shape[1]).contiguous(),
                                  b=p[f"input_proj_vision.{level}.0.bias"], gamma=p[f"input_proj_vision.{level}.1.weight"],
                                  beta=p[f"input_proj_vision.{level}.1.bias"]))
        self._tokens = []              # (an NCHW feature map handed out by the last forward, its token-major form): matched by identity, and kept alive
        self._pos_cache = {}
        self.op_calls = 0              # calls into the native library so far (a tally kept here, not a count of kernel launches)

    @classmethod
    def from_state_dict(cls, config, state_dict, device="cuda", dtype=torch.bfloat16):
        """``state_dict``: the ``backbone.`` and ``input_proj_vision.`` entries of a ``GroundingDinoModel`` state dict (a whole state dict of that model
        or of ``GroundingDinoForObjectDetection`` is filtered to them).  A missing or unexpected name is a RuntimeError."""
        pre = "model." if any(k.startswith("model.backbone.") for k in state_dict) else ""
        sub = {k[len(pre):]: v for k, v in state_dict.items()
               if k.startswith(pre + "backbone.") or k.startswith(pre + "input_proj_vision.")}
        return cls(config, sub, device, dtype)

    # ---- the backbone ------------------------------------------------------------------------------------------------------------------------
    def _block(self, x, blk, B, H, W, heads, taps=None):
        C = x.shape[1]
        n = H * W
        y = ops.layernorm(x, blk["ln1"][0], blk["ln1"][1], self.sc["eps"])
        qkv = ops.linear(y, blk["wqkv"], blk["bqkv"])
        o = torch.empty((B * n, C), dtype=x.dtype, device=x.device)
        ops.attention_swin(qkv, 3 * C, n * 3 * C, qkv[:, C:], 3 * C, n * 3 * C, qkv[:, 2 * C:], 3 * C, n * 3 * C, blk["pads"][0], blk["pads"][1],
                           blk["pads"][2], blk["table"], B, heads, H, W, blk["shift"], 32 ** -0.5, o, C, n * C)
        x = ops.linear(o, blk["wo"], blk["bo"], res=x)
        y = ops.layernorm(x, blk["ln2"][0], blk["ln2"][1], self.sc["eps"])
        y = ops.linear(y, blk["w1"], blk["b1"], act=ops.ACT_GELU)
        self.op_calls += 7
        return ops.linear(y, blk["w2"], blk["b2"], res=x)

    def _merge(self, x, ds, B, H, W):
        """transformers' SwinPatchMerging: the 2 x 2 neighbours in the order (row, col) = (0,0), (1,0), (0,1), (1,1), odd sides zero-padded"""
        C = x.shape[1]
        g = x.reshape(B, H, W, C)
        if H % 2 or W % 2:
            g = nn.functional.pad(g, (0, 0, 0, W % 2, 0, H % 2))
        g = torch.cat([g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
        y = ops.layernorm(g, ds["norm"][0], ds["norm"][1], 1e-5)
        self.op_calls += 2
        return ops.linear(y, ds["w"]), (H + 1) // 2, (W + 1) // 2

    def backbone(self, pixel_values, hidden_taps=None):
        """pixel_values [B, 3, h, w] -> [(feature NCHW, token-major [B * H * W, C], H, W)] for the configured out_indices.
        ``hidden_taps``: a list that receives (stage, block, [B, H, W, C] state) after every block of stage 0 (the tests' stage-1 checks)."""
        if not pixel_values.is_cuda:
            raise RuntimeError("theatergen_amd GroundingDINO front runs on the GPU only (no CPU fallback)")
        x = pixel_values.to(self.dtype)
        B, ch, h, w = x.shape
        if ch != 3:
            raise ValueError(f"GroundingDinoVisionFront: pixel_values {tuple(x.shape)}, expected [B, 3, h, w]")
        if h % 4 or w % 4:
            x = nn.functional.pad(x, (0, (-w) % 4, 0, (-h) % 4))
        H, W = x.shape[2] // 4, x.shape[3] // 4
        tok = ops.pixel_unshuffle(x, 4)
        x = ops.gemm(tok, self.patch_w, B * H * W, self.patch_w.shape[0], 48, bias=self.patch_b)
        x = ops.layernorm(x, self.embed_norm[0], self.embed_norm[1], 1e-5)          # SwinEmbeddings.norm is nn.LayerNorm(embed_dim): the default eps
        self.op_calls += 3
        feats = []
        for i, st in enumerate(self.stages):
            if min(H, W) < WINDOW:
                raise ValueError(f"GroundingDinoVisionFront: stage {i + 1} is {H} x {W} tokens, smaller than the window of 7 (image too small)")
            for j, blk in enumerate(st["blocks"]):
                x = self._block(x, blk, B, H, W, st["heads"])
                if hidden_taps is not None and i == 0:
                    hidden_taps.append((i, j, x.reshape(B, H, W, -1)))
            if i + 1 in self.out_norms:
                g, b_ = self.out_norms[i + 1]
                f = ops.layernorm(x, g, b_, 1e-5)
                C = f.shape[1]
                nchw = ops.transpose(f, B, H * W, C).reshape(B, C, H, W)
                self.op_calls += 2
                feats.append((nchw, f, H, W))
            if st["down"] is not None:
                x, H, W = self._merge(x, st["down"], B, H, W)
        return feats

    # ---- masks and position embeddings -------------------------------------------------------------------------------------------------------
    @staticmethod
    def level_mask(pixel_mask, size):
        """the nearest interpolation transformers uses"""
        return nn.functional.interpolate(pixel_mask[None].float(), size=size).to(torch.bool)[0]

    def position_embedding(self, feature_map, mask):
        """``GroundingDinoSinePositionEmbedding``: fp32 torch on the device, then the feature map's dtype"""
        half = self.d_model // 2
        y = mask.cumsum(1, dtype=torch.float32)
        x = mask.cumsum(2, dtype=torch.float32)
        y = y / (y[:, -1:, :] + 1e-6) * (2 * math.pi)
        x = x / (x[:, :, -1:] + 1e-6) * (2 * math.pi)
        dim_t = torch.arange(half, dtype=torch.float32, device=mask.device)
        dim_t = self.temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / half)
        px, py = x[:, :, :, None] / dim_t, y[:, :, :, None] / dim_t
        px = torch.stack((px[:, :, :, 0::2].sin(), px[:, :, :, 1::2].cos()), dim=4).flatten(3)
        py = torch.stack((py[:, :, :, 0::2].sin(), py[:, :, :, 1::2].cos()), dim=4).flatten(3)
        return torch.cat((py, px), dim=3).permute(0, 3, 1, 2).to(feature_map.dtype)

    def _masks_and_pos(self, pixel_mask, sizes, like):
        """Level masks and position embeddings of ``pixel_mask``, cached per mask TENSOR: the entry holds the tensor, and hits only for the same object at the
        same ``_version`` (no in-place write since).  Comparing contents would need a device-to-host copy and a stream synchronisation on every forward; a
        caller who passes a new mask tensor each time pays the fp32 torch computation instead, which stays on the stream."""
        key = (id(pixel_mask), pixel_mask._version, tuple(sizes), like.dtype)
        hit = self._pos_cache.get(key)
        if hit is None or hit[0] is not pixel_mask:
            if len(self._pos_cache) >= 8:
                self._pos_cache.clear()
            masks = [self.level_mask(pixel_mask, s) for s in sizes]
            hit = (pixel_mask, masks, [self.position_embedding(like, m) for m in masks])
            self._pos_cache[key] = hit
        return hit[1], hit[2]

    def forward(self, pixel_values, pixel_mask):
        """-> ([(feature [B, C, H, W], mask bool [B, H, W])], [position embedding [B, d_model, H, W]]), as ``GroundingDinoConvModel.forward``"""
        with torch.no_grad():
            feats = self.backbone(pixel_values)
            self._tokens = [(f[0], f[1], f[0]._version) for f in feats]
            masks, pos = self._masks_and_pos(pixel_mask.to(pixel_values.device), [(f[2], f[3]) for f in feats], feats[0][0])
            return [(f[0], m) for f, m in zip(feats, masks)], list(pos)

    __call__ = forward

    # ---- the projection levels -----------------------------------------------------------------------------------------------------------------
    def _token_form(self, source):
        """the token-major form of ``source`` if it IS a feature map the last forward handed out and nobody has written to it since, else None"""
        for nchw, tok, version in self._tokens:
            if nchw is source and source._version == version:
                return tok
        return None

    def project_level(self, level, source):
        """``input_proj_vision[level]`` on an NCHW ``source``: 1 x 1 convolution (GEMM) or the stride-2 3 x 3 one, then GroupNorm(32) -> NCHW.
        Any NCHW tensor is taken; a feature map of the last ``forward`` (the same object, unmodified) skips the transpose back to token-major."""
        with torch.no_grad():
            pr = self.proj[level]
            B, C, H, W = source.shape
            if C != pr["cin"]:
                raise ValueError(f"project_level: level {level} takes {pr['cin']} channels, source has {C}")
            tok = self._token_form(source)
            if tok is None:
                tok = ops.transpose(source.to(self.dtype).contiguous().reshape(B, C, H * W), B, C, H * W).reshape(B * H * W, C)
            if pr["k3"]:
                y = ops.conv3x3(tok, pr["w"], B, H, W, C, stride=2, bias=pr["b"])
                H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            else:
                y = ops.linear(tok, pr["w"], pr["b"])
            y = ops.groupnorm(y, B, H * W, 32, 1e-5, pr["gamma"], pr["beta"])
            self.op_calls += 3
            return ops.transpose(y, B, H * W, self.d_model).reshape(B, self.d_model, H, W)

    def project(self, features):
        """features: the (feature, mask) list of ``forward`` -> the ``num_feature_levels`` projected maps; levels past the backbone's come from the LAST
        raw feature map through the stride-2 3 x 3 convolution (GroundingDINO has one such level)."""
        out = [self.project_level(i, f[0]) for i, f in enumerate(features)]
        if self.levels > len(features) + 1:
            raise NotImplementedError("GroundingDinoVisionFront: more than one extra feature level")
        for level in range(len(features), self.levels):
            out.append(self.project_level(level, features[-1][0]))
        return out

    # ---- transformers integration --------------------------------------------------------------------------------------------------------------
    def attach(self, hf_model):
        """Make a ``transformers`` ``GroundingDinoModel`` / ``GroundingDinoForObjectDetection`` use this front: its ``backbone`` and ``input_proj_vision``
        are replaced by thin modules that call it.  Everything after them still runs as ``transformers`` code."""
        core = hf_model.model if hasattr(hf_model, "model") and hasattr(hf_model.model, "input_proj_vision") else hf_model
        if not hasattr(core, "input_proj_vision") or not hasattr(core, "backbone"):
            raise TypeError("attach: a transformers GroundingDinoModel or GroundingDinoForObjectDetection expected")
        p0 = next(iter(core.parameters()), None)
        out_dtype = p0.dtype if p0 is not None else self.dtype               # what the transformers modules behind the front compute in
        core.backbone = _FrontBackbone(self, out_dtype)
        core.input_proj_vision = nn.ModuleList([_FrontProjection(self, level, out_dtype) for level in range(self.levels)])
        return hf_model


class _FrontBackbone(nn.Module):
    def __init__(self, front, out_dtype):
        super().__init__()
        self._front, self.out_dtype = [front], out_dtype         # a list: the front is no nn.Module and is not to be registered

    def position_embedding(self, feature_map, mask):
        return self._front[0].position_embedding(feature_map, mask)

    def forward(self, pixel_values, pixel_mask):
        front = self._front[0]
        feats, pos = front.forward(pixel_values, pixel_mask)
        if self.out_dtype == front.dtype:
            return feats, pos
        out = []
        for f, m in feats:                                        # the caller's dtype; the cast map reaches the same token-major form
            g = f.to(self.out_dtype)
            front._tokens.append((g, front._token_form(f), g._version))
            out.append((g, m))
        return out, [p.to(self.out_dtype) for p in pos]


class _FrontProjection(nn.Module):
    def __init__(self, front, level, out_dtype):
        super().__init__()
        self._front, self.level, self.out_dtype = [front], level, out_dtype

    def forward(self, source):
        return self._front[0].project_level(self.level, source).to(self.out_dtype)
