"""Segment-Anything's prompt encoder and mask decoder on the native kernels, and ``SamModel`` = encoder + both (transformers' parameter names, so a
``transformers.SamModel`` state dict loads as it is).

Storage in bf16 / fp16 with fp32 accumulation, as everywhere in this tree — NOT ``torch.autocast``: the decoder Fourier-encodes pixel coordinates as
sin(2 pi x G) with |G| ~ 32, and coordinates rounded to half precision move that phase by up to a radian.  The positional matrix stays fp32 and
``ops.sam_posenc`` computes every encoding (box corners, points, the dense grid) in fp32 from fp32 coordinates.

One decode, token-major, P = B * nb prompts (each with its own copy of the image tokens, which the two-way transformer updates per prompt):
  tokens [P * nt, 256] = iou token | 4 mask tokens | sparse prompt embeddings (nt = 7 for a box); image tokens [P * g^2, 256] = embeddings + no_mask_embed.
  Per layer: self-attention of the tokens (head dim 32), tokens -> image cross-attention (head dim 16, nt queries against g^2 keys), ReLU MLP, image -> tokens
  cross-attention (g^2 queries against nt keys); every projection is ``ops.linear`` / ``ops.gemm`` (V leaves its GEMM transposed, the layout ``ops.attention``
  reads), every softmax ``ops.attention``, every LayerNorm ``ops.layernorm``.  Then the final tokens -> image attention, the four hypernetwork MLPs, the IoU head,
  and ``ops.sam_mask_head``: both ConvTransposes, the channel LayerNorm, both GELUs and the product with the hypernetwork outputs in one launch.
torch does indexing, concatenation and allocation only; nothing synchronises with the host, and every shape depends on (B, nb, prompt kind) alone.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .sam import SamVisionEncoder, sam_vit_h_config
from .unet import _Packed
from .weights_pack import pack_sam_upscale

SUPPORTED = ("hidden 256, 8 heads, attention downsample 2, mlp 2048, 2 layers, 3 multimask outputs, iou head depth 3 (hidden 256), 128 positional features, "
             "4 point embeddings, image_embedding_size a multiple of 8 up to 64")


class SamDecoderConfig(SimpleNamespace):
    pass


def sam_decoder_config(image_embedding_size=64, image_size=None):
    """facebook/sam-vit-* prompt encoder + mask decoder (the three checkpoints share it).  ``image_size``: the side of the padded input image the prompt
    coordinates are given in (16 pixels per embedding cell)."""
    g = int(image_embedding_size)
    return SamDecoderConfig(hidden_size=256, num_attention_heads=8, attention_downsample_rate=2, mlp_dim=2048, num_hidden_layers=2,
                            num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256, image_embedding_size=g,
                            image_size=int(image_size) if image_size is not None else 16 * g, num_pos_feats=128, mask_input_channels=16,
                            num_point_embeddings=4, layer_norm_eps=1e-6)


def _refuse(cfg):
    want = sam_decoder_config()
    bad = [f"{k} {getattr(cfg, k, None)}" for k in ("hidden_size", "num_attention_heads", "attention_downsample_rate", "mlp_dim", "num_hidden_layers",
                                                     "num_multimask_outputs", "iou_head_depth", "iou_head_hidden_dim", "num_pos_feats", "num_point_embeddings")
           if getattr(cfg, k, None) != getattr(want, k)]
    g = getattr(cfg, "image_embedding_size", None)
    if not isinstance(g, int) or g <= 0 or g % 8 or g > 64:
        bad.append(f"image_embedding_size {g}")
    if bad:
        raise NotImplementedError(f"SAM prompt encoder / mask decoder: {', '.join(bad)} has no kernel; supported: {SUPPORTED}")


def _embedding(rows, dim):
    m = nn.Module()
    m.weight = nn.Parameter(torch.zeros(rows, dim))
    return m


class _PositionalEmbedding(nn.Module):
    def __init__(self, feats):
        super().__init__()
        self.positional_embedding = nn.Parameter(torch.zeros(2, feats))


class SamPromptEncoder(nn.Module):
    """``transformers.SamPromptEncoder``'s parameters (``mask_embed`` included, so a state dict loads; mask prompts themselves are refused by ``SamModel``)
    and its sparse embeddings through ``ops.sam_posenc``."""

    def __init__(self, config=None):
        super().__init__()
        cfg = config if config is not None else sam_decoder_config()
        _refuse(cfg)
        self.config = cfg
        D, mc = cfg.hidden_size, cfg.mask_input_channels
        self.shared_embedding = _PositionalEmbedding(cfg.num_pos_feats)
        me = nn.Module()
        me.conv1, me.conv2, me.conv3 = nn.Conv2d(1, mc // 4, 2, stride=2), nn.Conv2d(mc // 4, mc, 2, stride=2), nn.Conv2d(mc, D, 1)
        me.layer_norm1, me.layer_norm2 = nn.LayerNorm(mc // 4), nn.LayerNorm(mc)
        self.mask_embed = me
        self.no_mask_embed = _embedding(1, D)
        self.point_embed = nn.ModuleList([_embedding(1, D) for _ in range(cfg.num_point_embeddings)])
        self.not_a_point_embed = _embedding(1, D)
        self._p = _Packed()
        for p_ in self.parameters():
            p_.requires_grad_(False)

    def table(self):
        """fp32 [5, 256]: point_embed[0..3] | not_a_point_embed, from the stored (rounded) values"""
        ws = [e.weight for e in self.point_embed] + [self.not_a_point_embed.weight]
        return self._p.get("table", ws, lambda: torch.cat([w.detach().float() for w in ws], 0).contiguous())

    def sparse(self, gauss, input_points, input_labels, input_boxes, dtype, device):
        """host prompts (pixels of the padded input image) -> ([P * ns, 256] in ``dtype``, ns).  points [B, nb, np, 2] + labels [B, nb, np] come first, then the
        two corners of boxes [B, nb, 4]; without a box the points get the padding point (label -1).  Labels: 1 / 0 / -1 (and 2 / 3 for the corners)."""
        S = np.float32(self.config.image_size)
        coords, labels = [], []
        if input_points is not None:
            if input_labels is None:
                raise ValueError("If points are provided, labels must also be provided.")
            pts, lab = _host(input_points, np.float32), _host(input_labels, np.int32)
            if pts.ndim != 4 or pts.shape[-1] != 2 or lab.shape != pts.shape[:3]:
                raise ValueError(f"input_points [B, nb, n, 2] with input_labels [B, nb, n] expected, got {pts.shape} and {lab.shape}")
            if input_boxes is None:
                pts = np.concatenate([pts, np.full(pts.shape[:2] + (1, 2), -0.5, np.float32)], 2)        # + 0.5 below: the reference's zero padding point
                lab = np.concatenate([lab, np.full(lab.shape[:2] + (1,), -1, np.int32)], 2)
            coords.append(pts)
            labels.append(lab)
        if input_boxes is not None:
            bx = _host(input_boxes, np.float32)
            if bx.ndim != 3 or bx.shape[-1] != 4:
                raise ValueError(f"input_boxes [B, nb, 4] expected, got {bx.shape}")
            coords.append(bx.reshape(bx.shape[0], bx.shape[1], 2, 2))
            labels.append(np.broadcast_to(np.array([2, 3], np.int32), bx.shape[:2] + (2,)))
        if not coords:
            raise ValueError("SamModel: a box or a point prompt is needed")
        if len({c.shape[:2] for c in coords}) != 1:
            raise ValueError("input_points and input_boxes must agree in [B, nb]")
        c = np.concatenate(coords, 2)
        lb = np.ascontiguousarray(np.concatenate(labels, 2).reshape(-1))
        B, nb, ns = c.shape[:3]
        c = np.ascontiguousarray(((c + np.float32(0.5)) / S).astype(np.float32).reshape(-1, 2))           # the reference's fp32 sequence: shift, divide
        emb = ops.sam_posenc(torch.from_numpy(c).to(device), gauss, torch.from_numpy(lb).to(device), self.table().reshape(5, -1), dtype=dtype)
        return emb, B, nb, ns


def _host(x, dt):
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise ValueError("SamModel: prompts are host data (lists, numpy arrays or CPU tensors), as the processor returns them")
        x = x.detach().to(torch.float64).numpy()
    return np.asarray(x, dtype=np.float64).astype(dt)


class _Attention(nn.Module):
    def __init__(self, D, heads, downsample):
        super().__init__()
        self.internal, self.heads = D // downsample, heads
        self.q_proj, self.k_proj, self.v_proj = nn.Linear(D, self.internal), nn.Linear(D, self.internal), nn.Linear(D, self.internal)
        self.out_proj = nn.Linear(self.internal, D)
        self._p = _Packed()

    def run(self, q_in, k_in, v_in, P, nq, nk, res=None):
        """q_in [P * nq, D], k_in / v_in [P * nk, D] -> out_proj(softmax(q k^T / sqrt(d)) v) (+ res) [P * nq, D]"""
        C_, d = self.internal, self.internal // self.heads
        dt, dev = q_in.dtype, q_in.device
        kp, vp = self.k_proj, self.v_proj
        wkv = self._p.get("kv", [kp.weight, vp.weight, kp.bias, vp.bias],
                          lambda: (torch.cat([kp.weight.detach(), vp.weight.detach()], 0).contiguous(), torch.cat([kp.bias.detach(), vp.bias.detach()]).contiguous()))
        q = ops.linear(q_in, self.q_proj.weight, self.q_proj.bias)
        ldt = (nk + 7) // 8 * 8
        vt = torch.empty((P, C_, ldt), dtype=dt, device=dev) if ldt == nk else torch.zeros((P, C_, ldt), dtype=dt, device=dev)
        k = torch.empty((P * nk, C_), dtype=dt, device=dev)
        # V leaves its GEMM transposed only next to untransposed columns: [k_proj ; v_proj] on the value input.  Where key and value inputs differ (the
        # positional encoding is added to the keys only) those columns are overwritten by k_proj of the key input
        ops.gemm(v_in, wkv[0], P * nk, 2 * C_, v_in.shape[1], bias=wkv[1], rows_per_batch=nk, out=k, n_split=C_, out_t=vt, ldt=ldt)
        if k_in is not v_in:
            ops.linear(k_in, kp.weight, kp.bias, out=k)
        o = torch.empty((P * nq, C_), dtype=dt, device=dev)
        ops.attention(q, C_, nq * C_, k, C_, nk * C_, vt, ldt, C_ * ldt, nk, P, self.heads, d, nq, float(d) ** -0.5, o, C_, nq * C_)
        return ops.linear(o, self.out_proj.weight, self.out_proj.bias, res=res)


class _TwoWayBlock(nn.Module):
    def __init__(self, cfg, skip_first_layer_pe):
        super().__init__()
        D, H, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
        self.skip_first_layer_pe, self.eps = skip_first_layer_pe, eps
        self.self_attn = _Attention(D, H, 1)
        self.layer_norm1 = nn.LayerNorm(D, eps=eps)
        self.cross_attn_token_to_image = _Attention(D, H, cfg.attention_downsample_rate)
        self.layer_norm2 = nn.LayerNorm(D, eps=eps)
        mlp = nn.Module()
        mlp.lin1, mlp.lin2 = nn.Linear(D, cfg.mlp_dim), nn.Linear(cfg.mlp_dim, D)
        self.mlp = mlp
        self.layer_norm3 = nn.LayerNorm(D, eps=eps)
        self.layer_norm4 = nn.LayerNorm(D, eps=eps)
        self.cross_attn_image_to_token = _Attention(D, H, cfg.attention_downsample_rate)

    def _ln(self, ln, x):
        return ops.layernorm(x, ln.weight, ln.bias, self.eps)

    def run(self, queries, keys, qpe, kpe, P, nt, n):
        if self.skip_first_layer_pe:
            queries = self.self_attn.run(queries, queries, queries, P, nt, nt)
        else:
            q = ops.add(queries, qpe)
            queries = self.self_attn.run(q, q, queries, P, nt, nt, res=queries)
        queries = self._ln(self.layer_norm1, queries)
        q, k = ops.add(queries, qpe), ops.add(keys, kpe)
        queries = self.cross_attn_token_to_image.run(q, k, keys, P, nt, n, res=queries)
        queries = self._ln(self.layer_norm2, queries)
        h = ops.relu(ops.linear(queries, self.mlp.lin1.weight, self.mlp.lin1.bias))
        queries = ops.linear(h, self.mlp.lin2.weight, self.mlp.lin2.bias, res=queries)
        queries = self._ln(self.layer_norm3, queries)
        q = ops.add(queries, qpe)
        keys = self.cross_attn_image_to_token.run(k, q, queries, P, n, nt, res=keys)
        return queries, self._ln(self.layer_norm4, keys)


class _FeedForward(nn.Module):
    def __init__(self, din, hidden, dout, depth):
        super().__init__()
        self.proj_in, self.proj_out = nn.Linear(din, hidden), nn.Linear(hidden, dout)
        self.layers = nn.ModuleList([nn.Linear(hidden, hidden) for _ in range(depth - 2)])
        self._p = _Packed()

    def run(self, x, out=None):
        """ReLU MLP; x may be a row-strided view.  An output narrower than 8 columns runs on a zero-padded copy of ``proj_out`` (its first columns are returned)."""
        if x.stride(1) != 1 or x.stride(0) != x.shape[1]:
            x = torch.empty(x.shape, dtype=x.dtype, device=x.device).copy_(x)            # a token's rows, gathered (data movement)
        h = ops.relu(ops.linear(x, self.proj_in.weight, self.proj_in.bias))
        for layer in self.layers:
            h = ops.relu(ops.linear(h, layer.weight, layer.bias))
        po = self.proj_out
        n = po.weight.shape[0]
        if n % 8 == 0:
            return ops.linear(h, po.weight, po.bias, out=out)
        pad = 8 - n % 8
        w, b = self._p.get("out", [po.weight, po.bias], lambda: (torch.nn.functional.pad(po.weight.detach(), (0, 0, 0, pad)).contiguous(),
                                                                 torch.nn.functional.pad(po.bias.detach(), (0, pad)).contiguous()))
        return ops.linear(h, w, b)[:, :n]


class SamMaskDecoder(nn.Module):
    """``transformers.SamMaskDecoder`` (same parameter names) on the native kernels; GPU only."""

    def __init__(self, config=None):
        super().__init__()
        cfg = config if config is not None else sam_decoder_config()
        _refuse(cfg)
        self.config = cfg
        D = cfg.hidden_size
        self.num_mask_tokens = cfg.num_multimask_outputs + 1
        self.iou_token = _embedding(1, D)
        self.mask_tokens = _embedding(self.num_mask_tokens, D)
        tr = nn.Module()
        tr.layers = nn.ModuleList([_TwoWayBlock(cfg, i == 0) for i in range(cfg.num_hidden_layers)])
        tr.final_attn_token_to_image = _Attention(D, cfg.num_attention_heads, cfg.attention_downsample_rate)
        tr.layer_norm_final_attn = nn.LayerNorm(D)                                      # eps 1e-5: transformers leaves this one at the default
        self.transformer = tr
        self.upscale_conv1 = nn.ConvTranspose2d(D, D // 4, 2, stride=2)
        self.upscale_conv2 = nn.ConvTranspose2d(D // 4, D // 8, 2, stride=2)
        self.upscale_layer_norm = nn.LayerNorm(D // 4, eps=1e-6)
        self.output_hypernetworks_mlps = nn.ModuleList([_FeedForward(D, D, D // 8, 3) for _ in range(self.num_mask_tokens)])
        self.iou_prediction_head = _FeedForward(D, cfg.iou_head_hidden_dim, self.num_mask_tokens, cfg.iou_head_depth)
        self._p = _Packed()
        for p_ in self.parameters():
            p_.requires_grad_(False)

    def run(self, keys, kpe, sparse, P, ns, g):
        """keys [P * g^2, 256] (image embeddings + dense prompt embedding), kpe the same shape (dense positional encoding), sparse [P * ns, 256] ->
        (fp32 logits [P, 4, 4g, 4g], iou [P, 4] in the storage dtype)"""
        D, n, nt = self.config.hidden_size, g * g, self.num_mask_tokens + 1 + ns
        dt, dev = keys.dtype, keys.device
        out_tok = torch.cat([self.iou_token.weight, self.mask_tokens.weight], 0)
        tokens = torch.cat([out_tok[None].expand(P, -1, -1), sparse.reshape(P, ns, D)], 1).reshape(P * nt, D).contiguous()
        tr = self.transformer
        queries = tokens
        for layer in tr.layers:
            queries, keys = layer.run(queries, keys, tokens, kpe, P, nt, n)
        q, k = ops.add(queries, tokens), ops.add(keys, kpe)
        queries = tr.final_attn_token_to_image.run(q, k, keys, P, nt, n, res=queries)
        queries = ops.layernorm(queries, tr.layer_norm_final_attn.weight, tr.layer_norm_final_attn.bias, tr.layer_norm_final_attn.eps)
        qv = queries.view(P, nt, D)
        hyper = torch.empty((P, self.num_mask_tokens, D // 8), dtype=dt, device=dev)
        for i, mlp in enumerate(self.output_hypernetworks_mlps):
            mlp.run(qv[:, 1 + i], out=hyper[:, i])
        c1, c2, ln = self.upscale_conv1, self.upscale_conv2, self.upscale_layer_norm
        w1, w2, vec = self._p.get("up", [c1.weight, c1.bias, ln.weight, ln.bias, c2.weight, c2.bias],
                                  lambda: pack_sam_upscale(c1.weight, c1.bias, ln.weight, ln.bias, c2.weight, c2.bias))
        logits = ops.sam_mask_head(keys, P, g, w1, w2, vec, hyper, eps=ln.eps)
        iou = self.iou_prediction_head.run(qv[:, 0])
        return logits, iou


class SamModel(nn.Module):
    """``transformers.SamModel``'s forward for box / point prompts on the native kernels: ``vision_encoder`` (``SamVisionEncoder``), ``prompt_encoder``,
    ``mask_decoder``, ``shared_image_embedding``.  -> SimpleNamespace(pred_masks fp32 [B, nb, 3 or 1, 4g, 4g], iou_scores [B, nb, 3 or 1] in the model dtype)."""

    def __init__(self, vision_config=None, decoder_config=None, with_vision=True):
        super().__init__()
        dcfg = decoder_config if decoder_config is not None else sam_decoder_config()
        _refuse(dcfg)
        self.decoder_config = dcfg
        self.vision_encoder = SamVisionEncoder(vision_config if vision_config is not None else sam_vit_h_config()) if with_vision else None
        self.prompt_encoder = SamPromptEncoder(dcfg)
        self.mask_decoder = SamMaskDecoder(dcfg)
        self.shared_image_embedding = _PositionalEmbedding(dcfg.num_pos_feats)
        self._cache = {}
        for p_ in self.parameters():
            p_.requires_grad_(False)

    @property
    def dtype(self):
        return self.mask_decoder.iou_token.weight.dtype

    @property
    def device(self):
        return self.mask_decoder.iou_token.weight.device

    def _gauss(self):
        g = self.shared_image_embedding.positional_embedding
        if g.dtype != torch.float32:
            raise RuntimeError("SamModel: shared_image_embedding.positional_embedding must stay fp32 (use from_state_dict, or .float() it after .to(dtype))")
        return g

    def _dense(self, P, dtype, device):
        """(dense positional encoding, dense prompt embedding), each [P * g^2, 256] in ``dtype``: constants, made once per (device, dtype, P)"""
        g = self.decoder_config.image_embedding_size
        key = (device, dtype, P, self._gauss().data_ptr(), self.prompt_encoder.no_mask_embed.weight.data_ptr())
        if key not in self._cache:
            c = ((torch.arange(g, dtype=torch.float32) + 0.5) / g)
            grid = torch.stack([c[None, :].expand(g, g), c[:, None].expand(g, g)], -1).reshape(g * g, 2).contiguous()          # token (i, j): (x, y) = (j, i)
            pe = ops.sam_posenc(grid.to(device), self._gauss(), dtype=dtype)
            nm = self.prompt_encoder.no_mask_embed.weight.detach()
            self._cache[key] = (pe.repeat(P, 1).contiguous(), nm.expand(P * g * g, -1).contiguous())
        return self._cache[key]

    def get_image_embeddings(self, pixel_values):
        if self.vision_encoder is None:
            raise RuntimeError("SamModel: built without a vision encoder; pass image_embeddings")
        return self.vision_encoder(pixel_values)

    def forward(self, pixel_values=None, image_embeddings=None, input_boxes=None, input_points=None, input_labels=None, multimask_output=True,
                input_masks=None, attention_similarity=None, target_embedding=None):
        for name, v in (("input_masks", input_masks), ("attention_similarity", attention_similarity), ("target_embedding", target_embedding)):
            if v is not None:
                raise NotImplementedError(f"SamModel: {name} is not supported (box and point prompts only)")
        if (pixel_values is None) == (image_embeddings is None):
            raise ValueError("SamModel: exactly one of pixel_values and image_embeddings")
        if self.device.type != "cuda":
            raise RuntimeError("theatergen_amd SAM decoder runs on the GPU only (no CPU fallback)")
        dt, dev, cfg = self.dtype, self.device, self.decoder_config
        g, D = cfg.image_embedding_size, cfg.hidden_size
        if image_embeddings is None:
            image_embeddings = self.get_image_embeddings(pixel_values.to(dev))
        if tuple(image_embeddings.shape[1:]) != (D, g, g) or not image_embeddings.is_cuda or image_embeddings.dtype != dt:
            raise ValueError(f"SamModel: image_embeddings must be a {dt} device tensor [B, {D}, {g}, {g}], got {tuple(image_embeddings.shape)} {image_embeddings.dtype}")
        sparse, B, nb, ns = self.prompt_encoder.sparse(self._gauss(), input_points, input_labels, input_boxes, dt, dev)
        if B != image_embeddings.shape[0]:
            raise ValueError(f"SamModel: {image_embeddings.shape[0]} images, prompts for {B}")
        P, n = B * nb, g * g
        x = ops.transpose(image_embeddings.contiguous().reshape(B, D, n), B, D, n).reshape(B * n, D)                             # token-major
        if nb > 1:
            x = x.reshape(B, 1, n, D).expand(B, nb, n, D).reshape(P * n, D)                                                      # one copy per prompt
        kpe, dense = self._dense(P, dt, dev)
        keys = ops.add(x.contiguous(), dense)
        logits, iou = self.mask_decoder.run(keys, kpe, sparse, P, ns, g)
        sl = slice(1, None) if multimask_output else slice(0, 1)
        L = 4 * g
        return SimpleNamespace(pred_masks=logits.view(B, nb, -1, L, L)[:, :, sl].contiguous(), iou_scores=iou.reshape(B, nb, -1)[:, :, sl].contiguous())

    __call__ = forward

    @classmethod
    def from_state_dict(cls, config, state_dict, device="cuda", dtype=torch.bfloat16, decoder_config=None):
        """``config``: the vision config (``sam_vit_h_config()`` ...), or None for a model without the vision encoder (``vision_encoder.*`` keys are then
        unexpected).  ``state_dict``: a whole ``transformers.SamModel`` state dict; ``prompt_encoder.shared_embedding.positional_embedding`` (tied to
        ``shared_image_embedding.positional_embedding``) may be present or not.  A missing or unexpected key is a RuntimeError.  The positional matrix stays fp32."""
        m = cls(config, decoder_config, with_vision=config is not None)
        sd = dict(state_dict)
        tied, shared = "prompt_encoder.shared_embedding.positional_embedding", "shared_image_embedding.positional_embedding"
        if shared in sd and tied not in sd:
            sd[tied] = sd[shared]
        missing, unexpected = m.load_state_dict(sd, strict=False)
        if unexpected or missing:
            raise RuntimeError(f"state dict mismatch: missing {missing[:5]}... unexpected {unexpected[:5]}...")
        gauss = sd[shared].detach().to(device=device, dtype=torch.float32).contiguous()
        m = m.to(device=device, dtype=dtype)
        m.shared_image_embedding.positional_embedding.data = gauss
        m.prompt_encoder.shared_embedding.positional_embedding.data = gauss
        return m
